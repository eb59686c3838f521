"""The line stack on the GPU over the texts of tests/geometry_cases.py: texts at the edges of the line table's geometry (`count` on
both sides of every fence shift and of every step of fm_bits, a boundary at position 0, none at all, nothing but boundaries, none at
the end), texts of period 1 and 2 (every hit overlaps its neighbour, the last windows are cut at textLength) and a text of code
units at and above 0x8000 — where the LDS staging loops, the launchers' n_fences / shift / key_bits, rocPRIM's sorts over exactly
key_bits bits and the clamps of k_line_counts / k_line_compact can go wrong without the log-shaped texts of the other suites
noticing.

One test per text: fmx_line_table_build / _info / fmx_line_bounds_batch, fmx_locate_all_batch, fmx_match_lines_batch,
fmx_match_query_batch, fmx_match_sequence_batch, fmx_field_values_batch, fmx_line_text_batch, their class twins, and the device
forms behind them (the runners of the other GPU suites: outputs prefilled with sentinels, n_hits = hit_off[n] and 37 more).  The
judge works from the Python text alone (geometry_cases.Case); tests/test_text_geometry_cpu.py has proven it against the oracle
and the host mirrors — no text of the table needs the oracle's hits.  The oracle is asked for one thing the text does not say: the
ORDER of a pattern's hits in the packed array (locate()'s).  Options are set inside the tests and put back in `finally`."""
import types

import numpy as np
import pytest

import geometry_cases as gc
import index4j_amd as ia
import orc
from test_field_values_cpu import check_values
from test_gpu_field_values import check as check_dev_values, dev_values
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import options
from test_gpu_match_lines import dev_lines
from test_gpu_match_query import dev_query
from test_gpu_match_sequence import dev_sequence, host_sequence
from test_locate_all_cpu import SENT, expected_packed
from test_match_lines_cpu import check_lines
from test_match_sequence_cpu import check_sequence

pytestmark = pytest.mark.gpu

SR = 4
MAX_LINES = (0, 1, 3)
MAX_LENS = (1, 4, 64)
PAD = 64


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def filled(fm, ch, off, total):
    d = DevAll(fm, ch, off, -1)
    assert d.total == total
    d.fill(0, d.total)
    return d


def sorted_within(locs, hit_off):
    """the packed hits, ascending inside every pattern"""
    which = np.repeat(np.arange(len(hit_off) - 1), np.diff(hit_off))
    return locs[np.lexsort((locs, which))]


_ORDER = {}


def oracle_order(c):
    """the batch's packed hits in the order locate() stores them, once per case"""
    if c.name not in _ORDER:
        _ORDER[c.name] = expected_packed(("text geometry", c.name), orc.OracleFmIndex(c.units(), SR, True), c.ch, c.off, -1)[0]
    return _ORDER[c.name]


def check_hits(got, hits, status, what):
    locs, hit_off, st = got
    want_off = np.concatenate([[0], np.cumsum([len(h) for h in hits])]).astype(np.int64)
    assert (hit_off == want_off).all() and (st == status).all(), what
    total = int(want_off[-1])
    assert (sorted_within(locs[:total], want_off) == np.concatenate(hits + [np.zeros(0, np.int32)])).all(), what
    assert (locs[total:] == SENT).all(), what + ": stored behind hit_off[n]"


def check_dev(dev, want, what, n_hits):
    """a device form's (lines, line_off, line_count); n_hits == 0: the offsets are zeroed and nothing else is written"""
    if n_hits == 0:
        assert (dev[1] == 0).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all() and len(want[0]) == 0, what
    else:
        check_lines(dev, want, what, tail=SENT)


def padded(a, fill=SENT):
    return np.concatenate([a, np.full(PAD, fill, a.dtype)])


def run_case(c, fm, what):
    """every call of the line stack on one resident index of the case's text, whole arrays against the judge"""
    assert fm.build_line_table(gc.NL) == c.n_lines
    info = fm.line_table_info()
    assert info[:2] == (10, c.count) and info[2] >= 4 * c.count
    ids = np.arange(-1, c.n_lines + 1, dtype=np.int32)
    start, stop = fm.line_bounds(ids)
    es, ee = c.bounds(ids)
    assert (start == es).all() and (stop == ee).all(), what + ": line_bounds"
    # every hit, packed
    hits, total = c.hits(), sum(len(h) for h in c.hits())
    locs, hit_off, st = fm.locate_all_batch(c.ch, c.off)
    check_hits((padded(locs), hit_off, st), hits, c.status, what + ": locate_all, host form")
    d = filled(fm, c.ch, c.off, total)
    dl, dho, dst, _ = d.result()
    check_hits((dl, dho, dst), hits, c.status, what + ": locate_all, device form")
    assert (locs == oracle_order(c)).all() and (dl[:total] == oracle_order(c)).all(), what + ": the order of the hits"
    # the lines of every pattern and of every query
    q = len(c.query_off) - 1
    qb = types.SimpleNamespace(n=c.n, q=q, query_off=c.query_off, kinds=c.kinds)
    occ_want = np.array([len(h) for h in hits], np.int32)
    for max_lines in MAX_LINES:
        w = "%s max_lines %d" % (what, max_lines)
        want = c.lines(max_lines)
        lines, line_off, st, line_count, occ = fm.match_lines_batch(c.ch, c.off, max_lines, want_counts=True)
        check_lines((padded(lines), line_off, line_count), want, w + ": match_lines, host form", tail=SENT)
        assert (st == c.status).all() and (occ == occ_want).all(), w
        wantq = c.queries(max_lines)
        lines, line_off, st, line_count, occ = fm.match_query_batch(c.ch, c.off, c.query_off, c.kinds, max_lines, want_counts=True)
        check_lines((padded(lines), line_off, line_count), wantq, w + ": match_query, host form", tail=SENT)
        assert (st == c.status).all() and (occ == occ_want).all(), w
        for extra in (0, 37):
            rc, dev = dev_lines(d, max_lines, extra_hits=extra)
            assert rc == 0, last_error()
            check_dev(dev, want, "%s: lines, device form, %d slots behind the hits" % (w, extra), total + extra)
            rc, dev = dev_query(d, qb, max_lines, extra_hits=extra)
            assert rc == 0, last_error()
            check_dev(dev, wantq, "%s: queries, device form, %d slots behind the hits" % (w, extra), total + extra)
    # the lines that hold a sequence of terms in order, with and without spans
    seq_hits = c.seq_hits()
    seq_total = sum(len(h) for h in seq_hits)
    seq_status = np.array([0 if t else 9 for t in c.seq_terms], np.int32)
    sb = types.SimpleNamespace(ch=c.seq_ch, off=c.seq_pat_off, n=len(c.seq_terms), q=len(c.sequences), query_off=c.seq_off,
                               term_len=np.diff(c.seq_pat_off).astype(np.int32), total=seq_total)
    ds = filled(fm, sb.ch, sb.off, seq_total)
    for max_lines in MAX_LINES:
        w = "%s max_lines %d" % (what, max_lines)
        want = c.sequence_packed(max_lines)
        got, spans, st, occ = host_sequence(fm, sb, max_lines)
        check_sequence(got, spans, want, w + ": match_sequence, host form")
        assert (st == seq_status).all() and (occ == [len(h) for h in seq_hits]).all(), w
        got, none, _, _ = host_sequence(fm, sb, max_lines, want_spans=False)
        check_sequence(got, None, want, w + ": match_sequence without spans, host form")
        for extra, want_spans in ((0, True), (37, True), (0, False)):
            rc, dev, dspans = dev_sequence(ds, sb, max_lines, extra_hits=extra, want_spans=want_spans)
            assert rc == 0, last_error()
            if seq_total + extra == 0:
                check_dev(dev, want[0], w + ": sequences, device form", 0)
                assert (dspans == SENT).all()
            else:
                check_sequence(dev, dspans if want_spans else None, want, "%s: sequences, device form, %d slots behind, spans %r" % (w, extra, want_spans))
                assert want_spans or (dspans == SENT).all()
    # the values that follow every pattern
    for stop_set in c.stops:
        for k, max_len in enumerate(MAX_LENS):
            w = "%s stop %r max_len %d" % (what, stop_set, max_len)
            want = c.values(stop_set, max_len)
            chars, text_off, counts, val_off, st, occ = fm.field_values_batch(c.ch, c.off, stop_set, max_len)
            check_values((chars, text_off, counts, val_off), want, w + ": field_values, host form")
            assert len(counts) == want.val_off[-1] and len(chars) == want.text_off[-1] and (st == c.status).all() and (occ == occ_want).all(), w
            rc, dev, dst = dev_values(d, c.lens, gc.units(stop_set), max_len, extra_hits=37 * (k % 2))
            assert rc == 0, last_error()
            check_dev_values(dev, want, w + ": values, device form")
            assert (dst == c.status).all(), w
    # the text of the lines
    ids = c.line_ids()
    chars, text_off, st = fm.line_text_batch(ids)
    texts = c.line_texts(ids)
    assert (st == 0).all() and (np.diff(text_off) == [len(s) for s in texts]).all() and (chars == gc.units("".join(texts))).all(), what + ": line_text"
    chars, text_off, st = fm.line_text_batch(np.array([-1, c.n_lines], np.int32))
    assert len(chars) == 0 and (text_off == 0).all() and (st == 2).all(), what + ": line_text of ids that are no lines"
    # the class twins, on the any-case / partner form of the same batch
    chits = c.hits(any_case=True)
    cocc = np.array([len(h) for h in chits], np.int32)
    locs, hit_off, st = fm.locate_all_class_batch(*c.class_arrays)
    check_hits((padded(locs), hit_off, st), chits, c.status, what + ": locate_all, class form")
    for max_lines in (0, 3):
        want = c.queries(max_lines, any_case=True)
        lines, line_off, st, line_count, occ = fm.match_query_class_batch(*c.class_arrays, c.query_off, c.kinds, max_lines, want_counts=True)
        check_lines((padded(lines), line_off, line_count), want, "%s max_lines %d: match_query, class form" % (what, max_lines), tail=SENT)
        assert (st == c.status).all() and (occ == cocc).all()
        want = c.sequence_packed(max_lines, any_case=True)
        out = fm.match_sequence_class_batch(*c.seq_classes, c.seq_off, max_lines, want_counts=True, want_spans=True)
        check_sequence((padded(out[0]), out[1], out[3]), padded(out[5].reshape(-1)), want, "%s max_lines %d: match_sequence, class form" % (what, max_lines))
        assert (out[2] == seq_status).all() and (out[4] == [len(h) for h in c.seq_hits(any_case=True)]).all()
    for stop_set in c.stops:
        want = c.values(stop_set, 4, any_case=True)
        chars, text_off, counts, val_off, st, occ = fm.field_values_class_batch(*c.class_arrays, stop_set, 4)
        check_values((chars, text_off, counts, val_off), want, "%s stop %r: field_values, class form" % (what, stop_set))
        assert len(counts) == want.val_off[-1] and len(chars) == want.text_off[-1] and (st == c.status).all() and (occ == cocc).all()
    return total, seq_total


@pytest.mark.parametrize("name", gc.names())
def test_text(name):
    c = gc.case(name)
    fm = ia.FmIndex(c.units(), SR, True, device=0)
    try:
        assert fm.line_table_info() == (-1, 0, 0)
        total, seq_total = run_case(c, fm, name)
        if name == "only_boundary_no_hits":  # the n_hits <= 0 early return of every launcher: empty answers, status 0
            assert total == 0 == seq_total and (c.status == 0).all() and all(c.seq_terms) and len(c.lines(0)[0]) == 0 and c.values(gc.NL, 4).val_off[-1] == 0
    finally:
        fm.close()


@pytest.mark.parametrize("cells,rows,compact", [(1, 1, 0), (2, 0, 1)])  # (the default residency: test_text)
@pytest.mark.parametrize("name", gc.RESIDENT)
def test_residencies(name, cells, rows, compact):
    c = gc.case(name)
    with options(window_cells=cells, locate_rows=rows, image_compact=compact):
        fm = ia.FmIndex(c.units(), SR, True, device=None)
        fm.blob()  # flattened under the option
        fm.to_device(0)
    try:
        assert (fm.locate_rows_info()[0] > 0) == bool(rows)
        run_case(c, fm, "%s, window_cells %d locate_rows %d compact %d" % (name, cells, rows, compact))
    finally:
        fm.close()

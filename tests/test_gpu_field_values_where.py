"""Field values and hits only within the lines of a query on the GPU (grep terminating | grep -o 'blk_[^ ]*' | sort | uniq -c): packed
hits -> the packed hits that lie in given lines (fmx_hits_in_lines_dev: the kernels of fmx_hit_filter.hip around rocPRIM's scan) and
the host forms fmx_field_values_where_batch / fmx_field_values_where_class_batch, with their Python and C++ mirrors.

The judge is Python over the oracle (tests/test_field_values_where_cpu.py: Where — expected_packed's hits, judge_table / judge_lines
and set algebra for the lines of the queries, np.searchsorted on the line table for the filter, judge_values on what is left),
computed once per batch.  Outputs are prefilled with a sentinel, and everything behind the answer must keep it.  The kept hits are
compared IN ORDER (check_kept): the compaction is stable.  Options are set inside the tests and put back in `finally`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from geometry_cases import count_text
from test_field_values_cpu import judge_values
from test_field_values_where_cpu import EVERY_LINE, INT32_MAX, NAMED, SYNTH, Trimmed, Where, assert_named, check_kept
from test_gpu_field_values import SENT64, ST_NOT_ENABLED, ST_TOO_MANY, check, last_error, padded
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import _torch, options
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table, texts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel


class Filled:
    """the two packed locate stages over a batch (a Where's terms + value patterns, or plain arrays): every hit on the device"""

    def __init__(self, fm, ch, off):
        self.d = DevAll(fm, np.array(ch, np.uint16), np.array(off, np.int32), -1)  # (copies: the judge's arrays are read-only)
        self.d.fill(0, self.d.total)
        self.fm, self.total, self.torch = fm, self.d.total, self.d.torch


def dev_filter(f, n_terms, n, where_of, q, line_off, lines, window=EVERY_LINE, n_hits=None, ws_bytes=None):
    """fmx_hits_in_lines_dev over the value patterns' part of a Filled block (hit_off + n_terms: it does not start at 0 when a term
    has a hit).  n_hits: the slots of the block the call may look at (default: all hits; up to 64 more: slots without a hit).
    Returns rc, (kept_off, kept_locs)"""
    torch, d = f.torch, f.d
    n_hits = f.total if n_hits is None else n_hits
    assert n_hits <= f.total + 64  # (d.locs has that many slots behind the hits)
    need = ia.lib.fmx_hits_in_lines_scratch_bytes(n, n_hits)
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    d_loff = torch.from_numpy(np.array(line_off, np.int64)).cuda()
    d_lines = torch.from_numpy(np.concatenate([lines, np.full(1, SENT, np.int32)]).astype(np.int32)).cuda()
    kept_off = torch.full((n + 1,), SENT64, dtype=torch.int64, device="cuda")
    kept_locs = torch.full((n_hits + PAD,), SENT, dtype=torch.int32, device="cuda")
    wo = np.array(where_of, np.int32)  # the call's own copy: scribbled over once it is back
    rc = ia.lib.fmx_hits_in_lines_dev(f.fm.handle, n, wo.ctypes.data, q, d_loff.data_ptr(), d_lines.data_ptr(), window[0], window[1],
                                      d.hit_off.data_ptr() + 8 * n_terms, d.locs.data_ptr(), n_hits, kept_off.data_ptr(), kept_locs.data_ptr(),
                                      ws.data_ptr(), use, d.stream)
    wo[:] = -9  # (the call has copied what it needs before it returns)
    torch.cuda.synchronize()
    return rc, (kept_off.cpu().numpy(), kept_locs.cpu().numpy())


def dev_where(f, w, **kw):
    return dev_filter(f, w.n_terms, w.n, w.where_of, w.q, w.line_off, w.lines, w.window, **kw)


def host_where(fm, w, stop, max_len):
    """the host form over a Where's arrays; ((chars, text_off, counts, val_off) with sentinels behind, status, occurrences, kept,
    term_status)"""
    out = fm.field_values_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, stop, max_len,
                                      None if w.window == EVERY_LINE else w.window)
    chars, text_off, counts, val_off, st, occ, kept, tst = out
    return padded(chars, text_off, counts, val_off), st, occ, kept, tst


def check_host(got, w, what):
    vals, st, occ, kept, tst = got
    check(vals, w.values, what)
    assert (kept == w.kept).all(), "%s: kept %r, expected %r" % (what, kept[:6], w.kept[:6])
    assert (occ == w.occurrences).all() and (st == w.status[w.n_terms:]).all() and (tst == w.term_status).all(), what
    per_pattern = [int(vals[2][a:b].sum()) for a, b in zip(w.values.val_off[:-1], w.values.val_off[1:])]
    assert per_pattern == kept.tolist(), what + ": the counts of a pattern's values add up to kept"


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


MIX_QUERIES = [dict(all=["terminating"]), dict(all=["blk_"], none=["PacketResponder"]), dict(all=["zzzq#"]), dict(none=["INFO"]), dict(),
               dict(any=["WARN", "Receiving"], none="src:")]
MIX_PATTERNS = ["blk_", "/10.", "INFO ", "WARN", " ", "1", "blk_", "zzzq#", "dfs.", ":", ""]
MIX_WHERE = [0, 0, 1, -1, 2, 3, 4, 0, 5, -1, 1]


def test_device_stage_on_the_tile_edges(hd):
    """value hits trimmed to 0, 1, 1,023, 1,024, 1,025 and to whole tiles of slots, several tiles, slots behind the hits; with terms
    in front of the value patterns (hit_off[0] != 0) and without; the kept hits in order, sentinels behind"""
    o, fm, T = hd
    for queries, where_of in (([], [-1, -1, -1, -1, -1]), ([dict(all=["terminating"]), dict(any=["WARN", "/10.250.1"])], [1, 0, -1, 0, 1])):
        w = Where("hd16 edges", o, T, [" ", "blk_", "zzzq#", "", "1"], queries, where_of, (3, 1990))
        f = Filled(fm, w.ch, w.off)
        first, total = int(w.hit_off[w.n_terms]), int(w.hit_off[-1])
        assert f.total == total and total - first > 5 * 1024 and (first > 0) == bool(queries)
        edges = [first + k for k in (1, 1023, 1024, 1025)] + [1024 * (first // 1024 + 1), 1024 * (first // 1024 + 3) + 1, total - 1]
        for n_hits in edges:
            t = Trimmed(w, n_hits)
            rc, got = dev_where(f, w, n_hits=n_hits)
            assert rc == 0, last_error()
            check_kept(got, t, "n_hits %d of %d, %d in front" % (n_hits, total, first), tail=SENT)
        for n_hits in (total, total + 37):
            rc, got = dev_where(f, w, n_hits=n_hits)
            assert rc == 0, last_error()
            check_kept(got, w, "n_hits %d of %d" % (n_hits, total), tail=SENT)
        assert 0 < w.kept.sum() < total - first
        # stable: the order the hits had (SA-row order), which is not the text's
        assert not (np.diff(w.kept_locs[:w.kept[0]]) > 0).all()
        if first:  # no value hit inside the slots: every offset 0, nothing stored
            rc, got = dev_where(f, w, n_hits=first)
            assert rc == 0 and (got[0] == 0).all() and (got[1] == SENT).all(), last_error()
    # n_hits == 0 and n == 0: the offsets are zeroed and nothing else is written
    rc, got = dev_where(f, w, n_hits=0)
    assert rc == 0 and (got[0] == 0).all() and (got[1] == SENT).all(), last_error()
    rc, got = dev_filter(f, w.n_terms, 0, [], w.q, w.line_off, w.lines)
    assert rc == 0 and got[0].tolist() == [0] and (got[1] == SENT).all(), last_error()


def test_where_of_mixes_and_windows(hd):
    o, fm, T = hd
    w = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    f = Filled(fm, w.ch, w.off)
    rc, got = dev_where(f, w)
    assert rc == 0, last_error()
    check_kept(got, w, "where_of mix", tail=SENT)
    assert w.kept[0] == 310 and w.kept[2] == 1317 and w.kept[3] == w.occurrences[3] > 0 and w.kept[4:8].sum() == 0 and w.status[-1] == 9
    n_lines = 2000
    for window in ((7, 7), (0, 1), (n_lines - 1, n_lines), (n_lines + 5, INT32_MAX), (100, 1900)):
        ww = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, window)
        rc, got = dev_where(f, ww)
        assert rc == 0, last_error()
        check_kept(got, ww, "window %r" % (window,), tail=SENT)
        assert (ww.kept.sum() == 0) == (window[0] == window[1] or window[0] > n_lines)


def test_grid_stride_loops_run_more_than_once(hd):
    """(" ", "1", "0") together, the batch repeated until its slots are more than the grids of fmx_hit_lines_geometry cover in one
    pass (they do not depend on the options; the stage runs under groups_per_cu=1 as the other hit stages' tests do)"""
    o, fm, T = hd
    w = Where("hd16 heavy", o, T, [" ", "1", "0"], [dict(all=["terminating"]), dict(any=["WARN", "/10.250.1"])], [0, -1, 1], (2, 1999))
    per = int(w.hit_off[-1] - w.hit_off[w.n_terms])
    key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
    assert ia.lib.fmx_hit_lines_geometry(fm.handle, 10 ** 9, C.byref(key_grid), C.byref(flat_grid)) == 0  # (the caps)
    reps = max(key_grid.value * 1024, flat_grid.value * 256) // per + 2
    nt = w.n_terms
    pats = [w.ch[w.off[i]:w.off[i + 1]] for i in range(nt + w.n)]
    ch, off = ia.pack_patterns(pats[:nt] + pats[nt:] * reps)
    with options(groups_per_cu=1):
        f = Filled(fm, ch, off.astype(np.int32))
        assert f.total == int(w.hit_off[nt]) + reps * per
        assert ia.lib.fmx_hit_lines_geometry(fm.handle, f.total, C.byref(key_grid), C.byref(flat_grid)) == 0
        assert key_grid.value * 1024 < f.total and flat_grid.value * 256 < f.total  # every loop runs more than once
        rc, got = dev_filter(f, nt, w.n * reps, w.where_of.tolist() * reps, w.q, w.line_off, w.lines, w.window)
    assert rc == 0, last_error()

    class Tiled:
        kept_off = np.concatenate([[0], np.cumsum(np.tile(w.kept, reps))]).astype(np.int64)
        kept_locs = np.tile(w.kept_locs, reps)

    check_kept(got, Tiled, "%d hits in %d patterns" % (f.total, w.n * reps), tail=SENT)
    assert w.kept.min() > 0 and (w.kept < w.occurrences).any()


def test_workspace_one_byte_short(hd):
    o, fm, T = hd
    w = Where("hd16", o, T, ["blk_"], [NAMED[0][3]], [0])
    f = Filled(fm, w.ch, w.off)
    need = ia.lib.fmx_hits_in_lines_scratch_bytes(w.n, f.total)
    assert need > 8 * f.total and need % 256 == 0
    rc, got = dev_where(f, w, ws_bytes=need - 1)
    assert rc == ia._lib.E_ARG and "fmx_hits_in_lines_scratch_bytes" in last_error()
    assert (got[0] == SENT64).all() and (got[1] == SENT).all()  # nothing launched, nothing written
    rc, got = dev_where(f, w, ws_bytes=need)
    assert rc == 0, last_error()
    check_kept(got, w, "the exact workspace", tail=SENT)


def line_search_texts():
    t = texts()
    return {"a few lines": t["empty lines"], "the fixture, last line unterminated": t["hdfs, last line unterminated"],
            "more lines than the fences hold": (count_text(8193, False), "\n")}


@pytest.mark.parametrize("name", sorted(line_search_texts()))
def test_line_search_paths(name):
    """fm_line_of inside the flag kernel: a table of a few entries, one entry per fence (the fixture of test_match_lines_cpu.texts(),
    2,000 lines), and more entries than the 4,096 fences hold (tests/geometry_cases.py's 8,194 lines: shift 2, the last levels over
    the table itself)"""
    text, boundary = line_search_texts()[name]
    t16 = ia.as_chars(text)
    o = orc.OracleFmIndex(text, 4 if len(text) < 100 else 16, True)
    T = judge_table(o, boundary)
    fm = ia.FmIndex(text, 4 if len(text) < 100 else 16, True, device=0)
    try:
        n_lines = fm.build_line_table(boundary)
        assert n_lines == judge_n_lines(T, len(text)) and (len(T) > 4096) == name.startswith("more")
        units = [np.array([u], np.uint16) for u in np.unique(t16)[:6]]
        some = t16[len(t16) // 2:len(t16) // 2 + 2]
        queries = [dict(all=[units[0]]), dict(any=[units[1], some], none=[units[0]])]
        patterns = units + [some, np.array([ord(boundary)], np.uint16)]
        where_of = [(-1, 0, 1)[i % 3] for i in range(len(patterns))]
        for window in (EVERY_LINE, (1, n_lines - 1), (n_lines - 1, n_lines), (n_lines // 2, n_lines // 2 + 1)):
            w = Where(name, o, T, patterns, queries, where_of, window, " \n", 4)
            rc, got = dev_where(Filled(fm, w.ch, w.off), w)
            assert rc == 0, last_error()
            check_kept(got, w, "%s, window %r" % (name, window), tail=SENT)
            check_host(host_where(fm, w, " \n", 4), w, "%s, window %r, host form" % (name, window))
        assert w.kept.sum() > 0
    finally:
        fm.close()


def test_host_forms_named_cases_and_mirrors(hd):
    o, fm, T = hd
    for pattern, stop, max_len, query, hits, kept, values, top in NAMED:
        w = Where("hd16", o, T, [pattern], [query], [0], EVERY_LINE, stop, max_len)
        assert_named(w, hits, kept, values, top)
        check_host(host_where(fm, w, stop, max_len), w, "named %r" % pattern)
        pairs = fm.field_values(pattern, stop=stop, max_len=max_len, where=query)
        assert pairs == w.values.strings(0) and sum(c for _, c in pairs) == kept and len(pairs) == values
        by_count = sorted(w.values.strings(0), key=lambda vc: (-vc[1], vc[0]))
        assert fm.field_values(pattern, stop=stop, max_len=max_len, where=query, top=2) == by_count[:2]
        if top:
            assert fm.field_values(pattern, stop=stop, max_len=max_len, where=query, top=len(top)) == top
        assert fm.count_where(pattern, where=query) == kept and fm.count_where(pattern) == hits
        ww = Where("hd16", o, T, [pattern], [query], [0], (100, 1500), stop, max_len)
        assert fm.field_values(pattern, stop=stop, max_len=max_len, where=query, lines=(100, 1500)) == ww.values.strings(0)
        assert fm.count_where(pattern, where=query, lines=(100, 1500)) == ww.kept[0] < kept
        w0 = Where("hd16", o, T, [pattern], [], [-1], (100, 1500), stop, max_len)
        assert fm.field_values(pattern, stop=stop, max_len=max_len, lines=(100, 1500)) == w0.values.strings(0)
    assert fm.field_values("blk_", where=dict(none=["INFO"])) == [] and fm.count_where("blk_", where=dict(all="zzzq#")) == 0
    assert fm.field_values("zzzq#", where=dict(all="INFO")) == []
    # the whole mix in one call: -1, a query shared by patterns, a query without lines, NONE only, no terms, an empty pattern
    for window in (EVERY_LINE, (0, 1), (1999, 2000), (2005, INT32_MAX), (7, 7)):
        w = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, window, " \n:", 12)
        check_host(host_where(fm, w, " \n:", 12), w, "mix, window %r" % (window,))
    assert w.status[-1] == 9  # (the empty pattern keeps FMX_ST_JAVA_AIOOBE)
    out = fm.field_values_where_batch(np.zeros(0, np.uint16), [0], *ia.pack_patterns(["INFO"]), [0, 1], [0], [], " ", 8)
    assert len(out[2]) == 0 and list(out[3]) == [0] and list(out[7]) == [0]


def test_synthetic_text_host_form():
    o = orc.OracleFmIndex(SYNTH, 4, True)
    T = judge_table(o, "\n")
    fm = ia.FmIndex(SYNTH, 4, True, device=0)
    try:
        assert fm.build_line_table("\n") == 41
        for stop in (" \n", " "):
            w = Where("synth", o, T, ["k=", "\nk=", "k=", "keep"], [dict(all=["keep"]), dict(all=["drop"])], [0, 0, 1, -1], EVERY_LINE, stop, 8)
            check_host(host_where(fm, w, stop, 8), w, "synth, stop %r" % stop)
            rc, got = dev_where(Filled(fm, w.ch, w.off), w)
            assert rc == 0, last_error()
            check_kept(got, w, "synth, device stage", tail=SENT)
        assert w.kept.tolist() == [43, 20, 40, 21]
        assert dict(fm.field_values("k=", stop=" \n", max_len=8, where=dict(all="keep")))["end"] == 1
        assert fm.count_where("k=", where=dict(all="keep"), lines=(40, 41)) == 3 and fm.count_where("k=", lines=(0, 1)) == 2
    finally:
        fm.close()


def test_class_form(hd):
    o, fm, T = hd
    words, term_words = ["block", "info "], ["TERMINATING", "packetresponder", "Blk_"]
    queries, where_of = [dict(all=[term_words[0]]), dict(all=[term_words[2]], none=[term_words[1]])], [0, 1]
    # the judge over the union of the spellings' hits: every spelling the text holds, as a literal (tests/test_gpu_field_values.py)
    spell = lambda word: sorted(set(re.findall("(?i)" + re.escape(word), HD)))  # noqa: E731
    assert len(spell("block")) > 1
    lit_queries = [dict(any=spell(term_words[0])), dict(any=spell(term_words[2]), none=spell(term_words[1]))]
    flat = [s for word in words for s in spell(word)]
    lit = Where("hd16 spellings", o, T, flat, lit_queries, [where_of[i] for i, word in enumerate(words) for _ in spell(word)])
    bounds = np.concatenate([[0], np.cumsum([len(spell(word)) for word in words])])
    kept_off = lit.kept_off[bounds]
    want = judge_values(o, lit.kept_locs, kept_off, [len(word) for word in words], " \n:", 20)
    kinds = np.array([0, 0, 2], np.uint8)  # (the class form's terms, query after query: TERMINATING | Blk_, not packetresponder)
    term_arrays = ia.pack_class_patterns([ia.ignore_case(x) for x in (term_words[0], term_words[2], term_words[1])])
    klass = ia.pack_class_patterns([ia.ignore_case(x) for x in words]) + term_arrays
    out = fm.field_values_where_class_batch(*klass, [0, 1, 3], kinds, where_of, " \n:", 20)
    chars, text_off, counts, val_off, st, occ, kept, tst = out
    check(padded(chars, text_off, counts, val_off), want, "class form")
    assert (kept == np.diff(kept_off)).all() and kept[0] < occ[0] == 2662 and (st == 0).all() and (tst == 0).all()
    assert fm.field_values("BLOCK", stop=" \n:", max_len=20, ignore_case=True, where=dict(all="TERMINATING")) == want.strings(0)
    assert fm.count_where("INFO ", where=dict(all="BLK_", none="PACKETRESPONDER"), ignore_case=True) == kept[1]
    assert fm.field_values("BLOCK", stop=" \n:", max_len=20, where=dict(all="terminating")) == []  # (no such spelling in the text)
    # a term whose frontier is larger than max_ranges has no hits, as in fmx_match_query_class_batch: its ALL query has no lines
    _, cst = fm.count_class_batch(*term_arrays, max_ranges=1)
    assert cst[0] == ST_TOO_MANY
    out = fm.field_values_where_class_batch(*klass, [0, 1, 3], kinds, where_of, " \n:", 20, max_ranges=1)
    assert out[7][0] == ST_TOO_MANY and out[6][0] == 0 and out[3][1] == 0


def test_unfiltered_call_is_field_values_batch(hd):
    """every where_of negative and no window: array for array fmx_field_values_batch's answer — also on an index without a line
    table, which returns FMX_E_ARG only when a filter or a window is asked for"""
    o, fm, T = hd
    bare = ia.FmIndex(HD, 16, True, device=0)
    try:
        pats = ["blk_", "", "INFO ", "zzzq#", " ", "/10."]
        ch, off = ia.pack_patterns(pats)
        tch, toff = ia.pack_patterns(["terminating", "WARN"])
        for index in (fm, bare):
            plain = index.field_values_batch(ch, off, " \n:", 16)
            got = index.field_values_where_batch(ch, off, tch, toff, [0, 1, 2], [0, 1], [-1] * len(pats), " \n:", 16)
            for a, b in zip(plain, got[:6]):
                assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
            assert (got[6] == plain[5]).all() and (got[7] == 0).all()
            got = index.field_values_where_batch(ch, off, tch[:0], [0], [0], [], [-1] * len(pats), " \n:", 16, lines=EVERY_LINE)
            assert all((a == b).all() for a, b in zip(plain, got[:6]))
            kl = ia.pack_class_patterns([ia.ignore_case(p) for p in pats if p])
            plain = index.field_values_class_batch(*kl, " \n:", 16)
            got = index.field_values_where_class_batch(*kl, *ia.pack_class_patterns([ia.ignore_case("warn")]), [0, 1], [1], [-1] * 5, " \n:", 16)
            assert all(a.shape == b.shape and (a == b).all() for a, b in zip(plain, got[:6])) and (got[6] == plain[5]).all()
        for kw in (dict(where_of=[0] + [-1] * 5), dict(lines=(0, 5)), dict(lines=(0, INT32_MAX - 1))):
            with pytest.raises(ia.FmxError) as e:
                bare.field_values_where_batch(ch, off, tch, toff, [0, 1, 2], [0, 1], kw.get("where_of", [-1] * 6), " \n:", 16, lines=kw.get("lines"))
            assert e.value.code == ia._lib.E_ARG and "fmx_line_table_build" in str(e.value)
        torch = _torch()
        p = torch.zeros(64, dtype=torch.int64, device="cuda")
        wo = np.array([-1], np.int32)
        args = (1, wo.ctypes.data, 0, p.data_ptr(), p.data_ptr(), 0, INT32_MAX, p.data_ptr(), p.data_ptr(), 5, p.data_ptr(), p.data_ptr(), p.data_ptr(), 512, None)
        assert ia.lib.fmx_hits_in_lines_dev(bare.handle, *args) == ia._lib.E_ARG and "fmx_line_table_build" in last_error()  # the device stage: always
        torch.cuda.synchronize()
        assert int(p.cpu().abs().sum()) == 0
    finally:
        bare.close()


def test_index_without_extraction(hd):
    o, fm0, T = hd
    fm = ia.FmIndex(HD, 16, False, device=0)
    try:
        fm.build_line_table("\n")
        w = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
        out = fm.field_values_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, " \n", 8)
        chars, text_off, counts, val_off, st, occ, kept, tst = out
        assert (st == ST_NOT_ENABLED).all() and (val_off == 0).all() and len(counts) == 0 and len(chars) == 0
        assert (kept == w.kept).all() and kept[0] == 310 and (occ == w.occurrences).all() and (tst == w.term_status).all()
        assert fm.count_where("blk_", where=dict(all="terminating")) == 310
        with pytest.raises(RuntimeError):
            fm.field_values("blk_", where=dict(all="terminating"))
    finally:
        fm.close()


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_field_values_where_mirror.cpp prints what fieldValuesWhereBatch / fieldValuesWhere return"""
    o, fm, T = hd
    exe = str(tmp_path / "test_field_values_where_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_field_values_where_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    stop = " \t\r\n:"
    w = Where("hd16 mirror", o, T, ["blk_", "INFO ", "zzqq#", "INFO "], [NAMED[0][3], NAMED[1][3]], [0, 1, 0, -1], EVERY_LINE, stop, 32)
    want = w.values
    assert out["batch_val_off"] == list(want.val_off) and out["batch_counts"] == list(want.counts)
    assert out["batch_text_off"] == list(want.text_off) and out["batch_chars"] == list(want.chars)
    assert out["batch_occurrences"] == list(w.occurrences) == [2468, 1920, 0, 1920] and out["batch_kept"] == list(w.kept) == [310, 1317, 0, 1920]
    assert out["batch_status"] == [0, 0, 0, 0] and out["batch_term_status"] == [0, 0, 0]
    top = sorted(want.per[1], key=lambda vc: (-vc[1], vc[0]))[:2]
    assert out["one_counts"] == [c for _, c in want.per[1]] and out["top_counts"] == [c for _, c in top] and top[0][1] == 525
    assert out["top_chars"] == [u for v, _ in top for u in v]
    assert out["window_kept"] == [int(Where("hd16", o, T, ["blk_"], [], [-1], (100, 200)).kept[0])]

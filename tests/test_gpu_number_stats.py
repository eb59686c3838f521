"""Statistics of the number behind a pattern, per bucket of lines, on the GPU: packed hits -> rows of n x B (count, the exact
128-bit sum, min, max, nearest-rank percentiles) and the per-pattern counters (fmx_numbers_of_hits_dev: the kernels of
fmx_hit_numbers.hip around the packed extract, rocPRIM's radix sorts and scans) and the host forms fmx_number_stats_where_batch /
fmx_number_stats_where_class_batch with their Python and C++ mirrors.

The judge is judge_numbers (tests/test_number_stats_cpu.py): the oracle's windows, Python's integers, Where's kept hits
(tests/test_field_values_where_cpu.py), judge_bins' buckets (tests/test_line_histogram_cpu.py), computed once per batch.  Every
output is prefilled with a sentinel and padded, and what lies behind the answer must keep it.  Options are set inside the tests and
put back in `finally`.  Every refused call returns before a launch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_where_cpu import EVERY_LINE, Trimmed, Where
from test_gpu_field_values import ST_NOT_ENABLED, ST_TOO_MANY, last_error
from test_gpu_field_values_where import MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, Filled
from test_gpu_line_histogram import many_edges
from test_gpu_locate_rows import _torch, options, run_block_text
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_stats_cpu import (FRACS, NAN, OVER, P5, assert_fixture_figures, check_numbers, judge_numbers, judge_where_numbers, parser_text,
                                   segments_text)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel
NAMES = ("count", "sum_lo", "sum_hi", "min", "max", "pct", "not_number", "overflow")
P16 = tuple(range(0, 1000, 63))


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def dev_numbers(fm, n, d_hit_off_ptr, d_locs_ptr, n_hits, lens, edges=None, permille=(500, 950), frac_digits=0, d_status_ptr=None, ws_bytes=None,
                skip=()):
    """fmx_numbers_of_hits_dev; rc, a dict of the outputs cut to the answer's sizes — what lies behind them has kept the sentinel
    (asserted).  skip: outputs handed in as NULL"""
    torch = _torch()
    B, P = (1 if edges is None else len(edges) - 1), len(permille)
    need = ia.lib.fmx_numbers_of_hits_scratch_bytes(n, n_hits, 0 if edges is None else len(edges), P)
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    sizes = dict(count=n * B, sum_lo=n * B, sum_hi=n * B, min=n * B, max=n * B, pct=n * B * P, not_number=n, overflow=n)
    out = {k: torch.full((sizes[k] + PAD,), SENT, dtype=torch.int32 if k in ("count", "not_number", "overflow") else torch.int64, device="cuda")
           for k in NAMES}
    e = None if edges is None else np.array(edges, np.int32)  # the call's own copies: scribbled over once it is back
    tl, pm = np.array(lens, np.int32), np.array(permille, np.int32)
    ptr = lambda k: None if k in skip else out[k].data_ptr()  # noqa: E731
    rc = ia.lib.fmx_numbers_of_hits_dev(fm.handle, n, tl.ctypes.data, d_hit_off_ptr, d_locs_ptr, n_hits, None if e is None else e.ctypes.data,
                                        0 if e is None else len(e), frac_digits, pm.ctypes.data if P else None, P, *(ptr(k) for k in NAMES),
                                        d_status_ptr, ws.data_ptr(), use, stream())
    tl[:] = -9  # (the call has copied what it needs before it returns)
    pm[:] = -9
    if e is not None:
        e[:] = -9
    torch.cuda.synchronize()
    got = {}
    for k in NAMES:
        a = out[k].cpu().numpy()
        assert (a[sizes[k]:] == SENT).all(), "stored beyond the answer: " + k
        assert k not in skip or (a == SENT).all(), "stored through a NULL's neighbour: " + k
        got[k] = a[:sizes[k]].view(np.uint64) if k.startswith("sum") else a[:sizes[k]]
    return rc, got


def untouched(got):
    return all((np.asarray(v).view(np.int64 if v.dtype.itemsize == 8 else np.int32) == SENT).all() for v in got.values())


def dev_block(f, n_terms, n, lens, edges=None, permille=(500, 950), frac_digits=0, n_hits=None, **kw):
    """... over the value patterns' part of a Filled block (hit_off + n_terms: it does not start at 0 when a term has a hit).
    n_hits: the slots of the block the call may look at (default: all hits; up to 64 more: slots without a hit)"""
    n_hits = f.total if n_hits is None else n_hits
    assert n_hits <= f.total + 64  # (d.locs has that many slots behind the hits)
    return dev_numbers(f.fm, n, f.d.hit_off.data_ptr() + 8 * n_terms, f.d.locs.data_ptr(), n_hits, lens, edges, permille, frac_digits,
                       d_status_ptr=f.d.st.data_ptr() + 4 * n_terms, **kw)


def host_numbers(fm, w, edges=None, permille=(500, 950), frac_digits=0):
    return fm.number_stats_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, edges, permille, frac_digits)


def check_host(fm, o, w, T, edges=None, permille=(500, 950), frac_digits=0, what=""):
    """the host form against the judge, and the invariant against fmx_hit_histogram_where_batch on the same call"""
    want = judge_where_numbers(o, w, T, edges, permille, frac_digits)
    got = host_numbers(fm, w, edges, permille, frac_digits)
    check_numbers(got, want, what)
    assert (got["kept"] == w.kept).all() and (got["occurrences"] == w.occurrences).all() and (got["status"] == w.status[w.n_terms:]).all(), what
    assert (got["term_status"] == w.term_status).all(), what
    hist = fm.hit_histogram_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, [0, 2 ** 31 - 1] if edges is None else edges)
    assert (got["count"].sum(axis=1) + got["not_number"] + got["overflow"] == hist.sum(axis=1)).all(), what + ": the invariant"
    return want, got


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


# ---- the fixture's figures ----
def test_fixture_figures(hd):
    """the issue's figures through FmIndex.number_stats (the host form), each call also against the judge and through the device
    stage over the kept hits"""
    o, fm, T = hd

    def get(pattern, edges, where, frac_digits):
        w = Where("hd16", o, T, [pattern], [where] if where else [], [0 if where else -1])
        want, got = check_host(fm, o, w, T, edges, (500, 950), frac_digits, "%r %r" % (pattern, where))
        if not where:
            f = Filled(fm, w.ch, w.off)
            rc, dev = dev_block(f, 0, 1, w.lens, edges, (500, 950), frac_digits)
            assert rc == 0, last_error()
            check_numbers(dev, want, "device stage, %r" % pattern)
        return fm.number_stats(pattern, edges, where, (500, 950), frac_digits)

    assert_fixture_figures(get)
    s = fm.number_stats("size ", EDGES_250)
    assert s.kept == 608 and abs(s.mean()[1] - 1_543_503_872 / 23) < 1e-6 and s.pct.shape == (8, 2)
    assert fm.number_stats("zzqq#").count.tolist() == [0] and np.isnan(fm.number_stats("zzqq#").mean()[0])


# ---- the parser's edges on the device ----
def test_parser_table_on_the_device():
    """the parser table in one synthetic text, one hit per case, through the device stage and the host form at F = 0, 3, 9: a digit
    run cut by the end of the text, a window clipped to zero length at textLength"""
    text, patterns, expected = parser_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    fm = ia.FmIndex(text, 4, True, device=0)
    try:
        fm.build_line_table("\n")
        w = Where("parser table", o, T, patterns, [], [-1] * len(patterns))
        f = Filled(fm, w.ch, w.off)
        for k, F in enumerate(FRACS):
            want = judge_where_numbers(o, w, T, None, P5, F)
            assert want.values == [e[k] for e in expected]
            rc, dev = dev_block(f, 0, w.n, w.lens, None, P5, F)
            assert rc == 0, last_error()
            check_numbers(dev, want, "parser table, device, F %d" % F)
            assert dev["not_number"].tolist() == [int(e[k] is NAN) for e in expected] and dev["overflow"].tolist() == [int(e[k] is OVER) for e in expected]
            assert [int(v) for v, e in zip(dev["min"], expected) if isinstance(e[k], int)] == [e[k] for e in expected if isinstance(e[k], int)]
            check_host(fm, o, w, T, [0, 5, 30], P5, F, "parser table, host, F %d" % F)
    finally:
        fm.close()


# ---- the packed form's edges ----
def test_device_form_on_the_tile_edges(hd):
    """value hits trimmed to 0, 1, 1,023, 1,024, 1,025 and to whole tiles of slots, several tiles, slots behind the hits; with terms
    in front of the value patterns (hit_off[0] != 0) and without; a pattern without hits between two with hits; no edges, equal
    edges, every hit outside the buckets, 4,096 and 4,097 edges"""
    o, fm, T = hd
    for queries in ([], [dict(all=["terminating"]), dict(any=["WARN", "/10.250.1"])]):
        pats = [":", "size ", "zzzq#", "", "blk_"]
        w = Where("hd16 number edges", o, T, pats, queries, [-1] * len(pats), EVERY_LINE)
        f = Filled(fm, w.ch, w.off)
        first, total = int(w.hit_off[w.n_terms]), int(w.hit_off[-1])
        assert f.total == total and total - first > 5 * 1024 and (first > 0) == bool(queries)
        for n_hits in [first + k for k in (1, 1023, 1024, 1025)] + [1024 * (first // 1024 + 1), 1024 * (first // 1024 + 3) + 1, total - 1]:
            want = judge_where_numbers(o, Trimmed(w, n_hits), T, EDGES_UNEVEN, (500,), 0, lens=w.lens)
            rc, got = dev_block(f, w.n_terms, w.n, w.lens, EDGES_UNEVEN, (500,), 0, n_hits=n_hits)
            assert rc == 0, last_error()
            check_numbers(got, want, "n_hits %d of %d, %d in front" % (n_hits, total, first))
        for n_hits, edges in ((total, None), (total + 37, EDGES_BEYOND), (total + 1, many_edges(4096)), (total, many_edges(4097)), (total, [0, 2000]),
                              (total, [9, 9]), (total, [2000, 2001])):
            want = judge_where_numbers(o, w, T, edges, P5, 3)
            rc, got = dev_block(f, w.n_terms, w.n, w.lens, edges, P5, 3, n_hits=n_hits)
            assert rc == 0, last_error()
            check_numbers(got, want, "n_hits %d, %r edges" % (n_hits, None if edges is None else len(edges)))
        assert want.count.sum() == 0 and want.not_number.sum() == 0 and w.kept[2] == 0 and w.kept[1] == 608  # every hit outside the buckets
        if first:  # no value hit inside the slots: every row 0
            rc, got = dev_block(f, w.n_terms, w.n, w.lens, EDGES_250, n_hits=first)
            assert rc == 0 and all((v == 0).all() for v in got.values()), last_error()
    # outputs handed in as NULL: the others are still stored
    want = judge_where_numbers(o, w, T, EDGES_250, (), 0)
    rc, got = dev_block(f, w.n_terms, w.n, w.lens, EDGES_250, (), 0, skip=("sum_lo", "sum_hi", "min", "pct", "overflow"))
    assert rc == 0 and (got["count"].reshape(w.n, 8) == want.count).all() and (got["max"].reshape(w.n, 8) == want.max).all(), last_error()
    assert (got["not_number"] == want.not_number).all()
    # n_hits == 0: rows and counters are zeroed; n == 0: nothing is written
    rc, got = dev_block(f, w.n_terms, w.n, w.lens, EDGES_250, n_hits=0)
    assert rc == 0 and got["count"].shape == (40,) and all((v == 0).all() for v in got.values()), last_error()
    rc, got = dev_block(f, w.n_terms, 0, [], EDGES_250)
    assert rc == 0 and got["count"].shape == (0,), last_error()
    # n = 1 with B = 1: the narrowest key; 0 hits and 1 hit
    one = Where("hd16 number one", o, T, ["size "], [], [-1])
    f1 = Filled(fm, one.ch, one.off)
    for n_hits in (1, f1.total):
        rc, got = dev_block(f1, 0, 1, one.lens, None, (0, 1000), 0, n_hits=n_hits)
        assert rc == 0, last_error()
        check_numbers(got, judge_where_numbers(o, Trimmed(one, n_hits), T, None, (0, 1000), 0, lens=one.lens), "n = B = 1, %d hits" % n_hits)


def test_three_hundred_patterns(hd):
    """n = 300: several workgroups of rows, tiles that hold many patterns"""
    o, fm, T = hd
    pats = ["size ", "blk_", ":", "zzzq#", "src: /10.", "blk_-"] * 50
    w = Where("hd16 number 300", o, T, pats, [], [-1] * len(pats))
    base = judge_numbers(o, w.kept_locs[:w.kept_off[6]], w.kept_off[:7], w.lens[:6], T, EDGES_UNEVEN, (500, 950), 3)
    f = Filled(fm, w.ch, w.off)
    rc, got = dev_block(f, 0, 300, w.lens, EDGES_UNEVEN, (500, 950), 3)
    assert rc == 0, last_error()
    B = len(EDGES_UNEVEN) - 1
    assert (got["count"].reshape(50, 6, B) == base.count).all() and (got["min"].reshape(50, 6, B) == base.min).all()
    assert (got["pct"].reshape(50, 6, B, 2) == base.pct).all() and (got["not_number"].reshape(50, 6) == base.not_number).all()
    check_numbers({k: np.asarray(v).reshape(50, -1)[49] for k, v in got.items()}, base, "the last six of 300")


# ---- percentile indices ----
def test_percentile_indices():
    """permille 0, 1, 500, 999, 1000 against segments of 1, 2, 3, 1,000 and 1,001 values with duplicates; P = 0 and P = 16"""
    text, patterns = segments_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    fm = ia.FmIndex(text, 4, True, device=0)
    try:
        fm.build_line_table("\n")
        w = Where("segments", o, T, patterns, [], [-1] * 5)
        f = Filled(fm, w.ch, w.off)
        for edges, pm in ((None, P5), (None, ()), ([0, 50, 50, 150, 300], P16), (None, (1000,) * 16)):
            want = judge_where_numbers(o, w, T, edges, pm, 0)
            rc, got = dev_block(f, 0, 5, w.lens, edges, pm, 0)
            assert rc == 0, last_error()
            check_numbers(got, want, "segments, %d permilles" % len(pm))
            check_host(fm, o, w, T, edges, pm, 0, "segments, host, %d permilles" % len(pm))
        assert want.count[:, 0].tolist() == [1, 2, 3, 1000, 1001]
    finally:
        fm.close()


# ---- quirk rows, image forms ----
def test_quirk_rows_follow_the_reference_extract():
    """the fixture followed by the run-block text (quirk Q1: its rows derail the reference's walks, the packed extract's redo list is
    not empty): the answer equals the judge built on the ORACLE's windows, which are not the text's"""
    text = HD + run_block_text()
    t16 = ia.as_chars(text)
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, "\n")
    pats = [chr(0x30A9), "log line ", "size "]
    w = Where("hd+runblocks numbers", o, T, pats, [], [-1] * len(pats))
    want = judge_where_numbers(o, w, T, None, P5, 0)
    rows, lengths = want.windows.rows, want.windows.lengths
    by_text = sum(1 for h, r, ln in zip(w.kept_locs[:w.kept_off[1]], rows, lengths) if t16[h + 1:h + 1 + ln].tolist() != r[:ln].tolist())
    assert w.kept[0] == 70_000 and by_text > 0 and w.kept[1] == 600 and want.count[1, 0] > 0
    fm = ia.FmIndex(text, 16, True, device=0)
    try:
        fm.build_line_table("\n")
        rc, dev = dev_block(Filled(fm, w.ch, w.off), 0, w.n, w.lens, None, P5, 0)
        assert rc == 0, last_error()
        check_numbers(dev, want, "quirk rows, device form")
        check_host(fm, o, w, T, [0, 1000, 2000, 3000], P5, 0, "quirk rows, host form")
    finally:
        fm.close()


def test_compact_image_and_index_without_extraction(hd):
    o, fm0, T = hd
    w = Where("hd16 number mix", o, T, ["size ", "blk_", "", "src: /10."], [dict(all=["addStoredBlock"])], [0, -1, -1, -1])
    with options(image_compact=1):
        fm = ia.FmIndex(HD, 16, True, device=None)
        fm.blob()  # flattened under the option
        fm.to_device(0)
    try:
        fm.build_line_table("\n")
        check_host(fm, o, w, T, EDGES_UNEVEN, (500, 950), 3, "compact image")
        raw = Where("hd16 number mix", o, T, ["size ", "blk_", "", "src: /10."], [], [-1] * 4)
        rc, dev = dev_block(Filled(fm, raw.ch, raw.off), 0, 4, raw.lens, EDGES_250, P5, 0)
        assert rc == 0, last_error()
        check_numbers(dev, judge_where_numbers(o, raw, T, EDGES_250, P5, 0), "compact image, device form")
    finally:
        fm.close()
    fm = ia.FmIndex(HD, 16, False, device=0)
    try:
        fm.build_line_table("\n")
        got = host_numbers(fm, w, EDGES_250)
        assert (got["status"] == ST_NOT_ENABLED).all() and (got["kept"] == w.kept).all() and (got["occurrences"] == w.occurrences).all()
        assert w.kept[0] == 314 and all((got[k] == 0).all() for k in NAMES)
        raw = Where("hd16 number mix", o, T, ["size ", "blk_", "", "src: /10."], [], [-1] * 4)
        f = Filled(fm, raw.ch, raw.off)
        rc, dev = dev_block(f, 0, 4, raw.lens, EDGES_250, P5, 0)
        assert rc == 0 and all((v == 0).all() for v in dev.values()), last_error()
        assert (f.d.st.cpu().numpy()[:4] == ST_NOT_ENABLED).all()
        with pytest.raises(RuntimeError):
            fm.number_stats("size ")
    finally:
        fm.close()


# ---- launch shapes ----
@pytest.mark.parametrize("opts", [dict(block=1024, groups_per_cu=1), dict(block=512, groups_per_cu=64)])
def test_launch_shapes(hd, opts):
    """ONE pattern with every hit of the block (lanes go to slots and to rows, not to patterns) and the mix, under `block` = 1024
    and a small groups_per_cu (looping grids in the extract and in the locate stages in front)"""
    o, fm, T = hd
    w = Where("hd16 number one", o, T, [" "], [], [-1])
    assert w.occurrences[0] > 30000
    mix = Where("hd16", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    with options(**opts):
        f = Filled(fm, w.ch, w.off)
        for edges in (EDGES_BEYOND, many_edges(257)):
            rc, got = dev_block(f, 0, 1, w.lens, edges, P5, 0)
            assert rc == 0, last_error()
            check_numbers(got, judge_where_numbers(o, w, T, edges, P5, 0), repr(opts))
        check_host(fm, o, mix, T, EDGES_UNEVEN, (500, 950), 0, "mix under %r" % opts)


def test_grid_stride_loops_run_more_than_once(hd):
    """(" ", "1", "0") repeated until the slots are more than the key grid covers in one pass, under groups_per_cu=1"""
    o, fm, T = hd
    w = Where("hd16 heavy raw", o, T, [" ", "1", "0"], [dict(all=["terminating"])], [-1, -1, -1])
    nt, per = w.n_terms, int(w.hit_off[-1] - w.hit_off[w.n_terms])
    key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
    assert ia.lib.fmx_hit_lines_geometry(fm.handle, 10 ** 9, C.byref(key_grid), C.byref(flat_grid)) == 0  # (the caps)
    reps = key_grid.value * 1024 // per + 2
    pats = [w.ch[w.off[i]:w.off[i + 1]] for i in range(nt + w.n)]
    ch, off = ia.pack_patterns(pats[:nt] + pats[nt:] * reps)
    want = judge_where_numbers(o, w, T, EDGES_UNEVEN, (500,), 0)
    with options(groups_per_cu=1):
        f = Filled(fm, ch, off.astype(np.int32))
        assert f.total == int(w.hit_off[nt]) + reps * per and key_grid.value * 1024 < f.total
        rc, got = dev_block(f, nt, w.n * reps, np.tile(w.lens, reps), EDGES_UNEVEN, (500,), 0)
    assert rc == 0, last_error()
    B = len(EDGES_UNEVEN) - 1
    assert (got["count"].reshape(reps, 3, B) == want.count).all() and (got["pct"].reshape(reps, 3, B) == want.pct[:, :, 0]).all()
    assert (got["max"].reshape(reps, 3, B) == want.max).all() and (got["not_number"].reshape(reps, 3) == want.not_number).all()
    lo, hi = got["sum_lo"].reshape(reps, 3, B), got["sum_hi"].reshape(reps, 3, B)
    assert [[(int(hi[-1, i, b]) << 64) | int(lo[-1, i, b]) for b in range(B)] for i in range(3)] == want.sums


# ---- the host forms and the mirrors ----
def test_mixes_over_uneven_edges(hd):
    o, fm, T = hd
    w = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    for edges, pm, F in ((EDGES_UNEVEN, (500, 950), 0), (None, P5, 3), (many_edges(4097), (), 9), (EDGES_BEYOND, P16, 0)):
        want, got = check_host(fm, o, w, T, edges, pm, F, "mix, %r edges" % (None if edges is None else len(edges)))
    assert want.count[4:8].sum() == 0 and w.status[-1] == 9 and want.hist_total[0] == 310
    # every where_of negative: the filter stage is skipped — with terms in the call and without; without edges no line table is needed
    raw = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, [-1] * len(MIX_PATTERNS))
    check_host(fm, o, raw, T, EDGES_UNEVEN, (500,), 0, "raw, terms in front")
    bare = Where("hd16 mix", o, T, MIX_PATTERNS, [], [-1] * len(MIX_PATTERNS))
    want, got = check_host(fm, o, bare, T, None, (500,), 0, "raw, no terms")
    assert (want.hist_total == bare.occurrences).all()
    plain = ia.FmIndex(HD, 16, True, device=0)
    try:
        check_numbers(host_numbers(plain, bare, None, (500,), 0), want, "no line table, no edges, no filter")
        for run in (lambda: plain.number_stats("size ", EDGES_250), lambda: plain.number_stats("size ", where=dict(all="INFO"))):
            with pytest.raises(ia.FmxError) as err:
                run()
            assert err.value.code == ia._lib.E_ARG and "fmx_line_table_build" in str(err.value)
    finally:
        plain.close()
    # n == 0: FMX_OK, nothing is searched, term_status zeroed
    out = fm.number_stats_where_batch(np.zeros(0, np.uint16), [0], *ia.pack_patterns(["INFO"]), [0, 1], [0], [], EDGES_250)
    assert out["count"].shape == (0, 8) and list(out["term_status"]) == [0]


def test_class_forms(hd):
    o, fm, T = hd
    spell = lambda word: sorted(set(re.findall("(?i)" + re.escape(word), HD)))  # noqa: E731
    assert len(spell("size ")) > 1 or len(spell("block")) > 1
    # the judge over the union of the spellings' hits: every spelling the text holds, as a literal
    for word, term in (("SIZE ", "ADDSTOREDBLOCK"), ("Blk_", "TERMINATING")):
        lit = Where("hd16 spellings", o, T, spell(word), [dict(any=spell(term))], [0] * len(spell(word)))
        want = judge_where_numbers(o, lit, T, EDGES_UNEVEN, (500, 950), 0)
        s = fm.number_stats(word, EDGES_UNEVEN, where=dict(all=term), ignore_case=True)
        assert s.count.tolist() == want.count.sum(axis=0).tolist() and s.sum == [sum(r[b] for r in want.sums) for b in range(want.B)]
        assert s.not_number == want.not_number.sum() and s.kept == lit.kept.sum() and s.count.sum() > 0
        if len(spell(word)) == 1:
            assert (s.min == want.min[0]).all() and (s.max == want.max[0]).all() and (s.pct == want.pct[0]).all()
        assert fm.number_stats(word, EDGES_UNEVEN, where=dict(all=term)).kept == 0  # (no such spelling in the text)
    # a frontier larger than max_ranges has no hits, as in fmx_hit_histogram_where_class_batch
    terms = ia.pack_class_patterns([ia.ignore_case("TERMINATING")])
    out = fm.number_stats_where_class_batch(*ia.pack_class_patterns([ia.ignore_case("size ")]), *terms, [0, 1], [0], [0], EDGES_250, max_ranges=1)
    assert out["term_status"][0] == ST_TOO_MANY and (out["count"] == 0).all() and out["kept"][0] == 0


# ---- refusals: every one returns before a launch ----
def test_refusals_leave_the_outputs_untouched(hd):
    o, fm, T = hd
    w = Where("hd16", o, T, ["size "], [], [-1])
    f = Filled(fm, w.ch, w.off)
    E_ARG = ia._lib.E_ARG
    need = ia.lib.fmx_numbers_of_hits_scratch_bytes(1, f.total, len(EDGES_250), 2)
    assert need > 124 * f.total and need % 256 == 0
    rc, got = dev_block(f, 0, 1, w.lens, EDGES_250, ws_bytes=need - 1)  # a workspace one byte short
    assert rc == E_ARG and "fmx_numbers_of_hits_scratch_bytes" in last_error() and untouched(got)
    big = np.arange((1 << 16) + 2, dtype=np.int32)
    for bad in (dict(edges=[5]), dict(edges=[-1, 5]), dict(edges=[5, 4]), dict(frac_digits=-1), dict(frac_digits=10), dict(permille=(1001,)),
                dict(permille=(-1,)), dict(permille=(5,) * 17), dict(lens=[-1]), dict(n_hits=-1)):
        args = dict(lens=w.lens, edges=EDGES_250)
        args.update(bad)
        rc, got = dev_block(f, 0, 1, **args)
        assert rc == E_ARG and untouched(got), bad
    torch = _torch()
    p = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    one, e = np.array([5], np.int32), np.array(EDGES_250, np.int32)
    dv = ia.lib.fmx_numbers_of_hits_dev

    def call(h=fm.handle, n=1, tl=one, n_hits=5, edges=e, n_edges=len(e), hoff=p.data_ptr(), count=p.data_ptr()):
        return dv(h, n, tl.ctypes.data, hoff, p.data_ptr(), n_hits, None if edges is None else edges.ctypes.data, n_edges, 0, None, 0, count, None, None,
                  None, None, None, None, None, None, p.data_ptr(), 256, stream())

    for bad in (dict(h=None), dict(n=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(count=None), dict(edges=None), dict(n_edges=0),
                dict(n=1 << 11, tl=np.zeros(1 << 11, np.int32), edges=big, n_edges=len(big))):
        assert call(**bad) == E_ARG, bad
    assert call() == E_ARG and "fmx_numbers_of_hits_scratch_bytes" in last_error()  # (256 bytes of workspace)
    # no line table: only when edges are given; a SuffixArray handle
    bare = ia.FmIndex(HD[:5000], 16, True, device=0)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    try:
        sa.construct()
        assert call(h=bare.handle) == E_ARG and "fmx_line_table_build" in last_error()
        assert call(h=bare.handle, edges=None, n_edges=0) == E_ARG and "fmx_numbers_of_hits_scratch_bytes" in last_error()
        assert call(h=sa._h) == E_ARG
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == SENT).all()  # nothing launched, nothing written
    # ... and the exact workspace serves
    rc, got = dev_block(f, 0, 1, w.lens, EDGES_250, ws_bytes=need)
    assert rc == 0, last_error()
    check_numbers(got, judge_where_numbers(o, w, T, EDGES_250), "the exact workspace")
    for kw in (dict(edges=[5]), dict(edges=[5, 4]), dict(frac_digits=10), dict(permille=[1001]), dict(permille=list(range(17)))):
        with pytest.raises(ia.FmxError) as err:
            fm.number_stats("size ", **kw)
        assert err.value.code == E_ARG


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_number_stats_mirror.cpp prints what numberStatsWhereBatch / numberStatsWhere return"""
    o, fm, T = hd
    exe = str(tmp_path / "test_number_stats_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_number_stats_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    w = Where("hd16 mirror", o, T, ["size ", "size ", "zzqq#", "blk_"], [dict(all=["addStoredBlock"])], [-1, 0, 0, -1])
    want = judge_where_numbers(o, w, T, EDGES_250, (500, 950), 0)
    assert out["batch_count"] == want.count.ravel().tolist() and out["batch_min"] == want.min.ravel().tolist()
    assert out["batch_max"] == want.max.ravel().tolist() and out["batch_pct"] == want.pct.ravel().tolist()
    sums = [(hi << 64) | lo for lo, hi in zip(out["batch_sum_lo"], out["batch_sum_hi"])]
    assert sums == [s for row in want.sums for s in row] and max(sums) > 2 ** 64
    assert out["batch_not_number"] == want.not_number.tolist() and out["batch_overflow"] == want.overflow.tolist()
    assert out["batch_occurrences"] == [608, 608, 0, 2468] and out["batch_kept"] == w.kept.tolist() and out["batch_status"] == [0] * 4
    assert out["batch_term_status"] == [0]
    src = Where("hd16 mirror", o, T, ["src: /10."], [], [-1])
    one = judge_where_numbers(o, src, T, None, (500, 950), 3)
    assert out["one_count"] == [235] and out["one_min"] == one.min.ravel().tolist() and out["one_pct"] == one.pct.ravel().tolist() == [251_195, 251_740]
    assert out["one_sum_lo"] == [59_007_553] and out["one_sum_hi"] == [0] and out["one_tails"] == [int(one.not_number[0]), int(one.overflow[0])]

"""Matching lines and hits per bucket of lines on the GPU, the timeline of a log search: packed ascending lists -> q x B counters
(fmx_lines_histogram_dev), packed hits -> n x B counters (fmx_hits_histogram_dev: the kernels of fmx_line_hist.hip around rocPRIM's
radix sort) and the host forms fmx_line_histogram_batch / fmx_hit_histogram_where_batch with their class twins, their Python and
C++ mirrors.

The judge is np.searchsorted(edges, lines, "right") - 1 over the existing judges' lines, kept hits and line table
(tests/test_line_histogram_cpu.py: judge_bins, judge_line_hist, judge_hit_hist over tests/test_field_values_where_cpu.py's Where),
computed once per batch.  Outputs are prefilled with a sentinel, and everything behind the answer must keep it.  Options are set
inside the tests and put back in `finally`.  Every refused call returns before a launch."""
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
from test_field_values_where_cpu import EVERY_LINE, Trimmed, Where
from test_gpu_field_values import ST_TOO_MANY, last_error
from test_gpu_field_values_where import MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, Filled
from test_gpu_locate_rows import _torch, options
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN, NAMED_HIST, judge_bins, judge_hit_hist, judge_line_hist, named_where
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table, texts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def dev_lines_hist(fm, line_off, lines, edges, ws_bytes=None):
    """fmx_lines_histogram_dev over packed lists; rc, (q, B) counters — what lies behind them has kept the sentinel (asserted)"""
    torch = _torch()
    q, B = len(line_off) - 1, len(edges) - 1
    need = ia.lib.fmx_lines_histogram_scratch_bytes(q, len(edges))
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    d_loff = torch.from_numpy(np.array(line_off, np.int64)).cuda()
    d_lines = torch.from_numpy(np.concatenate([lines, np.full(1, SENT, np.int32)]).astype(np.int32)).cuda()
    hist = torch.full((q * B + PAD,), SENT, dtype=torch.int32, device="cuda")
    e = np.array(edges, np.int32)  # the call's own copy: scribbled over once it is back
    rc = ia.lib.fmx_lines_histogram_dev(fm.handle, q, d_loff.data_ptr(), d_lines.data_ptr(), e.ctypes.data, len(e), hist.data_ptr(), ws.data_ptr(),
                                        use, stream())
    e[:] = -9  # (the call has copied what it needs before it returns)
    torch.cuda.synchronize()
    out = hist.cpu().numpy()
    assert (out[q * B:] == SENT).all(), "stored beyond q * B"
    return rc, out[:q * B].reshape(q, B)


def dev_hits_hist(fm, n, d_hit_off_ptr, d_locs_ptr, n_hits, edges, ws_bytes=None):
    torch = _torch()
    B = len(edges) - 1
    need = ia.lib.fmx_hits_histogram_scratch_bytes(n, n_hits, len(edges))
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    hist = torch.full((n * B + PAD,), SENT, dtype=torch.int32, device="cuda")
    e = np.array(edges, np.int32)
    rc = ia.lib.fmx_hits_histogram_dev(fm.handle, n, d_hit_off_ptr, d_locs_ptr, n_hits, e.ctypes.data, len(e), hist.data_ptr(), ws.data_ptr(), use,
                                       stream())
    e[:] = -9
    torch.cuda.synchronize()
    out = hist.cpu().numpy()
    assert (out[n * B:] == SENT).all(), "stored beyond n * B"
    return rc, out[:n * B].reshape(n, B)


def dev_block_hist(f, n_terms, n, edges, n_hits=None, **kw):
    """... over the value patterns' part of a Filled block (hit_off + n_terms: it does not start at 0 when a term has a hit).
    n_hits: the slots of the block the call may look at (default: all hits; up to 64 more: slots without a hit)"""
    n_hits = f.total if n_hits is None else n_hits
    assert n_hits <= f.total + 64  # (d.locs has that many slots behind the hits)
    return dev_hits_hist(f.fm, n, f.d.hit_off.data_ptr() + 8 * n_terms, f.d.locs.data_ptr(), n_hits, edges, **kw)


def many_edges(n_edges, top=2100, seed=5):
    """n_edges sorted line ids over the fixture's lines and a little beyond, with equal neighbours among them"""
    return np.sort(np.random.default_rng(seed).integers(0, top, n_edges)).astype(np.int32)


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


# ---- the device stage, lines form ----
def test_device_lines_form(hd):
    """lists of 0, 1, 2 and 1,025 lines and one with duplicates; q = 5 and 300 (several workgroups of counters, and with 4,097 edges
    more (list, edge) pairs than the grid covers in one pass); n_edges 2, 3, 257, 4,096 and 4,097; all lines in one bucket, all
    outside the buckets, equal edges; sentinels behind q * B stay"""
    o, fm, T = hd
    rng = np.random.default_rng(7)
    lists = [np.zeros(0, np.int32), np.array([77], np.int32), np.array([0, 9999], np.int32),
             np.sort(rng.choice(10000, 1025, replace=False)).astype(np.int32), np.sort(rng.integers(0, 50, 300)).astype(np.int32)]
    for reps in (1, 60):
        tiled = lists * reps
        line_off = np.concatenate([[0], np.cumsum([len(a) for a in tiled])]).astype(np.int64)
        lines = np.concatenate(tiled)
        shapes = ([0, 10000], [0, 77, 78], [10000, 20000], [5, 5], [50, 50, 50, 9999], np.linspace(0, 10001, 257), many_edges(4096, 11000),
                  many_edges(4097, 11000))
        for edges in shapes if reps == 1 else shapes[1:2] + shapes[-1:]:
            edges = np.asarray(edges, np.int32)
            want = np.tile(np.array([judge_bins(edges, a) for a in lists]), (reps, 1))
            rc, got = dev_lines_hist(fm, line_off, lines, edges)
            assert rc == 0, last_error()
            assert (got == want).all(), (reps, len(edges), np.argwhere(got != want)[:4])
    # one list alone (q = 1), and q == 0: nothing is written
    rc, got = dev_lines_hist(fm, [0, 1025], lists[3], EDGES_UNEVEN)
    assert rc == 0 and (got[0] == judge_bins(EDGES_UNEVEN, lists[3])).all(), last_error()
    rc, got = dev_lines_hist(fm, [0], np.zeros(0, np.int32), [0, 5])
    assert rc == 0 and got.shape == (0, 1), last_error()


# ---- the device stage, hits form ----
def test_device_hits_form_on_the_tile_edges(hd):
    """value hits trimmed to 0, 1, 1,023, 1,024, 1,025 and to whole tiles of slots, several tiles, slots behind the hits; with terms
    in front of the value patterns (hit_off[0] != 0) and without; a pattern without hits between two with hits"""
    o, fm, T = hd
    for queries in ([], [dict(all=["terminating"]), dict(any=["WARN", "/10.250.1"])]):
        pats = [" ", "blk_", "zzzq#", "", "1"]
        w = Where("hd16 edges", o, T, pats, queries, [-1] * len(pats), EVERY_LINE)
        f = Filled(fm, w.ch, w.off)
        first, total = int(w.hit_off[w.n_terms]), int(w.hit_off[-1])
        assert f.total == total and total - first > 5 * 1024 and (first > 0) == bool(queries)
        for n_hits in [first + k for k in (1, 1023, 1024, 1025)] + [1024 * (first // 1024 + 1), 1024 * (first // 1024 + 3) + 1, total - 1]:
            t = Trimmed(w, n_hits)
            rc, got = dev_block_hist(f, w.n_terms, w.n, EDGES_UNEVEN, n_hits=n_hits)
            assert rc == 0, last_error()
            assert (got == judge_hit_hist(t, T, EDGES_UNEVEN)).all(), "n_hits %d of %d, %d in front" % (n_hits, total, first)
        for n_hits, edges in ((total, EDGES_UNEVEN), (total + 37, EDGES_BEYOND), (total, EDGES_250), (total + 1, many_edges(4096)),
                              (total, many_edges(4097)), (total, [0, 2000]), (total, [2000, 2001]), (total, [9, 9])):
            want = judge_hit_hist(w, T, edges)
            rc, got = dev_block_hist(f, w.n_terms, w.n, edges, n_hits=n_hits)
            assert rc == 0, last_error()
            assert (got == want).all(), (n_hits, len(edges), np.argwhere(got != want)[:4])
            if edges[0] == 0 and edges[-1] >= 2000:
                assert (got.sum(axis=1) == w.kept).all()
        assert want.sum() == 0 and w.kept[2] == 0 and w.kept[1] == 2468 and w.kept[4] > 0
        if first:  # no value hit inside the slots: every counter 0
            rc, got = dev_block_hist(f, w.n_terms, w.n, EDGES_250, n_hits=first)
            assert rc == 0 and (got == 0).all(), last_error()
    # n_hits == 0: the counters are zeroed; n == 0: nothing is written
    rc, got = dev_block_hist(f, w.n_terms, w.n, EDGES_250, n_hits=0)
    assert rc == 0 and got.shape == (5, 8) and (got == 0).all(), last_error()
    rc, got = dev_block_hist(f, w.n_terms, 0, EDGES_250)
    assert rc == 0 and got.shape == (0, 8), last_error()


@pytest.mark.parametrize("opts", [dict(block=512, groups_per_cu=1), dict(block=1024, groups_per_cu=64)])
def test_one_pattern_owns_every_hit_under_the_options_extremes(hd, opts):
    """ONE pattern with every hit of the block (lanes go to slots and to counters, not to patterns); the grids are
    fmx_hit_lines_geometry's whatever `block` and `groups_per_cu` say, the locate stages in front honour them"""
    o, fm, T = hd
    w = Where("hd16 one", o, T, [" "], [], [-1])
    assert w.occurrences[0] > 30000
    with options(**opts):
        f = Filled(fm, w.ch, w.off)
        for edges in (EDGES_BEYOND, many_edges(257)):
            rc, got = dev_block_hist(f, 0, 1, edges)
            assert rc == 0, last_error()
            assert (got == judge_hit_hist(w, T, edges)).all()
        rc, got = dev_lines_hist(fm, [0, 0, 2000], np.arange(2000, dtype=np.int32), many_edges(257))
        assert rc == 0 and (got[1] == judge_bins(many_edges(257), np.arange(2000))).all() and got[0].sum() == 0


def test_grid_stride_loops_run_more_than_once(hd):
    """(" ", "1", "0") repeated until the slots are more than the key grid covers in one pass, under groups_per_cu=1 as the other
    hit stages' tests do"""
    o, fm, T = hd
    w = Where("hd16 heavy raw", o, T, [" ", "1", "0"], [dict(all=["terminating"])], [-1, -1, -1])
    nt, per = w.n_terms, int(w.hit_off[-1] - w.hit_off[w.n_terms])
    key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
    assert ia.lib.fmx_hit_lines_geometry(fm.handle, 10 ** 9, C.byref(key_grid), C.byref(flat_grid)) == 0  # (the caps)
    reps = key_grid.value * 1024 // per + 2
    pats = [w.ch[w.off[i]:w.off[i + 1]] for i in range(nt + w.n)]
    ch, off = ia.pack_patterns(pats[:nt] + pats[nt:] * reps)
    with options(groups_per_cu=1):
        f = Filled(fm, ch, off.astype(np.int32))
        assert f.total == int(w.hit_off[nt]) + reps * per and key_grid.value * 1024 < f.total
        rc, got = dev_block_hist(f, nt, w.n * reps, EDGES_UNEVEN)
    assert rc == 0, last_error()
    assert (got == np.tile(judge_hit_hist(w, T, EDGES_UNEVEN), (reps, 1))).all()


# ---- the host forms and the mirrors ----
def host_lines(fm, w, edges):
    ch, off = w.term_arrays()
    return fm.line_histogram_batch(ch, off, w.query_off, w.kinds, edges, want_counts=True)


def host_hits(fm, w, edges):
    return fm.hit_histogram_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, edges, want_counts=True)


def check_host_lines(fm, w, edges, what):
    hist, st, line_count, occ = host_lines(fm, w, edges)
    want = judge_line_hist(w, edges)
    assert hist.shape == want.shape and (hist == want).all(), what
    assert (line_count == [len(x) for x in w.query_lines]).all() and (occ == w.counts[:w.n_terms]).all() and (st == w.term_status).all(), what
    if edges[0] == 0 and edges[-1] >= 2000:
        assert (hist.sum(axis=1) == line_count).all(), what
    return hist


def check_host_hits(fm, w, T, edges, what):
    hist, st, occ, kept, tst = host_hits(fm, w, edges)
    want = judge_hit_hist(w, T, edges)
    assert hist.shape == want.shape and (hist == want).all(), what
    assert (kept == w.kept).all() and (occ == w.occurrences).all() and (st == w.status[w.n_terms:]).all() and (tst == w.term_status).all(), what
    assert (hist.sum(axis=1) <= kept).all()
    if edges[0] == 0 and edges[-1] >= 2000:
        assert (hist.sum(axis=1) == kept).all(), what
    return hist


def test_named_cases_c_abi_and_python(hd):
    o, fm, T = hd
    for form, pattern, query, per_bucket in NAMED_HIST:
        w = named_where(o, T, form, pattern, query)
        if form == "lines":
            assert check_host_lines(fm, w, EDGES_250, "named lines")[0].tolist() == per_bucket
            assert fm.line_histogram(EDGES_250, **query).tolist() == per_bucket
        else:
            assert check_host_hits(fm, w, T, EDGES_250, "named hits")[0].tolist() == per_bucket
            assert fm.hit_histogram(pattern, EDGES_250, where=query).tolist() == per_bucket
    assert fm.hit_histogram("blk_", [0, 2000]).tolist() == [2468] and fm.line_histogram([0, 2000, 2000, 5000], all="terminating").tolist() == [310, 0, 0]
    # an edge from a timestamp: the first line that holds it
    first = int(fm.match_lines(HD.split("\n")[1000][:11], max_lines=1)[0])
    assert 0 < first <= 1000 and fm.line_histogram([0, first, 2000], all="terminating").sum() == 310


def test_mixes_over_uneven_edges(hd):
    o, fm, T = hd
    w = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    for edges in (EDGES_UNEVEN, EDGES_BEYOND, many_edges(4097)):
        hist = check_host_hits(fm, w, T, edges, "mix, %d edges" % len(edges))
        check_host_lines(fm, w, edges, "mix lines, %d edges" % len(edges))
    # a query without lines, NONE only, no terms, a pattern without hits, the empty pattern (FMX_ST_JAVA_AIOOBE)
    hist = check_host_hits(fm, w, T, [0, 1000, 2000], "mix, two halves")
    assert hist[4:8].sum() == 0 and hist[10].sum() == 0 and w.status[-1] == 9 and hist[0].sum() == 310 and hist[3].sum() == w.occurrences[3]
    lines_hist = judge_line_hist(w, EDGES_BEYOND)
    assert lines_hist[3].sum() == 0 and lines_hist[4].sum() == 0 and lines_hist[0].sum() == 310
    # every where_of negative: the filter stage is skipped, the raw hits are binned — with terms in the call and without
    raw = Where("hd16 mix", o, T, MIX_PATTERNS, MIX_QUERIES, [-1] * len(MIX_PATTERNS))
    check_host_hits(fm, raw, T, EDGES_UNEVEN, "raw, terms in front")
    bare = Where("hd16 mix", o, T, MIX_PATTERNS, [], [-1] * len(MIX_PATTERNS))
    assert (check_host_hits(fm, bare, T, EDGES_BEYOND, "raw, no terms").sum(axis=1) == bare.occurrences).all()
    # n == 0: FMX_OK, nothing is searched, term_status zeroed
    out = fm.hit_histogram_where_batch(np.zeros(0, np.uint16), [0], *ia.pack_patterns(["INFO"]), [0, 1], [0], [], EDGES_250, want_counts=True)
    assert out[0].shape == (0, 8) and list(out[4]) == [0]
    out = fm.line_histogram_batch(np.zeros(0, np.uint16), [0], [0, 0, 0], [], EDGES_250, want_counts=True)
    assert out[0].shape == (2, 8) and (out[0] == 0).all() and list(out[2]) == [0, 0]


def test_one_all_term_per_query_against_match_lines(hd):
    """q queries of one ALL term: the lines are match_lines_batch's, binned on the host"""
    o, fm, T = hd
    terms = ["terminating", "blk_", "zzzq#", "WARN", " ", "PacketResponder", "081109", "INFO dfs.DataNode$PacketResponder"] * 40
    ch, off = ia.pack_patterns(terms)
    lines, line_off, status = fm.match_lines_batch(ch, off)
    q = len(terms)
    for edges in (EDGES_UNEVEN, many_edges(61)):
        hist, st, line_count, occ = fm.line_histogram_batch(ch, off, np.arange(q + 1), np.zeros(q, np.uint8), edges, want_counts=True)
        want = np.array([judge_bins(edges, lines[a:b]) for a, b in zip(line_off[:-1], line_off[1:])])
        assert (hist == want).all() and (line_count == np.diff(line_off)).all() and (st == status).all()
    assert hist[0].sum() > 0 and hist[2].sum() == 0 and q == 320


def test_class_forms(hd):
    o, fm, T = hd
    spell = lambda word: sorted(set(re.findall("(?i)" + re.escape(word), HD)))  # noqa: E731
    assert len(spell("block")) > 1
    # the judge over the union of the spellings' hits: every spelling the text holds, as a literal
    lit = Where("hd16 spellings", o, T, spell("block"), [dict(any=spell("TERMINATING"))], [0] * len(spell("block")))
    want_hits = judge_hit_hist(lit, T, EDGES_UNEVEN).sum(axis=0)
    assert fm.hit_histogram("BLOCK", EDGES_UNEVEN, where=dict(all="TERMINATING"), ignore_case=True).tolist() == want_hits.tolist()
    assert fm.hit_histogram("BLOCK", EDGES_UNEVEN, where=dict(all="terminating")).sum() == 0  # (no such spelling in the text)
    want_lines = judge_bins(EDGES_UNEVEN, lit.query_lines[0])
    assert fm.line_histogram(EDGES_UNEVEN, all="TERMINATING", ignore_case=True).tolist() == want_lines.tolist() and want_lines.sum() > 0
    # a term whose frontier is larger than max_ranges has no hits, as in fmx_match_query_class_batch: its ALL query has no lines
    terms = ia.pack_class_patterns([ia.ignore_case("TERMINATING")])
    hist, st, line_count, occ = fm.line_histogram_class_batch(*terms, [0, 1], [0], EDGES_250, want_counts=True, max_ranges=1)
    assert st[0] == ST_TOO_MANY and (hist == 0).all() and line_count[0] == 0
    out = fm.hit_histogram_where_class_batch(*ia.pack_class_patterns([ia.ignore_case("blk_")]), *terms, [0, 1], [0], [0], EDGES_250, want_counts=True,
                                             max_ranges=1)
    assert out[4][0] == ST_TOO_MANY and (out[0] == 0).all() and out[3][0] == 0


def line_search_texts():
    t = texts()
    return {"a few lines": t["empty lines"], "the fixture, last line unterminated": t["hdfs, last line unterminated"],
            "more lines than the fences hold": (count_text(8193, False), "\n")}


@pytest.mark.parametrize("name", sorted(line_search_texts()))
def test_line_search_paths(name):
    """fm_line_of inside the key kernel: a table of a few entries, one entry per fence, and more entries than the 4,096 fences hold"""
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
        w = Where(name, o, T, patterns, queries, [(-1, 0, 1)[i % 3] for i in range(len(patterns))])
        for edges in ([0, n_lines], [0, 1, n_lines - 1, n_lines, n_lines + 7], np.unique(np.linspace(0, n_lines, 50).astype(np.int32)), [1, max(n_lines - 1, 1)]):
            edges = np.asarray(edges, np.int32)
            hist, st, occ, kept, tst = host_hits(fm, w, edges)
            assert (hist == judge_hit_hist(w, T, edges)).all() and (kept == w.kept).all(), (name, edges[:5])
            lh = host_lines(fm, w, edges)[0]
            assert (lh == judge_line_hist(w, edges)).all(), (name, edges[:5])
        assert w.kept.sum() > 0
    finally:
        fm.close()


# ---- refusals: every one returns before a launch ----
def test_refusals_leave_the_outputs_untouched(hd):
    o, fm, T = hd
    w = Where("hd16", o, T, ["blk_"], [], [-1])
    f = Filled(fm, w.ch, w.off)
    E_ARG = ia._lib.E_ARG
    # a workspace one byte short
    need = ia.lib.fmx_hits_histogram_scratch_bytes(1, f.total, len(EDGES_250))
    assert need > 16 * f.total and need % 256 == 0
    torch = _torch()
    hist = torch.full((64,), SENT, dtype=torch.int32, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    e = np.array(EDGES_250, np.int32)

    def hcall(h=fm.handle, n=1, n_hits=f.total, edges=e, n_edges=len(e), ws_bytes=need, hoff=f.d.hit_off.data_ptr(), out=hist.data_ptr()):
        return ia.lib.fmx_hits_histogram_dev(h, n, hoff, f.d.locs.data_ptr(), n_hits, None if edges is None else edges.ctypes.data, n_edges, out,
                                             ws.data_ptr(), ws_bytes, stream())

    assert hcall(ws_bytes=need - 1) == E_ARG and "fmx_hits_histogram_scratch_bytes" in last_error()
    lists = np.arange(100, dtype=np.int32)
    d_loff, d_lines = torch.tensor([0, 100], dtype=torch.int64, device="cuda"), torch.from_numpy(lists).cuda()
    lneed = ia.lib.fmx_lines_histogram_scratch_bytes(1, len(e))

    def lcall(h=fm.handle, q=1, edges=e, n_edges=len(e), ws_bytes=lneed, out=hist.data_ptr()):
        return ia.lib.fmx_lines_histogram_dev(h, q, d_loff.data_ptr(), d_lines.data_ptr(), None if edges is None else edges.ctypes.data, n_edges,
                                              out, ws.data_ptr(), ws_bytes, stream())

    assert lcall(ws_bytes=lneed - 1) == E_ARG and "fmx_lines_histogram_scratch_bytes" in last_error()
    big = np.arange((1 << 16) + 2, dtype=np.int32)
    bad_edges = (dict(edges=None), dict(n_edges=1), dict(n_edges=-1), dict(edges=np.array([-1, 1, 2], np.int32), n_edges=3),
                 dict(edges=np.array([0, 2, 1], np.int32), n_edges=3))
    for bad in bad_edges + (dict(h=None), dict(n=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(out=None),
                            dict(n=1 << 11, edges=big, n_edges=len(big))):
        assert hcall(**bad) == E_ARG, bad
    for bad in bad_edges + (dict(h=None), dict(q=-1), dict(out=None), dict(q=(1 << 11) + 1, edges=big, n_edges=len(big) - 1)):
        assert lcall(**bad) == E_ARG, bad
    # no line table: the hits form in every case, the lines forms as fmx_match_query_batch; a SuffixArray handle
    bare = ia.FmIndex(HD[:5000], 16, True, device=0)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    try:
        sa.construct()
        assert hcall(h=bare.handle) == E_ARG and "fmx_line_table_build" in last_error()
        assert hcall(h=sa._h) == E_ARG and lcall(h=sa._h) == E_ARG
        for run in (lambda: bare.hit_histogram("blk_", EDGES_250), lambda: bare.hit_histogram("blk_", EDGES_250, where=dict(all="INFO")),
                    lambda: bare.line_histogram(EDGES_250, all="INFO")):
            with pytest.raises(ia.FmxError) as err:
                run()
            assert err.value.code == E_ARG and "fmx_line_table_build" in str(err.value)
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (hist.cpu().numpy() == SENT).all()  # nothing launched, nothing written
    # ... and the exact workspaces serve
    assert hcall() == 0 and lcall(out=hist.data_ptr() + 4 * 16) == 0, last_error()
    torch.cuda.synchronize()
    out = hist.cpu().numpy()
    assert out[:8].tolist() == NAMED_HIST[2][3] and out[16:24].tolist() == judge_bins(e, lists).tolist() and (out[24:] == SENT).all()
    for edges in ([5], [-1, 5], [5, 4], []):
        for run in (lambda: fm.line_histogram(edges, all="INFO"), lambda: fm.hit_histogram("INFO", edges)):
            with pytest.raises(ia.FmxError) as err:
                run()
            assert err.value.code == E_ARG


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_line_histogram_mirror.cpp prints what lineHistogramBatch / lineHistogram / hitHistogramWhereBatch /
    hitHistogramWhere return"""
    o, fm, T = hd
    exe = str(tmp_path / "test_line_histogram_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_line_histogram_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    queries = [NAMED_HIST[0][2], NAMED_HIST[1][2], dict(none=["INFO"])]
    wl = Where("hd16 mirror", o, T, [], queries, [])
    assert out["lines_counts"] == judge_line_hist(wl, EDGES_250).ravel().tolist() == NAMED_HIST[0][3] + NAMED_HIST[1][3] + [0] * 8
    assert out["lines_line_count"] == [310, sum(NAMED_HIST[1][3]), 0] and out["lines_occurrences"] == wl.counts.tolist()
    assert out["lines_status"] == [0] * 4 and out["lines_row1"] == NAMED_HIST[1][3]
    assert out["lines_one"] == judge_bins(EDGES_UNEVEN, wl.query_lines[1]).tolist()
    wh = Where("hd16 mirror", o, T, ["blk_", "blk_", "zzqq#", "INFO "], queries[:2], [-1, 0, 0, 1])
    assert out["hits_counts"] == judge_hit_hist(wh, T, EDGES_250).ravel().tolist()
    assert out["hits_counts"][:16] == NAMED_HIST[2][3] + NAMED_HIST[3][3]
    assert out["hits_occurrences"] == [2468, 2468, 0, 1920] and out["hits_kept"] == wh.kept.tolist() == [2468, 310, 0, 1317]
    assert out["hits_status"] == [0] * 4 and out["hits_term_status"] == [0] * 3
    assert out["hits_one"] == judge_hit_hist(wh, T, EDGES_UNEVEN)[1].tolist() and out["hits_raw_uneven"] == judge_hit_hist(wh, T, EDGES_UNEVEN)[0].tolist()

"""The distinct values of a field per bucket of lines, dc over time, on the GPU: the device stage fmx_values_distinct_histogram_dev
(index4j_amd/csrc/fmx_distinct.hip), the host forms fmx_distinct_values_histogram_where_batch / _where_class_batch and the Python and
C++ conveniences.

The judge is judge_distinct (tests/test_distinct_values_cpu.py), computed once per case and shared; made-up blocks are judged by
judge_distinct_slots (tests/distinct_judges.py).  The device stage runs over the judge's KEPT hits and their groups, uploaded as a
packed block with slots in front of and behind the hits; the host form runs the whole call — the values stage included — and is held
to the invariants against hit_histogram_where_batch, field_values_where_batch and field_values_histogram_where_batch called here.
Every output of the stage is prefilled with a sentinel and padded, and what lies behind the answer must keep it.  Options are set
inside the tests and put back in `finally`.  Every refused call returns before a launch and stores nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from distinct_judges import judge_distinct_slots
from test_distinct_values_cpu import (EDGES_EQUAL, Distinct, assert_fixture_figures, check_distinct, check_invariants, judge_distinct, judged,
                                      made_up_block, slots_of)
from test_field_values_histogram_cpu import EDGES_4097, Hits
from test_field_values_where_cpu import EVERY_LINE, Where
from test_gpu_field_values import ST_NOT_ENABLED, last_error
from test_gpu_locate_rows import _torch, options
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel
E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def dev_slots(fm, hit_off, locs, groups, val_off, edges, short=0):
    """the stage over a packed block (hit_off and val_off: n + 1; locs and groups: one per slot); rc of a refused call — every output
    then keeps its sentinels —, or 0 and a dict with distinct and first_seen.  short: the workspace is that many bytes too small"""
    torch = _torch()
    lib, n, slots, st = ia.lib, len(hit_off) - 1, len(locs), stream()
    d_off = torch.from_numpy(np.asarray(hit_off, np.int64).copy()).cuda()
    d_locs = torch.from_numpy(np.concatenate([np.asarray(locs, np.int32), np.zeros(1, np.int32)])).cuda()
    d_groups = torch.from_numpy(np.concatenate([np.asarray(groups, np.int32), np.zeros(1, np.int32)])).cuda()
    edges_a = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32).copy()
    B = max(len(edges_a) - 1, 1)
    cells = n * B if n * B <= 1 << 27 else 8  # (a call beyond the limit is refused: it must not store)
    distinct = torch.full((cells + PAD,), SENT, dtype=torch.int32, device="cuda")
    first = torch.full((cells + PAD,), SENT, dtype=torch.int32, device="cuda")
    voff = np.asarray(val_off, np.int64).copy()
    use = lib.fmx_values_distinct_histogram_scratch_bytes(n, int(voff[n]), slots, len(edges_a)) - short
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    rc = lib.fmx_values_distinct_histogram_dev(fm.handle, n, voff.ctypes.data, edges_a.ctypes.data if len(edges_a) else None, len(edges_a), d_off.data_ptr(),
                                               d_locs.data_ptr(), slots, d_groups.data_ptr(), distinct.data_ptr(), first.data_ptr(), ws.data_ptr(), use, st)
    voff[:] = -9  # (the call has copied what it needs before it returns)
    edges_a[:] = -9
    torch.cuda.synchronize()
    d, f = distinct.cpu().numpy(), first.cpu().numpy()
    if rc:
        assert (d == SENT).all() and (f == SENT).all(), "a refused call stored"
        return rc, None
    assert (d[cells:] == SENT).all() and (f[cells:] == SENT).all(), "stored beyond the answer"
    return 0, dict(distinct=d[:cells].reshape(n, B), first_seen=f[:cells].reshape(n, B))


def dev_distinct(fm, hits, want, edges, lead=0, extra=0, **kw):
    """... over a judge's hits and groups"""
    hit_off, locs, groups = slots_of(hits, want, lead, extra)
    return dev_slots(fm, hit_off, locs, groups, want.val_off, edges, **kw)


def host_distinct(fm, w, edges, stop, max_len):
    return fm.distinct_values_histogram_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, edges, stop, max_len)


class answer:
    """a host form's dict under the judge's attribute names (check_invariants)"""

    def __init__(self, got):
        self.__dict__.update(got)


def case(tag, fm, o, T, patterns, queries, where_of, edges, stop, max_len, lead=3, extra=70, siblings=False):
    """the judge (once per case), the host form with its invariants and the device stage; siblings: also against the calls that the
    new one replaces"""
    w, want = judged(tag, o, T, patterns, queries, where_of, edges, stop, max_len)
    what = "%s %r" % (tag, patterns)
    got = host_distinct(fm, w, edges, stop, max_len)
    check_distinct(got, want, what + ", host form")
    assert (got["kept"] == want.kept).all() and (got["n_values"] == want.n_values).all() and (got["occurrences"] == w.occurrences).all(), what
    assert (got["status"] == w.status[w.n_terms:]).all() and (got["term_status"] == w.term_status).all(), what  # (the empty pattern has the reference's)
    batches = (*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of)
    hit_hist = fm.hit_histogram_where_batch(*batches, edges) if edges is not None else got["kept"].reshape(w.n, 1)
    check_invariants(answer(got), hit_hist)
    if siblings:
        top = fm.field_values_histogram_where_batch(*batches, edges, 65536, stop, max_len)  # top >= G: every value is a row
        assert (top["n_values"] == got["n_values"]).all() and not top["other"].any(), what
        for i in range(w.n):
            rows = top["hist"][int(top["row_off"][i]):int(top["row_off"][i + 1])]
            assert ((rows > 0).sum(axis=0) == got["distinct"][i]).all(), what
        if edges is not None and len(edges) <= 9:  # the composition the call replaces: one values call per bucket, len() of each
            for b in range(len(edges) - 1):
                val_off = fm.field_values_where_batch(*batches, stop, max_len, (int(edges[b]), int(edges[b + 1])))[3]
                assert (np.diff(val_off) == got["distinct"][:, b]).all(), (what, b)
    if w.kept.sum() > 0:
        rc, dev = dev_distinct(fm, Hits(w.kept_off, w.kept_locs, w.lens), want, edges, lead, extra)
        assert rc == 0, last_error()
        check_distinct(dev, want, what + ", device stage")
    return w, want, got


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


# ---- 1. the fixture's figures ----
def test_fixture_figures(hd):
    """the issue's figures through the host form, the Python convenience and the device stage, each against the judge"""
    o, fm, T = hd

    def get(pattern, stop, max_len, where, edges):
        q = dict(queries=[where], where_of=[0]) if where else dict(queries=[], where_of=[-1])
        w, want, got = case("hd16 dc", fm, o, T, [pattern], q["queries"], q["where_of"], edges, stop, max_len)
        s = fm.distinct_values(pattern, edges, where, stop, max_len)  # the convenience: the same answer
        assert s.distinct == want.distinct[0].tolist() and s.first_seen == want.first_seen[0].tolist()
        assert (s.n_values, s.kept, s.occurrences) == (int(want.n_values[0]), int(want.kept[0]), int(w.occurrences[0]))
        return answer(got)

    assert_fixture_figures(get)
    none = fm.distinct_values("zzzq#", EDGES_250)
    assert none.distinct == [0] * 8 and none.first_seen == [0] * 8 and (none.n_values, none.kept, none.occurrences) == (0, 0, 0)


# ---- 2. the stage against the judge ----
def test_stage_trimmed_blocks(hd):
    """kept hits trimmed to 0, 1, 1,023, 1,024, 1,025 and whole tiles + 1; hit_off[0] != 0 and slots behind the hits; a pattern
    without hits between two with hits and the empty pattern; slots whose group is -1 or beyond the pattern's groups; what lies
    behind every answer keeps the sentinel (dev_slots asserts it)"""
    o, fm, T = hd
    w = Where("hd16 dc", o, T, [" ", "blk_", "zzzq#", "", "1"], [dict(all=["terminating"])], [-1, 0, -1, -1, 0], EVERY_LINE)
    assert w.kept[2] == 0 and w.kept[1] > 0 and w.kept[4] > 0
    for n_hits, lead, extra in ((0, 0, 0), (0, 2, 5), (1, 1, 0), (1023, 0, 1), (1024, 3, 0), (1025, 1023, 1025), (3073, 5, 70), (int(w.kept_off[-1]), 1, 1)):
        hits = Hits(w.kept_off, w.kept_locs, w.lens, n_hits)
        want = judge_distinct(o, T, hits, EDGES_250, " \n", 16)
        rc, dev = dev_distinct(fm, hits, want, EDGES_250, lead, extra)
        assert rc == 0, last_error()
        check_distinct(dev, want, "%d hits, %d in front, %d behind" % (n_hits, lead, extra))  # (nothing at all: both outputs are zeroed)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    want = judge_distinct(o, T, hits, EDGES_250, " \n", 16)
    hit_off, locs, groups = slots_of(hits, want, 1023, 1025)
    groups = groups.copy()
    groups[1023::3] = -1
    groups[1024::7] = 2 ** 31 - 1
    d, f = judge_distinct_slots(hit_off, locs, len(locs), groups, want.val_off, T, EDGES_250)
    assert 0 < d.sum() < want.distinct.sum()
    rc, dev = dev_slots(fm, hit_off, locs, groups, want.val_off, EDGES_250)
    assert rc == 0, last_error()
    check_distinct(dev, Distinct(distinct=d, first_seen=f), "slots without a group")


def test_group_shapes(hd):
    """every hit one value; every hit its own value (the 310 under `terminating`); a value present in every bucket; G = 0"""
    o, fm, T = hd
    _, one, _ = case("hd16 dc", fm, o, T, [" from /10.25", "zzzq#", "INFO dfs.FSNamesystem"], [], [-1, -1, -1], EDGES_250, "01:", 64)
    assert one.n_values.tolist() == [1, 0, 1] and (one.distinct[0] == 1).all() and one.first_seen[2].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    _, own, _ = case("hd16 dc", fm, o, T, ["blk_"], [dict(all=["terminating"])], [0], EDGES_250, " \t\r\n", 32, siblings=True)
    assert own.n_values[0] == 310 and (own.distinct == own.first_seen).all()
    _, every, _ = case("hd16 dc", fm, o, T, [" from /10."], [], [-1], EDGES_250, ".", 64, siblings=True)
    assert (every.distinct == 2).all() and every.first_seen[0].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    # G = 0: hits that have no group at all
    w = Where("hd16 dc", o, T, ["WARN "], [], [-1], EVERY_LINE)
    hit_off, locs = w.kept_off.astype(np.int64), w.kept_locs
    rc, dev = dev_slots(fm, hit_off, locs, np.full(len(locs), -1, np.int32), np.zeros(2, np.int64), EDGES_250)
    assert rc == 0 and not dev["distinct"].any() and not dev["first_seen"].any(), last_error()


def test_edge_shapes(hd):
    """no edges, uneven edges with empty buckets, equal edges, edges beyond the line count, and 4,097 edges (searched in HBM) with n = 1;
    the stage alone over hits that lie in no bucket: they count nowhere, and a group without a hit in a bucket is no first anywhere"""
    o, fm, T = hd
    batch = [" ", "blk_", "zzzq#", "", "1"]
    for edges in (None, EDGES_250, EDGES_UNEVEN, EDGES_EQUAL, EDGES_BEYOND):
        case("hd16 dc", fm, o, T, batch, [dict(all=["terminating"])], [-1, 0, -1, -1, 0], edges, " \n", 16, lead=7, extra=9)
    case("hd16 dc", fm, o, T, ["INFO "], [], [-1], EDGES_4097, " :", 64)
    w = Where("hd16 dc", o, T, ["INFO ", "WARN "], [], [-1, -1], EVERY_LINE)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    want = judge_distinct(o, T, hits, EDGES_UNEVEN, " :", 64)
    assert (want.first_seen.sum(axis=1) < want.n_values).any()
    rc, dev = dev_distinct(fm, hits, want, EDGES_UNEVEN, 2, 3)
    assert rc == 0, last_error()
    check_distinct(dev, want, "hits outside the span")


def test_launch_shapes(hd):
    """1,024-lane workgroups and grids that loop: the stages in front of the new one honour them.  The new stage's grids are
    fmx_hit_lines_geometry's, capped per CU whatever groups_per_cu says: a made-up block of 3 * key_grid * 1024 + 1 slots and more than
    3 * flat_grid * 256 counters, sized from that function, makes every kernel of the new stage pass over its grid at least three
    times (asserted before the run)"""
    o, fm, T = hd
    for kw in (dict(block=1024), dict(groups_per_cu=1), dict(block=1024, groups_per_cu=1)):
        with options(**kw):
            case("hd16 dc", fm, o, T, ["WARN ", "INFO "], [], [-1, -1], EDGES_250, " :", 64)
            case("hd16 dc", fm, o, T, ["blk_"], [dict(all=["terminating"])], [0], EDGES_250, " \t\r\n", 32)

    def grids(items):
        key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
        assert ia.lib.fmx_hit_lines_geometry(fm.handle, items, C.byref(key_grid), C.byref(flat_grid)) == 0
        return key_grid.value, flat_grid.value

    with options(groups_per_cu=1):
        key_cap, flat_cap = grids(10 ** 9)  # (the caps)
        slots, n = 3 * max(key_cap * 1024, flat_cap * 256) + 1, 5
        many = np.arange(3 * flat_cap * 256 // n + 3, dtype=np.int32)  # a bucket per line, most of them beyond the lines; searched in HBM
        counters = n * (len(many) - 1)
        assert 3 * grids(slots)[0] * 1024 < slots and 3 * grids(slots)[1] * 256 < slots  # k_dv_keys' tiles, k_dv_heads' slots
        assert 3 * grids(counters)[1] * 256 < counters <= 1 << 27  # k_dv_counts' counters
        hit_off, locs, groups, val_off = made_up_block(slots, T, n)
        for edges in (many, None):
            d, f = judge_distinct_slots(hit_off, locs, len(locs), groups, val_off, T, edges)
            assert f.sum() > 0 and (edges is None or d.sum() > f.sum())
            rc, dev = dev_slots(fm, hit_off, locs, groups, val_off, edges)
            assert rc == 0, last_error()
            check_distinct(dev, Distinct(distinct=d, first_seen=f), "made-up hits, %s edges" % (None if edges is None else len(edges)))


# ---- 3. the host forms ----
def test_sibling_invariants(hd):
    """every invariant of the definition against the sibling calls: the hits histogram, the top-values call with top >= G, and per
    bucket len() of field_values_where_batch(lines=(edges[b], edges[b + 1])), the composition this call replaces"""
    o, fm, T = hd
    q = dict(all=["blk_"], none=["PacketResponder"])
    case("hd16 dc", fm, o, T, ["INFO ", "zzzq#", "WARN ", "size "], [q], [0, -1, -1, 0], EDGES_250, " :", 64, siblings=True)
    case("hd16 dc", fm, o, T, ["INFO ", "src: /10."], [q], [-1, 0], None, ".: ", 64, siblings=True)
    _, want, got = case("hd16 dc", fm, o, T, ["blk_"], [], [-1], EDGES_250, " \t\r\n", 32, siblings=True)
    assert got["distinct"].sum() == 2200 and got["n_values"][0] == 2199  # one block id is seen in two buckets


def test_class_form_and_ignore_case(hd):
    """class patterns of one spelling give the literal form's answer; on a text of mixed case ignore_case= joins the spellings"""
    o, fm, T = hd
    q = dict(all=["blk_"], none=["PacketResponder"])
    w, want, _ = case("hd16 dc", fm, o, T, ["INFO ", "WARN "], [q], [0, -1], EDGES_250, " :", 64)
    single = lambda ps: ia.pack_class_patterns([list(p) for p in ps])  # noqa: E731
    got = fm.distinct_values_histogram_where_class_batch(*single(["INFO ", "WARN "]), *single(["blk_", "PacketResponder"]), [0, 2], [0, 2], [0, -1], EDGES_250, " :", 64)
    check_distinct(got, want, "class patterns of one spelling")
    assert (got["kept"] == want.kept).all() and (got["n_values"] == want.n_values).all() and (got["status"] == 0).all()
    with pytest.raises(ia.FmxError) as err:
        fm.distinct_values_histogram_where_class_batch(*single(["INFO "]), *single([]), [0], [], [-1], EDGES_250, " :", 64, max_ranges=0)
    assert err.value.code == E_ARG
    text = "Status=200 a\nstatus=200 b\nSTATUS=404 c\nstatus=404 d\nstatus=200 e\nnone\nStatus=500 f\n"
    mixed = ia.FmIndex(text, 4, True, device=0)
    try:
        mixed.build_line_table("\n")
        edges = [0, 3, 7]
        s = mixed.distinct_values("status=", edges, ignore_case=True)  # lines 0 - 2: 200, 404; lines 3 - 6: 404, 200, 500
        assert (s.distinct, s.first_seen, s.n_values, s.kept) == ([2, 3], [2, 1], 3, 6)
        one = mixed.distinct_values("status=", edges)  # the one spelling: 200 | 404, 200
        assert (one.distinct, one.first_seen, one.n_values, one.kept) == ([1, 2], [1, 1], 2, 3)
        w = mixed.distinct_values("status=", edges, where=dict(none=["E"], all=["STATUS"]), ignore_case=True)  # the terms in any case: not line 4
        assert (w.distinct, w.first_seen, w.n_values, w.kept) == ([2, 2], [2, 1], 3, 5)
    finally:
        mixed.close()


def test_no_line_table_and_no_extraction():
    """edges=None without a query needs no line table; with edges, or a query, the refusal names fmx_line_table_build.  An index
    without extraction: FMX_ST_NOT_ENABLED, every counter zero; occurrences and kept are still filled"""
    bare = ia.FmIndex(HD[:40000], 16, True, device=0)
    plain = ia.FmIndex(HD[:40000], 16, False, device=0)
    try:
        s = bare.distinct_values("INFO ", stop=" :")
        assert s.distinct == s.first_seen == [len(bare.field_values("INFO ", " :", 64))] and s.kept == HD[:40000].count("INFO ")
        for kw in (dict(edges=[0, 100]), dict(where=dict(all=["blk_"]))):
            with pytest.raises(ia.FmxError) as err:
                bare.distinct_values("INFO ", **kw)
            assert err.value.code == E_ARG and "fmx_line_table_build" in str(err.value)
        plain.build_line_table("\n")
        out = plain.distinct_values_histogram_where_batch(*ia.pack_patterns([ia.as_chars("INFO "), ia.as_chars("blk_")]), *ia.pack_patterns([]), [0], [], [-1, -1],
                                                          [0, 100, 200], " :", 64)
        assert (out["status"] == ST_NOT_ENABLED).all() and not out["distinct"].any() and not out["first_seen"].any() and not out["n_values"].any()
        lines = HD[:40000].split("\n")[:200]
        assert out["kept"].tolist() == [sum(ln.count("INFO ") for ln in lines), sum(ln.count("blk_") for ln in lines)]
        assert out["occurrences"].tolist() == [HD[:40000].count("INFO "), HD[:40000].count("blk_")]
        out = plain.distinct_values_histogram_where_batch(*ia.pack_patterns([ia.as_chars("INFO ")]), *ia.pack_patterns([]), [0], [], [-1], None, " :", 64)
        assert (out["status"] == ST_NOT_ENABLED).all() and out["kept"].tolist() == out["occurrences"].tolist() and not out["distinct"].any()
    finally:
        bare.close()
        plain.close()


# ---- 4. refusals ----
def test_refusals(hd):
    """each returns before a launch and leaves every output untouched (dev_slots asserts the sentinels; the host form's arrays keep
    their fill)"""
    o, fm, T = hd
    w = Where("hd16 dc", o, T, ["INFO "], [], [-1], EVERY_LINE)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    want = judge_distinct(o, T, hits, EDGES_250, " :", 8)
    assert dev_distinct(fm, hits, want, EDGES_250)[0] == 0
    for edges, word in (([0, 5, 4], "edges"), ([7], "edges"), ([-1, 4], "edge")):
        rc, _ = dev_distinct(fm, hits, want, edges)
        assert rc == E_ARG and word in last_error(), (edges, rc, last_error())
    rc, _ = dev_slots(fm, np.zeros(65537, np.int64), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(65537, np.int64), list(range(2050)))
    assert rc == E_ARG and "2^27" in last_error(), (rc, last_error())  # 65,536 patterns * 2,049 buckets
    rc, _ = dev_slots(fm, w.kept_off, w.kept_locs, want.group_of_hit, np.array([0, 2 ** 31], np.int64), EDGES_250)
    assert rc == E_ARG and "val_off" in last_error(), (rc, last_error())
    rc, _ = dev_distinct(fm, hits, want, EDGES_250, short=1)
    assert rc == E_ARG and "fmx_values_distinct_histogram_scratch_bytes" in last_error(), (rc, last_error())
    # no line table with edges; a handle that is not resident; a SuffixArray handle
    bare = ia.FmIndex(HD[:4000], 16, True, device=0)
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    pat, off = ia.pack_patterns([ia.as_chars("INFO ")])
    off = off.astype(np.int32)

    def host_call(h=fm.handle, edges=(0, 1000, 2000), max_len=8, where_of=(-1,)):
        e = np.asarray(edges, np.int32)
        ints = {k: np.full(8, SENT, np.int32) for k in ("distinct", "first_seen", "n_values", "occurrences", "kept", "status")}
        stop, qoff, kinds, wo = ia.as_chars(" :").astype(np.uint16), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.array(where_of, np.int32)
        tch, toff = np.zeros(1, np.uint16), np.zeros(1, np.int32)
        rc = ia.lib.fmx_distinct_values_histogram_where_batch(h, pat.ctypes.data, off.ctypes.data, 1, tch.ctypes.data, toff.ctypes.data, 0, qoff.ctypes.data,
                                                              kinds.ctypes.data, 0, wo.ctypes.data, e.ctypes.data if len(e) else None, len(e), stop.ctypes.data, 2,
                                                              max_len, ints["distinct"].ctypes.data, ints["first_seen"].ctypes.data, ints["n_values"].ctypes.data,
                                                              ints["occurrences"].ctypes.data, ints["kept"].ctypes.data, ints["status"].ctypes.data, None)
        return rc, all((a == SENT).all() for a in ints.values()), ints

    try:
        sa.construct()
        rc, _, ints = host_call()
        assert rc == 0 and (ints["distinct"][2:] == SENT).all() and 0 < ints["first_seen"][:2].sum() == ints["n_values"][0], last_error()
        for kw, code, word in ((dict(edges=(0, 5, 4)), E_ARG, "edges"), (dict(max_len=65), E_ARG, "max_len"), (dict(where_of=(0,)), E_ARG, "where_of"),
                               (dict(h=bare.handle), E_ARG, "fmx_line_table_build"), (dict(h=host_only.handle), E_NO_DEVICE, ""), (dict(h=sa._h), E_ARG, "")):
            rc, untouched, _ = host_call(**kw)
            assert rc == code and word in last_error() and untouched, (kw, rc, last_error(), untouched)
        torch = _torch()
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        p, voff, e2 = t.data_ptr(), np.array([0, 1], np.int64), np.array([0, 10], np.int32)
        for h, code, word in ((bare.handle, E_ARG, "fmx_line_table_build"), (host_only.handle, E_NO_DEVICE, ""), (sa._h, E_ARG, "")):
            assert ia.lib.fmx_values_distinct_histogram_dev(h, 1, voff.ctypes.data, e2.ctypes.data, 2, p, p, 4, p, p, p, p, 1 << 20, stream()) == code
            assert word in last_error()
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0).all()
    finally:
        bare.close()
        host_only.close()


# ---- 5. the C++ mirror ----
def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_distinct_values_mirror.cpp prints what distinctValuesBatch returns, and holds distinctValues to the fixture's
    figures"""
    o, fm, T = hd
    exe = str(tmp_path / "test_distinct_values_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_distinct_values_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    w, want = judged("hd16 dc", o, T, ["INFO ", "zzzq#", "WARN "], [dict(all=["blk_"], none=["PacketResponder"])], [0, -1, -1], EDGES_250, " :", 64)
    assert out["distinct"] == want.distinct.ravel().tolist() and out["first_seen"] == want.first_seen.ravel().tolist()
    assert out["n_values"] == want.n_values.tolist() and out["kept"] == want.kept.tolist() and out["occurrences"] == w.occurrences.tolist()
    assert out["status"] == [0] * 3

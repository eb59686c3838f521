"""The top values of a field per bucket of lines, the stacked timeline, on the GPU: the device stages fmx_values_top_histogram_dev and
fmx_values_gather_rows_dev (index4j_amd/csrc/fmx_value_hist.hip) behind fmx_values_of_hits_groups_dev and fmx_values_fill_dev, the host
forms fmx_field_values_histogram_where_batch / _where_class_batch and the Python and C++ conveniences.

The judge is judge_top_hist (tests/test_field_values_histogram_cpu.py), computed once per case and shared.  The device stages run
over the judge's KEPT hits, uploaded as a packed block with slots in front of and behind the hits; the host form runs the whole
call and is held to the invariants against hit_histogram_where_batch and field_values_where_batch called here.  Every output of a
stage is prefilled with a sentinel and padded, and what lies behind the answer must keep it.  Options are set inside the tests and
put back in `finally`.  Every refused call returns before a launch and stores nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_histogram_cpu import (EDGES_4097, Hits, assert_fixture_figures, check_invariants, check_top_hist, judge_top_hist, judged,
                                              span)
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


def filled(count, dtype):
    torch = _torch()
    return torch.full((count + PAD,), SENT, dtype=dtype, device="cuda")


def cut(t, count, what):
    a = t.cpu().numpy()
    assert (a[count:] == SENT).all(), "stored beyond the answer: " + what
    return a[:count]


def dev_top_hist(fm, hits, edges, top, stop, max_len, lead=0, extra=0, short=None):
    """the values stage, the new stage, the fill and the gather over packed hits with `lead` slots in front (hit_off[0] = lead) and
    `extra` behind; rc of the stage that refused (and its name), or 0 and a dict under the judge's names.  short = (stage, bytes):
    that stage gets a workspace that many bytes too small"""
    torch = _torch()
    lib, n, st = ia.lib, hits.n, stream()
    total = int(hits.kept_off[-1])
    slots, K = lead + total + extra, total + extra
    hit_off = torch.from_numpy((hits.kept_off + lead).astype(np.int64)).cuda()
    own_off = torch.from_numpy(hits.kept_off.astype(np.int64)).cuda()  # (the values stage takes offsets that start at 0)
    locs = torch.from_numpy(np.concatenate([np.full(lead, -5, np.int32), hits.kept_locs, np.full(extra, -5, np.int32), np.zeros(1, np.int32)])).cuda()
    edges_a = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32).copy()
    B = max(len(edges_a) - 1, 1)

    def ws_of(stage, need):
        use = need - (short[1] if short and short[0] == stage else 0)
        return torch.empty(max(use, 1), dtype=torch.uint8, device="cuda"), use

    # the groups of the kept hits and the group of every hit (slots behind own_off[n] are no hits)
    val_off, count, text_off = filled(n + 1, torch.int64), filled(max(K, 1), torch.int32), filled(max(K, 1) + 1, torch.int64)
    group = torch.full((slots + PAD,), SENT, dtype=torch.int32, device="cuda")
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    tl, sp = np.array(hits.lens, np.int32), ia.as_chars(stop).astype(np.uint16)
    ws_b, use_b = ws_of("b", lib.fmx_values_of_hits_groups_scratch_bytes(n, K, max_len))
    rc = lib.fmx_values_of_hits_groups_dev(fm.handle, n, tl.ctypes.data, sp.ctypes.data if len(sp) else None, len(sp), max_len, own_off.data_ptr(),
                                           locs.data_ptr() + 4 * lead, K, val_off.data_ptr(), count.data_ptr(), text_off.data_ptr(),
                                           group.data_ptr() + 4 * lead, status.data_ptr(), ws_b.data_ptr(), use_b, st)
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    voff = cut(val_off, n + 1, "val_off").astype(np.int64).copy()
    G = int(voff[n])
    row_off_want = np.concatenate([[0], np.cumsum(np.minimum(np.diff(voff), top))]).astype(np.int64)
    R = int(row_off_want[n])
    got = dict(val_off=voff.copy(), counts=count.cpu().numpy()[:G], group_of_hit=group.cpu().numpy()[lead:lead + total])
    # the ranks, the rows and the counters
    row_off, row_group, row_count = filled(n + 1, torch.int64), filled(R, torch.int32), filled(R, torch.int32)
    hist, other = filled(R * B, torch.int32), filled(n * B, torch.int32)
    ws_h, use_h = ws_of("h", lib.fmx_values_top_histogram_scratch_bytes(n, G, slots, len(edges_a)))
    rc = lib.fmx_values_top_histogram_dev(fm.handle, n, voff.ctypes.data, top, edges_a.ctypes.data if len(edges_a) else None, len(edges_a),
                                          hit_off.data_ptr(), locs.data_ptr(), slots, count.data_ptr(), group.data_ptr(), row_off.data_ptr(),
                                          row_group.data_ptr(), row_count.data_ptr(), hist.data_ptr(), other.data_ptr(), ws_h.data_ptr(), use_h, st)
    keep = voff.copy()
    voff[:] = -9  # (the call has copied what it needs before it returns)
    edges_a[:] = -9
    torch.cuda.synchronize()
    if rc:
        assert all((t.cpu().numpy() == SENT).all() for t in (row_off, row_group, row_count, hist, other))
        return rc, "h"
    got.update(row_off=cut(row_off, n + 1, "row_off"), row_group=cut(row_group, R, "row_group"), row_count=cut(row_count, R, "row_count"),
               hist=cut(hist, R * B, "hist").reshape(R, B), other=cut(other, n * B, "other").reshape(n, B))
    assert (got["row_off"] == row_off_want).all()
    # the text of ALL groups, then the rows' alone
    units = int(text_off.cpu().numpy()[G]) if G else 0
    chars = torch.full((units + PAD,), 0x7A7A, dtype=torch.int16, device="cuda")
    if G:
        assert lib.fmx_values_fill_dev(fm.handle, G, text_off.data_ptr(), chars.data_ptr(), ws_b.data_ptr(), max(use_b, 0), st) == 0, last_error()
    row_text_off, row_chars = filled(R + 1, torch.int64), torch.full((units + PAD,), 0x7B7B, dtype=torch.int16, device="cuda")
    ws_g, use_g = ws_of("g", lib.fmx_values_gather_rows_scratch_bytes(n, R))
    rc = lib.fmx_values_gather_rows_dev(fm.handle, n, keep.ctypes.data, top, units, row_group.data_ptr(), text_off.data_ptr(), chars.data_ptr(),
                                        row_text_off.data_ptr(), row_chars.data_ptr(), ws_g.data_ptr(), use_g, st)
    keep[:] = -9
    torch.cuda.synchronize()
    if rc:
        assert (row_text_off.cpu().numpy() == SENT).all() and (row_chars.cpu().numpy() == 0x7B7B).all()
        return rc, "g"
    got["text_off"] = cut(row_text_off, R + 1, "row_text_off")
    c = row_chars.cpu().numpy()
    row_units = int(got["text_off"][R])
    assert (c[row_units:] == 0x7B7B).all(), "stored beyond the answer: row_chars"
    got["chars"] = c[:row_units].view(np.uint16)
    assert (status.cpu().numpy() == 0).all()
    return 0, got


def host_top_hist(fm, w, edges, top, stop, max_len):
    return fm.field_values_histogram_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, edges, top, stop, max_len)


def case(tag, fm, o, T, patterns, queries, where_of, edges, top, stop, max_len, device=True, lead=3, extra=70):
    """the judge (once per case), the host form with its invariants and the device stages"""
    w, want = judged(tag, o, T, patterns, queries, where_of, edges, top, stop, max_len)
    what = "%s %r top %d" % (tag, patterns, top)
    got = host_top_hist(fm, w, edges, top, stop, max_len)
    check_top_hist(got, want, what + ", host form")
    assert (got["kept"] == want.kept).all() and (got["n_values"] == want.n_values).all() and (got["occurrences"] == w.occurrences).all(), what
    assert (got["status"] == w.status[w.n_terms:]).all() and (got["term_status"] == w.term_status).all(), what  # (the empty pattern has the reference's)
    # the invariants, against the sibling calls made here
    assert (got["hist"].sum(axis=1) == got["row_count"]).all(), what
    if edges is not None:
        hit_hist = fm.hit_histogram_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, edges)
    else:
        hit_hist = got["kept"].reshape(w.n, 1)
    check_invariants(ia_answer(got, top), hit_hist)
    chars, text_off, counts, val_off = fm.field_values_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, stop, max_len,
                                                                   None if edges is None else span(edges))[:4]
    assert (np.diff(val_off) == got["n_values"]).all(), what
    for i in range(w.n):
        a, b = int(got["row_off"][i]), int(got["row_off"][i + 1])
        g = val_off[i] + got["row_group"][a:b]
        assert (counts[g] == got["row_count"][a:b]).all(), what
        for r, gg in zip(range(a, b), g):
            assert (got["chars"][got["text_off"][r]:got["text_off"][r + 1]] == chars[text_off[gg]:text_off[gg + 1]]).all(), what
        if top >= got["n_values"][i]:
            assert sorted(got["row_group"][a:b].tolist()) == list(range(b - a)) and not got["other"][i].any(), what
    if device and w.kept.sum() > 0:
        rc, dev = dev_top_hist(fm, Hits(w.kept_off, w.kept_locs, w.lens), edges, top, stop, max_len, lead, extra)
        assert rc == 0, (dev, last_error())
        assert (dev["val_off"] == want.val_off).all() and (dev["counts"] == want.counts).all() and (dev["group_of_hit"] == want.group_of_hit).all(), what
        check_top_hist(dev, want, what + ", device stages")
    return w, want, got


class ia_answer:
    """a host form's dict under the judge's attribute names (check_invariants)"""

    def __init__(self, got, top):
        self.n, self.top = len(got["n_values"]), top
        for k in ("row_off", "row_group", "row_count", "hist", "other", "n_values"):
            setattr(self, k, got[k])


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
    """the issue's figures through the host form, the Python convenience and the device stages, each against the judge"""
    o, fm, T = hd

    def get(pattern, stop, top, where):
        q = dict(queries=[where], where_of=[0]) if where else dict(queries=[], where_of=[-1])
        w, want, got = case("hd16 top", fm, o, T, [pattern], q["queries"], q["where_of"], EDGES_250, top, stop, 64)
        s = fm.field_values_histogram(pattern, EDGES_250, top, where, stop)  # the convenience: the same rows
        assert [(r["value"], r["count"], r["hist"]) for r in s.rows] == want.rows() and [r["group"] for r in s.rows] == want.row_group.tolist()
        assert s.other == want.other[0].tolist() and (s.n_values, s.kept, s.occurrences) == (int(want.n_values[0]), int(want.kept[0]), int(w.occurrences[0]))
        return want

    assert_fixture_figures(get)
    # edges=None: the device-side top-k of field_values
    top5 = fm.field_values_histogram("INFO ", top=5, stop=" :")
    assert [(r["value"], r["count"]) for r in top5.rows] == fm.field_values("INFO ", " :", 64, top=5) and [r["hist"] for r in top5.rows] == [[r["count"]] for r in top5.rows]
    assert top5.other == [1920 - sum(r["count"] for r in top5.rows)] and top5.by_value()["dfs.FSNamesystem"]["count"] == 525
    assert fm.field_values_histogram("zzzq#", EDGES_250).rows == [] and fm.field_values_histogram("zzzq#", EDGES_250).other == [0] * 8


# ---- 2. the stage against the judge ----
def test_stage_trimmed_blocks(hd):
    """kept hits trimmed to 0, 1, 1,023, 1,024, 1,025 and whole tiles + 1; hit_off[0] != 0 and slots behind the hits; a pattern
    without hits between two with hits; what lies behind every answer keeps the sentinel (dev_top_hist asserts it)"""
    o, fm, T = hd
    w = Where("hd16 top", o, T, [" ", "blk_", "zzzq#", "", "1"], [dict(all=["terminating"])], [-1, 0, -1, -1, 0], EVERY_LINE)
    assert w.kept[2] == 0 and w.kept[1] > 0 and w.kept[4] > 0
    for n_hits, lead, extra in ((0, 0, 0), (0, 2, 5), (1, 1, 0), (1023, 0, 1), (1024, 3, 0), (1025, 1023, 1025), (3073, 5, 70), (int(w.kept_off[-1]), 1, 1)):
        hits = Hits(w.kept_off, w.kept_locs, w.lens, n_hits)
        want = judge_top_hist(o, T, hits, EDGES_250, 6, " \n", 16)
        rc, dev = dev_top_hist(fm, hits, EDGES_250, 6, " \n", 16, lead, extra)
        assert rc == 0, (dev, last_error())
        if n_hits + lead + extra == 0:  # (nothing at all: the rows' offsets and `other` are zeroed)
            assert not dev["row_off"].any() and not dev["other"].any()
            continue
        check_top_hist(dev, want, "%d hits, %d in front, %d behind" % (n_hits, lead, extra))


def test_group_shapes(hd):
    """G of 0, 1, top - 1, top and top + 1; every hit one value; every hit its own value (310 values of count 1: the whole selection
    is the tie rule); ties across the cut; top = 1 and top >= G"""
    o, fm, T = hd
    for top in (1, 2, 3):  # G = 2
        case("hd16 top", fm, o, T, [" from /10."], [], [-1], EDGES_250, top, ".", 64)
    _, one, _ = case("hd16 top", fm, o, T, [" from /10.25", "zzzq#", "INFO dfs.FSNamesystem"], [], [-1, -1, -1], EDGES_250, 3, "01:", 64)
    assert one.n_values.tolist() == [1, 0, 1] and one.row_count.tolist() == [222, 525]
    _, own, _ = case("hd16 top", fm, o, T, ["blk_"], [dict(all=["terminating"])], [0], EDGES_250, 7, " \t\r\n", 32)
    assert own.n_values[0] == 310 and own.row_group.tolist() == list(range(7)) and own.other.sum() == 303
    _, ties, _ = case("hd16 top", fm, o, T, ["WARN "], [], [-1], EDGES_250, 4, " :", 64)
    assert ties.row_count.tolist() == [62, 1, 1, 1]
    for top in (1, 19, 20, 65536):
        case("hd16 top", fm, o, T, ["WARN ", "INFO "], [], [-1, -1], EDGES_250, top, " :", 64)


def test_edge_shapes(hd):
    """no edges, uneven edges with empty buckets, edges beyond the line count, and 4,097 edges (searched in HBM) with n = 1, top = 2;
    the stage alone over hits that lie in no bucket"""
    o, fm, T = hd
    batch = [" ", "blk_", "zzzq#", "", "1"]
    for edges in (None, EDGES_250, EDGES_UNEVEN, EDGES_BEYOND):
        case("hd16 top", fm, o, T, batch, [dict(all=["terminating"])], [-1, 0, -1, -1, 0], edges, 6, " \n", 16, lead=7, extra=9)
    case("hd16 top", fm, o, T, ["INFO "], [], [-1], EDGES_4097, 2, " :", 64)
    w = Where("hd16 top", o, T, ["INFO ", "WARN "], [], [-1, -1], EVERY_LINE)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    want = judge_top_hist(o, T, hits, EDGES_UNEVEN, 3, " :", 64)
    rc, dev = dev_top_hist(fm, hits, EDGES_UNEVEN, 3, " :", 64, 2, 3)
    assert rc == 0, (dev, last_error())
    check_top_hist(dev, want, "hits outside the span")


def test_launch_shapes(hd):
    """1,024-lane workgroups and grids that loop: the range stage, the fill and the packed extract in front of the new stage honour them"""
    o, fm, T = hd
    for kw in (dict(block=1024), dict(groups_per_cu=1), dict(block=1024, groups_per_cu=1)):
        with options(**kw):
            case("hd16 top", fm, o, T, ["WARN ", "INFO "], [], [-1, -1], EDGES_250, 19, " :", 64)
            case("hd16 top", fm, o, T, ["blk_"], [dict(all=["terminating"])], [0], EDGES_250, 7, " \t\r\n", 32)


# ---- 3. the host forms ----
def test_class_form_and_ignore_case(hd):
    """class patterns of one spelling give the literal form's answer; on a text of mixed case ignore_case= joins the spellings: a
    value's row is the sum of its rows over the spellings"""
    o, fm, T = hd
    q = dict(all=["blk_"], none=["PacketResponder"])
    w, want, _ = case("hd16 top", fm, o, T, ["INFO ", "WARN "], [q], [0, -1], EDGES_250, 3, " :", 64)
    single = lambda ps: ia.pack_class_patterns([list(p) for p in ps])  # noqa: E731
    got = fm.field_values_histogram_where_class_batch(*single(["INFO ", "WARN "]), *single(["blk_", "PacketResponder"]), [0, 2], [0, 2], [0, -1], EDGES_250, 3, " :", 64)
    check_top_hist(got, want, "class patterns of one spelling")
    assert (got["kept"] == want.kept).all() and (got["n_values"] == want.n_values).all() and (got["status"] == 0).all()
    with pytest.raises(ia.FmxError) as err:
        fm.field_values_histogram_where_class_batch(*single(["INFO "]), *single([]), [0], [], [-1], EDGES_250, 3, " :", 64, max_ranges=0)
    assert err.value.code == E_ARG
    text = "Status=200 a\nstatus=200 b\nSTATUS=404 c\nstatus=404 d\nstatus=200 e\nnone\nStatus=500 f\n"
    mixed = ia.FmIndex(text, 4, True, device=0)
    try:
        mixed.build_line_table("\n")
        edges = [0, 3, 7]
        s = mixed.field_values_histogram("status=", edges, 2, ignore_case=True)
        assert [(r["value"], r["count"], r["hist"]) for r in s.rows] == [("200", 3, [2, 1]), ("404", 2, [1, 1])] and s.other == [0, 1]
        assert (s.n_values, s.kept) == (3, 6)
        total = {}
        for spelling in ("status=", "Status=", "STATUS="):
            for r in mixed.field_values_histogram(spelling, edges, 10).rows:
                total[r["value"]] = [a + b for a, b in zip(total.get(r["value"], [0, 0]), r["hist"])]
        assert all(total[r["value"]] == r["hist"] for r in s.rows) and total["500"] == s.other
        w = mixed.field_values_histogram("status=", edges, 2, where=dict(none=["E"], all=["STATUS"]), ignore_case=True)  # the terms in any case
        assert [(r["value"], r["hist"]) for r in w.rows] == [("200", [2, 0]), ("404", [1, 1])] and w.other == [0, 1] and w.kept == 5
    finally:
        mixed.close()


def test_no_line_table_and_no_extraction():
    """edges=None without a query needs no line table; with edges, or a query, the refusal names fmx_line_table_build.  An index
    without extraction: FMX_ST_NOT_ENABLED, no rows, `other` zero; occurrences and kept are still filled"""
    bare = ia.FmIndex(HD[:40000], 16, True, device=0)
    plain = ia.FmIndex(HD[:40000], 16, False, device=0)
    try:
        s = bare.field_values_histogram("INFO ", top=3, stop=" :")
        assert [(r["value"], r["count"]) for r in s.rows] == bare.field_values("INFO ", " :", 64, top=3) and s.kept == HD[:40000].count("INFO ")
        for kw in (dict(edges=[0, 100]), dict(where=dict(all=["blk_"]))):
            with pytest.raises(ia.FmxError) as err:
                bare.field_values_histogram("INFO ", **kw)
            assert err.value.code == E_ARG and "fmx_line_table_build" in str(err.value)
        plain.build_line_table("\n")
        out = plain.field_values_histogram_where_batch(*ia.pack_patterns([ia.as_chars("INFO "), ia.as_chars("blk_")]), *ia.pack_patterns([]), [0], [], [-1, -1],
                                                       [0, 100, 200], 3, " :", 64)
        assert (out["status"] == ST_NOT_ENABLED).all() and out["row_off"].tolist() == [0, 0, 0] and not out["other"].any() and not out["n_values"].any()
        lines = HD[:40000].split("\n")[:200]
        assert out["kept"].tolist() == [sum(ln.count("INFO ") for ln in lines), sum(ln.count("blk_") for ln in lines)]
        assert out["occurrences"].tolist() == [HD[:40000].count("INFO "), HD[:40000].count("blk_")]
        out = plain.field_values_histogram_where_batch(*ia.pack_patterns([ia.as_chars("INFO ")]), *ia.pack_patterns([]), [0], [], [-1], None, 3, " :", 64)
        assert (out["status"] == ST_NOT_ENABLED).all() and out["kept"].tolist() == out["occurrences"].tolist() and not out["other"].any()
    finally:
        bare.close()
        plain.close()


# ---- 4. refusals ----
def test_refusals(hd):
    """each returns before a launch and leaves every output untouched (dev_top_hist asserts the sentinels; the host form's arrays
    keep their fill)"""
    o, fm, T = hd
    w = Where("hd16 top", o, T, ["INFO "], [], [-1], EVERY_LINE)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    assert dev_top_hist(fm, hits, EDGES_250, 3, " :", 8)[0] == 0
    for kw, word in ((dict(top=0), "top"), (dict(top=65537), "top"), (dict(edges=[0, 5, 4]), "edges"), (dict(edges=[7]), "edges"),
                     (dict(edges=[-1, 4]), "edge"), (dict(top=65536, edges=list(range(2050))), "2^27")):
        args = dict(edges=EDGES_250, top=3)
        args.update(kw)
        rc, where = dev_top_hist(fm, hits, args["edges"], args["top"], " :", 8)
        assert rc == E_ARG and where == "h" and word in last_error(), (kw, rc, where, last_error())
    for stage, word in (("h", "fmx_values_top_histogram_scratch_bytes"), ("g", "fmx_values_gather_rows_scratch_bytes")):
        rc, where = dev_top_hist(fm, hits, EDGES_250, 3, " :", 8, short=(stage, 1))
        assert rc == E_ARG and where == stage and word in last_error(), (stage, rc, where, last_error())
    # no line table with edges; a handle that is not resident; a SuffixArray handle
    bare = ia.FmIndex(HD[:4000], 16, True, device=0)
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    pat, off = ia.pack_patterns([ia.as_chars("INFO ")])
    off = off.astype(np.int32)

    def host_call(h=fm.handle, top=3, edges=(0, 1000, 2000), max_len=8, where_of=(-1,)):
        e = np.asarray(edges, np.int32)
        ints = {k: np.full(8, SENT, np.int32) for k in ("n_values", "other", "occurrences", "kept", "status")}
        row_off = np.full(4, SENT, np.int64)
        ptrs = [C.c_void_p(0x5A5A) for _ in range(5)]
        stop, qoff, kinds, wo = ia.as_chars(" :").astype(np.uint16), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.array(where_of, np.int32)
        tch, toff = np.zeros(1, np.uint16), np.zeros(1, np.int32)
        rc = ia.lib.fmx_field_values_histogram_where_batch(h, pat.ctypes.data, off.ctypes.data, 1, tch.ctypes.data, toff.ctypes.data, 0, qoff.ctypes.data,
                                                           kinds.ctypes.data, 0, wo.ctypes.data, e.ctypes.data if len(e) else None, len(e), top, stop.ctypes.data,
                                                           2, max_len, ints["n_values"].ctypes.data, row_off.ctypes.data, *(C.byref(p) for p in ptrs),
                                                           ints["other"].ctypes.data, ints["occurrences"].ctypes.data, ints["kept"].ctypes.data,
                                                           ints["status"].ctypes.data, None)
        untouched = all((a == SENT).all() for a in list(ints.values()) + [row_off])
        return rc, untouched, [p.value for p in ptrs]

    try:
        sa.construct()
        rc, _, ptrs = host_call()
        assert rc == 0 and ptrs[0] not in (None, 0x5A5A), last_error()
        ia.lib.fmx_free_buffer(C.c_void_p(ptrs[0]))
        for kw, code, word in ((dict(top=0), E_ARG, "top"), (dict(top=65537), E_ARG, "top"), (dict(top=65536, edges=tuple(range(2050))), E_ARG, "2^27"),
                               (dict(edges=(0, 5, 4)), E_ARG, "edges"), (dict(max_len=65), E_ARG, "max_len"), (dict(where_of=(0,)), E_ARG, "where_of"),
                               (dict(h=bare.handle), E_ARG, "fmx_line_table_build"), (dict(h=host_only.handle), E_NO_DEVICE, ""), (dict(h=sa._h), E_ARG, "")):
            rc, untouched, ptrs = host_call(**kw)
            assert rc == code and word in last_error() and untouched and all(p is None for p in ptrs), (kw, rc, last_error(), untouched, ptrs)
        torch = _torch()
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        p, voff, e2 = t.data_ptr(), np.array([0, 1], np.int64), np.array([0, 10], np.int32)
        for h, code, word in ((bare.handle, E_ARG, "fmx_line_table_build"), (host_only.handle, E_NO_DEVICE, ""), (sa._h, E_ARG, "")):
            assert ia.lib.fmx_values_top_histogram_dev(h, 1, voff.ctypes.data, 3, e2.ctypes.data, 2, p, p, 4, p, p, p, p, p, p, p, p, 1 << 20, stream()) == code
            assert word in last_error()
        for h, code in ((host_only.handle, E_NO_DEVICE), (sa._h, E_ARG)):
            assert ia.lib.fmx_values_gather_rows_dev(h, 1, voff.ctypes.data, 3, 4, p, p, p, p, p, p, 1 << 20, stream()) == code
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0).all()
    finally:
        bare.close()
        host_only.close()


# ---- 5. the C++ mirror ----
def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_field_values_histogram_mirror.cpp prints what fieldValuesHistogramBatch returns, and holds fieldValuesHistogram to
    the fixture's figures"""
    o, fm, T = hd
    exe = str(tmp_path / "test_field_values_histogram_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_field_values_histogram_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    w, want = judged("hd16 top", o, T, ["INFO ", "zzzq#", "WARN "], [dict(all=["blk_"], none=["PacketResponder"])], [0, -1, -1], EDGES_250, 4, " :", 64)
    assert out["row_off"] == want.row_off.tolist() and out["row_count"] == want.row_count.tolist() and out["row_group"] == want.row_group.tolist()
    assert out["hist"] == want.hist.ravel().tolist() and out["other"] == want.other.ravel().tolist() and out["n_values"] == want.n_values.tolist()
    assert out["kept"] == want.kept.tolist() and out["occurrences"] == w.occurrences.tolist() and out["status"] == [0] * 3
    assert out["values"] == [u for v in want.strings() for u in [ord(c) for c in v] + [0xFFFF]]

"""Statistics of the number behind a pattern, by the value of a field of the same line, per bucket of lines, on the GPU: the device
stage fmx_numbers_by_key_buckets_dev (fmx_by_hist.hip) behind stages a and b of "stats ... by", the text of its key rows through
fmx_values_fill_dev and fmx_values_gather_rows_dev, the host forms fmx_number_stats_by_histogram_batch /
fmx_number_stats_by_histogram_class_batch and the Python convenience FmIndex.number_stats_by_histogram.

The judge is judge_by_hist (tests/test_number_stats_by_histogram_cpu.py), computed once per case and shared; on the edge text the
regular expressions of that file judge the judge.  The device stage runs over the judge's KEPT hits, uploaded as one packed block
with 3 slots in front of and 70 behind the hits; the host form runs the whole call.  Every output is prefilled with a sentinel and
padded by 64 entries that must keep it; whole arrays are compared.  Options are set inside the tests and put back in `finally`.
Every refused call returns before a launch."""
import ctypes as C

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_where_cpu import Where
from test_gpu_field_values import ST_NOT_ENABLED, last_error
from test_gpu_locate_rows import _torch, options
from test_gpu_number_stats_by import PAD, Block, cut, filled, stream
from test_gpu_stage_loops import TILE, LANES, WS_LIMIT, geometry
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_stats_by_cpu import EDGE_KEYS, EDGE_LINES, EDGE_NUMBERS, edge_text
from test_number_stats_by_histogram_cpu import EDGES_EMPTY, assert_fixture_figures, assert_regex, check_by_hist, judged, span

pytestmark = pytest.mark.gpu

HD = hdfs_text()
E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
CELL_NAMES = ("count", "sum_lo", "sum_hi", "min", "max", "pct", "no_key", "not_number", "overflow")
CHAR_SENT = 0x7A7A


def dev_by_hist(fm, w, m, by_of, stop, max_len, edges, top, permille=(500, 950), frac_digits=0, lead=3, extra=70, short=0, base=None):
    """stages a and b, the new stage and the text of its key rows over a Block; rc of the new stage and None where it refused (every
    output then keeps the sentinel), or 0 and a dict under the judge's names.  short: the new stage's workspace is that many bytes
    too small.  base: judge_by's answer, to hold stages a and b to"""
    torch = _torch()
    lib, n, st = ia.lib, w.n - m, stream()
    b = Block(w, lead, extra)
    key_end = int(w.kept_off[m]) + lead
    a_slots = min(b.slots, key_end + extra)
    K = max(int(w.kept_off[m]), 1)
    first_off, first_lines, first_locs = filled(m + 1, torch.int64), filled(K, torch.int32), filled(K, torch.int32)
    need = lib.fmx_first_hits_of_lines_scratch_bytes(m, a_slots)
    ws_a = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    assert lib.fmx_first_hits_of_lines_dev(fm.handle, m, b.hit_off.data_ptr(), b.locs.data_ptr(), a_slots, first_off.data_ptr(), first_lines.data_ptr(),
                                           first_locs.data_ptr(), ws_a.data_ptr(), need, st) == 0, last_error()
    val_off, lines, text_off, group = filled(m + 1, torch.int64), filled(K, torch.int32), filled(K + 1, torch.int64), filled(K, torch.int32)
    status = torch.zeros(m + n + 1, dtype=torch.int32, device="cuda")
    tl, sp = np.array(w.lens[:m], np.int32), ia.as_chars(stop).astype(np.uint16)
    need_b = lib.fmx_values_of_hits_groups_scratch_bytes(m, K, max_len)
    ws_b = torch.empty(max(need_b, 1), dtype=torch.uint8, device="cuda")
    assert lib.fmx_values_of_hits_groups_dev(fm.handle, m, tl.ctypes.data, sp.ctypes.data if len(sp) else None, len(sp), max_len, first_off.data_ptr(),
                                             first_locs.data_ptr(), K, val_off.data_ptr(), lines.data_ptr(), text_off.data_ptr(), group.data_ptr(),
                                             status.data_ptr(), ws_b.data_ptr(), need_b, st) == 0, last_error()
    torch.cuda.synchronize()
    voff = cut(val_off, m + 1, "val_off").astype(np.int64).copy()
    G = int(voff[m])
    if base is not None:
        assert (voff == base.val_off).all() and (lines.cpu().numpy()[:G] == base.lines).all(), "stage b"
        F = int(base.first_off[m])
        assert (first_lines.cpu().numpy()[:F] == base.first_lines).all() and (group.cpu().numpy()[:F] == base.group_of_first).all(), "stages a, b"
    # the new stage over the numbers' part: hit_off + m, the slots [0, all_end + extra)
    B, P = 1 if edges is None else len(edges) - 1, len(permille)
    rows_of = np.minimum(np.diff(voff), top)
    R = int(rows_of.sum())
    cells = int(((rows_of[np.clip(np.asarray(by_of, np.int64), 0, m - 1)] + 1) * B).sum()) if n else 0
    sizes = dict(count=cells, sum_lo=cells, sum_hi=cells, min=cells, max=cells, pct=cells * P, no_key=n, not_number=n, overflow=n)
    out = {k: filled(sizes[k], torch.int32 if k in ("count", "no_key", "not_number", "overflow") else torch.int64) for k in CELL_NAMES}
    key_row_off, key_row_group, key_row_lines, cell_off = filled(m + 1, torch.int64), filled(R, torch.int32), filled(R, torch.int32), filled(n + 1, torch.int64)
    tl, bo, pm = np.array(w.lens[m:], np.int32), np.array(by_of, np.int32), np.array(permille, np.int32)
    e = None if edges is None else np.array(edges, np.int32)
    need_c = lib.fmx_numbers_by_key_buckets_scratch_bytes(n, m, G, b.slots, 0 if e is None else len(e), P)
    assert 0 < need_c < WS_LIMIT
    ws_c = torch.empty(need_c, dtype=torch.uint8, device="cuda")
    vcopy = voff.copy()
    rc = lib.fmx_numbers_by_key_buckets_dev(fm.handle, n, tl.ctypes.data, bo.ctypes.data, m, vcopy.ctypes.data, top, None if e is None else e.ctypes.data,
                                            0 if e is None else len(e), b.hit_off.data_ptr() + 8 * m, b.locs.data_ptr(), b.slots, first_off.data_ptr(),
                                            first_lines.data_ptr(), group.data_ptr(), lines.data_ptr(), frac_digits, pm.ctypes.data if P else None, P,
                                            key_row_off.data_ptr(), key_row_group.data_ptr(), key_row_lines.data_ptr(), cell_off.data_ptr(),
                                            *(out[k].data_ptr() for k in CELL_NAMES), status.data_ptr() + 4 * m, ws_c.data_ptr(), need_c - short, st)
    for a in (tl, bo, pm, vcopy) + (() if e is None else (e,)):
        a[:] = -9  # (the call has copied what it needs before it returns)
    torch.cuda.synchronize()
    if rc:
        assert all((t.cpu().numpy() == SENT).all() for t in list(out.values()) + [key_row_off, key_row_group, key_row_lines, cell_off])
        return rc, None
    got = dict(key_row_off=cut(key_row_off, m + 1, "key_row_off"), key_row_group=cut(key_row_group, R, "key_row_group"),
               key_row_lines=cut(key_row_lines, R, "key_row_lines"), cell_off=cut(cell_off, n + 1, "cell_off"), n_groups=np.diff(voff))
    for k in CELL_NAMES:
        a = cut(out[k], sizes[k], k)
        got[k] = a.view(np.uint64) if k.startswith("sum") else a
    assert (status.cpu().numpy() == 0).all()
    # the text of the key rows: the fill of ALL groups, the gather of the rows
    units = int(text_off.cpu().numpy()[G]) if G else 0
    chars = torch.full((units + PAD,), CHAR_SENT, dtype=torch.int16, device="cuda")
    assert lib.fmx_values_fill_dev(fm.handle, G, text_off.data_ptr(), chars.data_ptr(), ws_b.data_ptr(), need_b, st) == 0, last_error()
    row_text_off, row_chars = filled(R + 1, torch.int64), torch.full((units + PAD,), CHAR_SENT, dtype=torch.int16, device="cuda")
    need_g = lib.fmx_values_gather_rows_scratch_bytes(m, R)
    ws_g = torch.empty(max(need_g, 1), dtype=torch.uint8, device="cuda")
    assert lib.fmx_values_gather_rows_dev(fm.handle, m, voff.ctypes.data, top, units, key_row_group.data_ptr(), text_off.data_ptr(), chars.data_ptr(),
                                          row_text_off.data_ptr(), row_chars.data_ptr(), ws_g.data_ptr(), need_g, st) == 0, last_error()
    torch.cuda.synchronize()
    rto = cut(row_text_off, R + 1, "row_text_off")
    rc_all = row_chars.cpu().numpy()
    assert (rc_all[int(rto[R]):] == CHAR_SENT).all(), "stored beyond the answer: row_chars"
    text = rc_all[:int(rto[R])].view(np.uint16)
    got["row_text"] = [text[rto[r]:rto[r + 1]].tobytes().decode("utf-16-le", "surrogatepass") for r in range(R)]
    return 0, got


def host_by_hist(fm, w, m, by_of, stop, max_len, edges, top, permille=(500, 950), frac_digits=0):
    kch, koff = ia.pack_patterns(w.patterns[:m])
    nch, noff = ia.pack_patterns(w.patterns[m:])
    got = fm.number_stats_by_histogram_batch(kch, koff, nch, noff, by_of, *w.term_arrays(), w.query_off, w.kinds, w.where_of[:m], w.where_of[m:], stop,
                                             max_len, edges, top, permille, frac_digits)
    to, ch = got["text_off"], got["chars"]
    got["row_text"] = [ch[to[r]:to[r + 1]].tobytes().decode("utf-16-le", "surrogatepass") for r in range(len(to) - 1)]
    return got


def check_whole(got, want, w, m, what):
    check_by_hist(got, want, what)
    assert got["row_text"] == want.row_text and (np.asarray(got["n_groups"]) == want.n_groups).all(), what
    for i in range(want.n):  # invariant 1
        mine = got["count"][got["cell_off"][i]:got["cell_off"][i + 1]]
        assert mine.sum() + got["no_key"][i] + got["not_number"][i] + got["overflow"][i] == want.kept[i], what


def case(tag, fm, o, T, keys, numbers, by_of, stop, max_len, edges=None, top=10, queries=(), key_where=None, where=None, permille=(500, 950),
         frac_digits=0, device=True, host=True, lead=3, extra=70):
    """the judge (once per case), the host form and the device stage"""
    w, want = judged(tag, o, T, keys, numbers, by_of, stop, max_len, edges, top, queries, key_where, where, permille, frac_digits)
    m = len(keys)
    what = "%s %r by %r top %d edges %s" % (tag, numbers, keys, top, None if edges is None else len(edges))
    if host:
        got = host_by_hist(fm, w, m, by_of, stop, max_len, edges, top, permille, frac_digits)
        if w.kept[:m].sum() == 0:  # no key pattern has a kept hit: nothing beyond the filter runs, no key rows and no cells at all
            assert not got["key_row_off"].any() and not got["cell_off"].any() and len(got["count"]) == len(got["key_row_lines"]) == 0, what
            assert (got["no_key"] == want.kept).all() and not got["not_number"].any() and not got["overflow"].any() and not want.count.any(), what
        else:
            check_whole(got, want, w, m, what + ", host form")
        assert (got["kept"] == want.kept).all() and (got["key_kept"] == want.key_kept).all() and (got["occurrences"] == w.occurrences[m:]).all(), what
        assert (got["key_occurrences"] == w.occurrences[:m]).all() and (got["status"] == 0).all() and (got["key_status"] == 0).all(), what
        assert (got["term_status"] == w.term_status).all(), what
    if device and w.kept[:m].sum() > 0:
        rc, dev = dev_by_hist(fm, w, m, by_of, stop, max_len, edges, top, permille, frac_digits, lead, extra, base=want.base)
        assert rc == 0, last_error()
        check_whole(dev, want, w, m, what + ", device stage")
    return want


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


@pytest.fixture(scope="module")
def edge():
    text = edge_text()
    o = orc.OracleFmIndex(text, 8, True)
    fm = ia.FmIndex(text, 8, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == EDGE_LINES
    yield text, o, fm, T
    fm.close()


# ---- 1. the device stage over stages a and b (and the host form over the same cases) ----
def test_tops_at_and_around_the_groups(hd):
    """top below, at and above G_k = 356, and a top that cuts through a run of groups with equal lines"""
    o, fm, T = hd
    cut300 = case("hd16 byhist", fm, o, T, ["INFO "], ["size "], [0], " :", 32, EDGES_250, 300)
    assert len(cut300.key_row_lines) == 300 and cut300.key_row_lines[-1] == cut300.key_row_lines[-100] == 1
    for top in (1, 355, 356, 357, 65536):
        want = case("hd16 byhist", fm, o, T, ["INFO "], ["size "], [0], " :", 32, None, top)
        assert len(want.key_row_lines) == min(top, 356)


@pytest.mark.parametrize("edges", [None, EDGES_250, EDGES_UNEVEN, EDGES_EMPTY, EDGES_BEYOND], ids=["none", "250", "uneven", "empty", "beyond"])
def test_two_keys_three_numbers(hd, edges):
    """two key patterns with different G_k and three number patterns of which two share a key: the packed cell_off and the fold to
    each pattern's own R_k"""
    o, fm, T = hd
    want = case("hd16 byhist", fm, o, T, ["INFO ", " from /10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, edges, 5, permille=(0, 500, 1000))
    assert want.key_row_off.tolist()[1] == 5 and want.key_row_off[2] - 5 == min(5, int(want.n_groups[1])) < 5 < want.n_groups[0]
    B = want.B
    assert np.diff(want.cell_off).tolist() == [6 * B, 6 * B, (int(want.key_row_off[2]) - 5 + 1) * B]


def test_fractions_and_percentile_counts(hd):
    o, fm, T = hd
    case("hd16 byhist", fm, o, T, ["INFO "], ["src: /10."], [0], " :", 32, EDGES_250, 4, permille=tuple(range(0, 1000, 63)), frac_digits=3)
    case("hd16 byhist", fm, o, T, [" from /10.", "INFO "], ["blk_", "size "], [1, 0], " :.", 16, EDGES_250, 3, permille=())


def test_edge_text(edge):
    text, o, fm, T = edge
    thirds = np.array([0, 1000, 2000, 3000], np.int32)
    odd = np.array([5, 6, 6, 13, 150, 2101, 2999], np.int32)
    for edges, top in ((None, 3), (odd, 8)):
        want = case("edge byhist", fm, o, T, EDGE_KEYS, EDGE_NUMBERS, [0, 0, 0], " \n", 32, edges, top, permille=(0, 500, 950, 1000))
        assert_regex(want, 0, 0, text, "k=", "n=", " \n", 32, edges, top)
    want = case("edge byhist", fm, o, T, EDGE_KEYS, EDGE_NUMBERS, [3, 1, 2], " \n", 32, thirds, 4, permille=(500,), frac_digits=3)
    assert want.no_key[0] == want.kept[0] > EDGE_LINES and want.n_groups.tolist()[1:] == [EDGE_LINES, 1, 0]
    case("edge byhist", fm, o, T, ["k="], ["n="], [0], " \n", 32, thirds, 5, lead=0, extra=0)  # exactly the hits


# ---- 2. the host form and the convenience on the fixture's figures ----
def fixture_get(hd):
    o, fm, T = hd

    def get(number, key, stop, edges, top, where):
        q = dict(queries=[where], key_where=[0], where=[0]) if where else {}
        want = case("hd16 byhist", fm, o, T, [key], [number], [0], stop, 32, edges, top, **q)
        for kw in (dict(), dict(ignore_case=True)):  # (the fixture has one spelling of each: the class form gives the same answer)
            s = fm.number_stats_by_histogram(number, key, edges, top, stop, 32, where, **kw)
            rows = want.rows(0)
            assert [(r["value"], r["lines"], r["count"], r["sum"]) for r in s.rows] == [tuple(r) for r in rows[:-1]]
            assert [r["group"] for r in s.rows] == want.key_row_group.tolist()
            assert (s.other["count"], s.other["sum"]) == (rows[-1][2], rows[-1][3])
            c0 = int(want.cell_off[0])
            for r, row in enumerate(s.rows + [s.other]):
                a = c0 + r * want.B
                assert row["min"] == want.min[a:a + want.B].tolist() and row["max"] == want.max[a:a + want.B].tolist()
                assert row["pct"] == want.pct[a:a + want.B].tolist()
            assert (s.n_groups, s.no_key, s.not_number, s.overflow, s.kept) == (int(want.n_groups[0]), int(want.no_key[0]), int(want.not_number[0]),
                                                                                 int(want.overflow[0]), int(want.kept[0]))
        return want

    return get


def test_fixture_figures(hd):
    """the issue's figures through the host form (literal and class), the Python convenience and the device stage"""
    assert_fixture_figures(fixture_get(hd))


def test_degenerate_calls(hd, edge):
    """no kept key hit; no kept number hit; ignore_case= joins the spellings; an index without extraction; one without a line table"""
    o, fm, T = hd
    s = fm.number_stats_by_histogram("size ", "zzqq#", EDGES_250, 3)
    assert s.rows == [] and s.other["count"] == [0] * 8 and (s.no_key, s.kept, s.n_groups) == (608, 608, 0)
    out = fm.number_stats_by_histogram_batch(*ia.pack_patterns([ia.as_chars("zzqq#")]), *ia.pack_patterns([ia.as_chars("size ")]), [0], *ia.pack_patterns([]),
                                             [0], [], [-1], [-1], " ", 8, EDGES_250, 3)
    assert out["key_row_off"].tolist() == [0, 0] and out["cell_off"].tolist() == [0, 0] and len(out["count"]) == 0 and out["no_key"].tolist() == [608]
    empty = fm.number_stats_by_histogram("zzqq#", "INFO ", EDGES_250, 3, " :")
    assert [r["lines"] for r in empty.rows] == [525, 480, 283] and all(r["count"] == [0] * 8 and r["sum"] == [0] * 8 for r in empty.rows + [empty.other])
    assert empty.kept == 0 and empty.n_groups == 356
    text, eo, efm, eT = edge
    for kw in (dict(), dict(where=dict(all=["k=far"]))):  # neither pattern has a hit, without a query and with one
        s = efm.number_stats_by_histogram("zzqq%", "zzqq#", [0, 1000, 3000], 3, " \n", 32, **kw)
        assert s.rows == [] and s.other["count"] == [0, 0] and (s.no_key, s.not_number, s.overflow, s.kept, s.n_groups) == (0, 0, 0, 0, 0)
    q = [dict(all=["nokey"]), dict(all=["k=far"]), dict(all=["only"])]
    thirds = np.array([0, 1000, 2000, 3000], np.int32)
    none = case("edge byhist", efm, eo, eT, ["k="], ["n="], [0], " \n", 32, thirds, 5, queries=q, key_where=[0], where=[-1])
    assert none.n_groups[0] == 0 and none.no_key[0] == none.kept[0] > EDGE_LINES
    kept_none = case("edge byhist", efm, eo, eT, ["k="], ["n="], [0], " \n", 32, thirds, 5, queries=q, key_where=[-1], where=[2])
    assert kept_none.kept[0] == 0 and len(kept_none.key_row_lines) == 5
    mixed_text = "Status=200 Bytes=10 ok\nstatus=200 bytes=5 OK\nSTATUS=404 BYTES=7 ok\nstatus=404 none\nbytes=9 missing\nstatus=200 bytes=x Ok\n"
    mixed = ia.FmIndex(mixed_text, 4, True, device=0)
    bare = ia.FmIndex(HD[:4000], 16, True, device=0)
    plain = ia.FmIndex(edge_text()[:6000], 8, False, device=0)
    try:
        mixed.build_line_table("\n")
        s = mixed.number_stats_by_histogram("bytes=", "status=", [0, 3, 6], 1, ignore_case=True)  # the union of the spellings
        assert [(r["value"], r["lines"], r["count"], r["sum"]) for r in s.rows] == [("200", 3, [2, 0], [15, 0])]
        assert (s.other["count"], s.other["sum"], s.no_key, s.not_number, s.kept, s.n_groups) == ([1, 0], [7, 0], 1, 1, 5, 2)
        exact = mixed.number_stats_by_histogram("bytes=", "status=", [0, 3, 6], 1)
        assert [(r["value"], r["lines"], r["count"], r["sum"]) for r in exact.rows] == [("200", 2, [1, 0], [5, 0])] and exact.no_key == 1
        with pytest.raises(ia.FmxError) as err:
            bare.number_stats_by_histogram("size ", "INFO ", None, 3)
        assert err.value.code == E_ARG and "fmx_line_table_build" in str(err.value)
        plain.build_line_table("\n")
        sub = edge_text()[:6000]
        out = plain.number_stats_by_histogram_batch(*ia.pack_patterns([ia.as_chars("k=")]), *ia.pack_patterns([ia.as_chars("n="), ia.as_chars("m=")]),
                                                    [0, 0], *ia.pack_patterns([]), [0], [], [-1], [-1, -1], " \n", 32, None, 3)
        assert out["key_row_off"].tolist() == [0, 0] and out["cell_off"].tolist() == [0, 0, 0] and out["n_groups"].tolist() == [0]
        assert (out["status"] == ST_NOT_ENABLED).all() and (out["key_status"] == ST_NOT_ENABLED).all()
        assert out["kept"].tolist() == [sub.count("n="), sub.count("m=")] == out["occurrences"].tolist() and out["no_key"].tolist() == [0, 0]
        # neither the key pattern nor the number pattern has a hit: nothing runs, the statuses still say why there are no key rows
        out = plain.number_stats_by_histogram_batch(*ia.pack_patterns([ia.as_chars("zzqq#")]), *ia.pack_patterns([ia.as_chars("zzqq%")]), [0],
                                                    *ia.pack_patterns([]), [0], [], [-1], [-1], " \n", 32, None, 3)
        assert out["key_row_off"].tolist() == [0, 0] and out["cell_off"].tolist() == [0, 0] and out["n_groups"].tolist() == [0]
        assert (out["status"] == ST_NOT_ENABLED).all() and (out["key_status"] == ST_NOT_ENABLED).all()
        assert out["kept"].tolist() == [0] == out["occurrences"].tolist() and out["no_key"].tolist() == [0]
    finally:
        mixed.close()
        bare.close()
        plain.close()


# ---- 3. the five invariants against the existing calls on the same index ----
@pytest.mark.parametrize("edges", [None, EDGES_250, EDGES_EMPTY], ids=["none", "250", "empty"])
def test_invariants_against_the_existing_calls(hd, edges):
    o, fm, T = hd
    keys, numbers = ia.pack_patterns([ia.as_chars("INFO ")]), ia.pack_patterns([ia.as_chars("size "), ia.as_chars("blk_")])
    none = ia.pack_patterns([])
    for top in (400, 7):
        got = fm.number_stats_by_histogram_batch(*keys, *numbers, [0, 0], *none, [0], [], [-1], [-1, -1], " :", 32, edges, top, (0, 500, 950))
        by = fm.number_stats_by_batch(*keys, *numbers, [0, 0], *none, [0], [], [-1], [-1, -1], " :", 32, None if edges is None else span(edges), (0, 500, 950))
        B, G = got["buckets"], int(by["val_off"][1])
        R = min(top, G)
        assert got["n_groups"].tolist() == [G] and got["key_row_off"].tolist() == [0, R] and got["cell_off"].tolist() == [0, (R + 1) * B, 2 * (R + 1) * B]
        order = sorted(range(G), key=lambda g: -int(by["lines"][g]))[:R]
        assert got["key_row_group"].tolist() == order and got["key_row_lines"].tolist() == sorted(by["lines"].tolist(), reverse=True)[:R]  # invariant 5
        if edges is not None:
            hist = fm.hit_histogram_where_batch(*numbers, *none, [0], [], [-1, -1], edges)
        for i in range(2):
            c0, r0 = int(got["cell_off"][i]), int(by["row_off"][i])
            cnt = got["count"][c0:c0 + (R + 1) * B].reshape(R + 1, B)
            tails = int(got["no_key"][i]) + int(got["not_number"][i]) + int(got["overflow"][i])
            assert cnt.sum() + tails == got["kept"][i] == by["kept"][i]  # invariant 1
            assert (got["no_key"][i], got["not_number"][i], got["overflow"][i]) == (by["no_key"][i], by["not_number"][i], by["overflow"][i])
            sums = [(int(h) << 64) | int(lo) for lo, h in zip(got["sum_lo"][c0:c0 + (R + 1) * B], got["sum_hi"][c0:c0 + (R + 1) * B])]
            for r, g in enumerate(order):  # invariants 2 and 3: a row's cells over b are number_stats_by's row
                cs = range(r * B, (r + 1) * B)
                assert cnt[r].sum() == by["count"][r0 + g] and sum(sums[c] for c in cs) == (int(by["sum_hi"][r0 + g]) << 64) | int(by["sum_lo"][r0 + g])
                full = [c for c in cs if cnt[r][c - r * B]]
                assert min((int(got["min"][c0 + c]) for c in full), default=0) == by["min"][r0 + g]
                assert max((int(got["max"][c0 + c]) for c in full), default=0) == by["max"][r0 + g]
                if B == 1:
                    assert (got["pct"][c0 + r] == by["pct"][r0 + g]).all()
            if top >= G:
                assert cnt[R].sum() == 0 and not any(sums[R * B:])  # "other" is zero
            else:
                assert cnt[R].sum() == by["count"][r0:r0 + G].sum() - cnt[:R].sum() > 0
            if edges is not None:  # invariant 4: what a bucket's cells lack of the hits histogram are its hits without a cell
                assert (cnt.sum(axis=0) <= hist[i]).all() and int((hist[i] - cnt.sum(axis=0)).sum()) == tails


# ---- 4. refusals ----
def test_refusals(hd):
    """each returns before a launch and leaves every output untouched (dev_by_hist asserts the sentinels)"""
    o, fm, T = hd
    w = Where("hd16 byhist", o, T, ["INFO ", "size "], [], [-1, -1], span(EDGES_250))
    for kw, word in ((dict(short=1), "fmx_numbers_by_key_buckets_scratch_bytes"), (dict(top=0), "top"), (dict(top=65537), "top"),
                     (dict(edges=[0]), "edge"), (dict(edges=[5, 4]), "edge"), (dict(edges=[-1, 4]), "edge"), (dict(frac_digits=10), "frac_digits"),
                     (dict(permille=(1001,)), "permille"), (dict(by_of=[1]), "by_of"),
                     (dict(top=65536, edges=np.arange(2050, dtype=np.int32)), "2^27 cells"),  # 65,537 * 2,049 cells: one above the bound's reach
                     (dict(top=65535, edges=np.arange(1026, dtype=np.int32), permille=(1, 2)), "2^27 percentiles")):
        args = dict(edges=EDGES_250, top=3, permille=(500,), frac_digits=0, by_of=[0], short=0)
        args.update(kw)
        rc, got = run_refused(fm, w, args)
        assert rc == E_ARG and got is None and word in last_error(), (kw, rc, last_error())
    keys, numbers, none = ia.pack_patterns([ia.as_chars("INFO ")]), ia.pack_patterns([ia.as_chars("size ")]), ia.pack_patterns([])

    def call(index=fm, by_of=(0,), stop=" :", max_len=8, permille=(500,), frac_digits=0, keys=keys, edges=EDGES_250, top=3):
        try:
            index.number_stats_by_histogram_batch(*keys, *numbers, by_of, *none, [0], [], [-1] * (len(keys[1]) - 1), [-1], stop, max_len, edges, top,
                                                  permille, frac_digits)
        except ia.FmxError as e:
            return e.code, str(e)
        return 0, ""

    assert call()[0] == 0
    for kw, word in ((dict(by_of=(1,)), "by_of[0]"), (dict(keys=none), "m == 0"), (dict(max_len=0), "max_len"), (dict(max_len=65), "max_len"),
                     (dict(stop="x" * 65), "stop set"), (dict(frac_digits=10), "frac_digits"), (dict(permille=(1001,)), "permille"),
                     (dict(permille=tuple(range(17))), "n_permille"), (dict(top=0), "top"), (dict(top=65537), "top"), (dict(edges=[4]), "edge"),
                     (dict(edges=[4, 3]), "edge"), (dict(edges=[-2, 3]), "edge"), (dict(edges=np.arange(2 ** 27 // 4 + 2, dtype=np.int32)), "2^27 cells"),
                     (dict(edges=np.arange(2 ** 27 // 8 + 1, dtype=np.int32), permille=(1, 2, 3)), "2^27 percentiles")):
        code, msg = call(**kw)
        assert code == E_ARG and word in msg, (kw, code, msg)
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    try:
        sa.construct()
        assert call(index=host_only)[0] == E_NO_DEVICE
        torch = _torch()
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        p, one, voff = t.data_ptr(), np.zeros(4, np.int32), np.array([0, 1], np.int64)
        for h, code in ((host_only.handle, E_NO_DEVICE), (sa._h, E_ARG)):
            assert ia.lib.fmx_numbers_by_key_buckets_dev(h, 1, one.ctypes.data, one.ctypes.data, 1, voff.ctypes.data, 3, None, 0, p, p, 4, p, p, p, p, 0, None, 0,
                                                         *([p] * 14), p, 1 << 20, stream()) == code
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0).all()
    finally:
        host_only.close()


def run_refused(fm, w, args):
    """dev_by_hist for a call the stage refuses; where the refused shape has no scratch size, the workspace is the good shape's"""
    lib = ia.lib
    good = lib.fmx_numbers_by_key_buckets_scratch_bytes

    class Sized:
        """(ctypes function objects take no attributes of ours: a stand-in with the one call dev_by_hist makes)"""

        def __getattr__(self, name):
            if name == "fmx_numbers_by_key_buckets_scratch_bytes":
                return lambda n, m, G, H, ne, P: good(n, m, G, H, len(EDGES_250), 1)
            return getattr(lib, name)

    ia.lib = Sized()
    try:
        return dev_by_hist(fm, w, 1, args["by_of"], " :", 8, args["edges"], args["top"], args["permille"], args["frac_digits"], short=args["short"])
    finally:
        ia.lib = lib


# ---- 5. loops ----
def test_code_and_cell_kernels_loop(hd):
    """the fixture's batch repeated until k_bh_codes and k_bh_cells each make at least two passes over fmx_hit_lines_geometry's grids;
    the judge is the one-repetition judge, tiled"""
    o, fm, T = hd
    keys, numbers, by_of, stop, max_len, permille, top, edges = ["INFO ", " from /10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, (0, 500, 1000), 356, EDGES_250
    m, nb, P, B = len(keys), len(numbers), len(permille), len(edges) - 1
    w, want = judged("hd16 byhist", o, T, keys, numbers, by_of, stop, max_len, edges, top, (), None, None, permille, 0)
    key_hits = int(w.kept_off[m])
    per, cells_per = int(w.kept_off[-1]) - key_hits, int(want.cell_off[-1])
    KEY, FLAT = geometry(fm, 10 ** 9)[0] * TILE, geometry(fm, 10 ** 9)[1] * LANES
    reps = max(KEY // per, FLAT // cells_per) + 2
    slots, cells = 3 + key_hits + reps * per + 70, reps * cells_per
    code_passes = -(-slots // (geometry(fm, slots)[0] * TILE))
    cell_passes = -(-cells // (geometry(fm, cells)[1] * LANES))
    print("by histogram: passes k_bh_codes %d, k_bh_cells %d (%d repetitions, %d slots, %d cells)" % (code_passes, cell_passes, reps, slots, cells))
    assert code_passes >= 2 and cell_passes >= 2

    class Tiled:
        n = m + nb * reps
        kept_off = np.concatenate([w.kept_off[:m + 1], key_hits + np.cumsum(np.tile(w.kept[m:], reps))]).astype(np.int64)
        kept_locs = np.concatenate([w.kept_locs[:key_hits], np.tile(w.kept_locs[key_hits:], reps)]).astype(np.int32)
        lens = np.concatenate([w.lens[:m], np.tile(w.lens[m:], reps)]).astype(np.int32)

    rc, got = dev_by_hist(fm, Tiled, m, by_of * reps, stop, max_len, edges, top, permille, 0, base=want.base)
    assert rc == 0, last_error()

    class Cells:
        n, P = nb * reps, len(permille)
        key_row_off, key_row_group, key_row_lines = want.key_row_off, want.key_row_group, want.key_row_lines
        cell_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(want.cell_off), reps))]).astype(np.int64)
        count, min, max = np.tile(want.count, reps), np.tile(want.min, reps), np.tile(want.max, reps)
        pct = np.tile(want.pct, (reps, 1))
        sums = want.sums * reps
        no_key, not_number, overflow = np.tile(want.no_key, reps), np.tile(want.not_number, reps), np.tile(want.overflow, reps)

    assert want.count.sum() > 0 and max(want.sums) > 2 ** 64
    check_by_hist(got, Cells, "%d repetitions of %d number hits" % (reps, per))
    assert got["row_text"] == want.row_text


# ---- 6. geometry ----
def test_geometry(hd, edge):
    """1,024-lane workgroups and one workgroup per CU: the same answers"""
    o, fm, T = hd
    text, eo, efm, eT = edge
    for kw in (dict(block=1024), dict(groups_per_cu=1), dict(block=1024, groups_per_cu=1)):
        with options(**kw):
            case("hd16 byhist", fm, o, T, ["INFO ", " from /10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, EDGES_UNEVEN, 5, permille=(0, 500, 1000))
            case("edge byhist", efm, eo, eT, EDGE_KEYS, EDGE_NUMBERS, [0, 0, 0], " \n", 32, None, 3, permille=(0, 500, 950, 1000))

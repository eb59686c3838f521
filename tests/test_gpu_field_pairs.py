"""Statistics and line counts by the values of two fields of the same line, on the GPU: the join stage
(fmx_pairs_of_first_hits_dev: fmx_hit_pairs.hip), stage c (fmx_numbers_by_key_dev, unchanged) over its joined lists, the host forms
fmx_number_stats_by_pair_batch / _class_batch and the Python conveniences FmIndex.number_stats_by_pair / field_value_pairs.

The judge is judge_pairs (tests/test_field_pairs_cpu.py), computed once per case and shared; on the edge text the regular
expressions of that file judge the judge there.  The join runs over the judge's first-hit lists, uploaded with entries in front of
first_off[0] and n_slots larger than the real slots; every output is prefilled with a sentinel and padded by 64 entries, and what
lies behind the answer must keep it.  Options are set inside the tests and put back in `finally`.  Every refused call returns before
a launch."""
import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_pairs_cpu import (EDGE_PAIRS, FIX_KEYS, FIX_MAX_LEN, FIX_STOP, JOIN_NAMES, PAIR_KEYS, assert_pair_figures, check_join, check_pairs, edge_case,
                                  fixture_case, np_join)
from test_field_values_where_cpu import EVERY_LINE
from test_gpu_field_values import ST_NOT_ENABLED, last_error
from test_gpu_locate_rows import _torch, options
from test_gpu_number_stats_by import ROW_NAMES, Block, cut, filled, stream
from test_gpu_stage_loops import assert_loops, caps, check_whole, flat_passes, up
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_stats_by_cpu import EDGE_LINES, edge_text

pytestmark = pytest.mark.gpu

HD = hdfs_text()
E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE


def dev_join(fm, first_off, first_lines, group_of_first, val_off, pairs, lead=3, extra=70, short=0):
    """the join stage over first-hit lists with `lead` entries in front of first_off[0] and n_slots = the real slots + extra; a
    workspace `short` bytes too small.  rc and None where it refuses (every output untouched), else 0 and a dict under the judge's
    names"""
    torch = _torch()
    lib, m, c = ia.lib, len(first_off) - 1, len(pairs)
    fo = up(np.asarray(first_off, np.int64) + lead, np.int64)
    fl = up(np.concatenate([np.full(lead, -5, np.int32), np.asarray(first_lines, np.int32), np.zeros(1, np.int32)]), np.int32)
    fg = up(np.concatenate([np.full(lead, -5, np.int32), np.asarray(group_of_first, np.int32), np.zeros(1, np.int32)]), np.int32)
    n_slots = int(sum(first_off[a + 1] - first_off[a] for a, _ in pairs if 0 <= a < m)) + extra
    voff, pa, pb = np.array(val_off, np.int64), np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    room = max(n_slots, 1)
    out = dict(pair_off=filled(c + 1, torch.int64), pair_group_a=filled(room, torch.int32), pair_group_b=filled(room, torch.int32),
               pair_lines=filled(room, torch.int32), joined_off=filled(c + 1, torch.int64), joined_lines=filled(room, torch.int32),
               joined_group=filled(room, torch.int32))
    need = lib.fmx_pairs_of_first_hits_scratch_bytes(m, c, n_slots)
    ws = torch.empty(max(need - short, 1), dtype=torch.uint8, device="cuda")
    rc = lib.fmx_pairs_of_first_hits_dev(fm.handle, m, voff.ctypes.data, c, pa.ctypes.data, pb.ctypes.data, fo.data_ptr(), fl.data_ptr(), fg.data_ptr(), n_slots,
                                         *(out[k].data_ptr() for k in JOIN_NAMES), ws.data_ptr(), need - short, stream())
    for a in (voff, pa, pb):  # (the call has copied what it needs before it returns)
        a[:] = -9
    torch.cuda.synchronize()
    if rc:
        assert all((t.cpu().numpy() == SENT).all() for t in out.values()), "a refused call stored something"
        return rc, None
    got = dict(pair_off=cut(out["pair_off"], c + 1, "pair_off"), joined_off=cut(out["joined_off"], c + 1, "joined_off"))
    R, J = int(got["pair_off"][c]), int(got["joined_off"][c])
    assert 0 <= R <= n_slots and 0 <= J <= n_slots
    for name, count in (("pair_group_a", R), ("pair_group_b", R), ("pair_lines", R), ("joined_lines", J), ("joined_group", J)):
        a = out[name].cpu().numpy()
        assert (a[count:] == SENT).all(), "stored beyond the answer: " + name
        got[name] = a[:count]
    got["device"] = out  # (stage c reads the joined lists where they lie)
    return 0, got


def dev_rows(fm, w, m, got, by_of, permille, frac_digits, lead=3, extra=70):
    """stage c, unchanged, over the joined lists of dev_join and the judge's kept number hits: the pairs are its key patterns"""
    torch = _torch()
    lib, n, c = ia.lib, w.n - m, len(got["pair_off"]) - 1
    b = Block(w, lead, extra)
    poff = got["pair_off"].astype(np.int64).copy()
    R, P = int(np.diff(poff)[np.asarray(by_of, np.int64)].sum()) if n else 0, len(permille)
    sizes = dict(count=R, sum_lo=R, sum_hi=R, min=R, max=R, pct=R * P, no_key=n, not_number=n, overflow=n)
    out = {k: filled(sizes[k], torch.int32 if k in ("count", "no_key", "not_number", "overflow") else torch.int64) for k in ROW_NAMES}
    row_off = filled(n + 1, torch.int64)
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    tl, bo, pm = np.array(w.lens[m:], np.int32), np.array(by_of, np.int32), np.array(permille, np.int32)
    need = lib.fmx_numbers_by_key_scratch_bytes(n, b.slots, P)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    d = got["device"]
    rc = lib.fmx_numbers_by_key_dev(fm.handle, n, tl.ctypes.data, bo.ctypes.data, c, poff.ctypes.data, b.hit_off.data_ptr() + 8 * m, b.locs.data_ptr(), b.slots,
                                    d["joined_off"].data_ptr(), d["joined_lines"].data_ptr(), d["joined_group"].data_ptr(), frac_digits,
                                    pm.ctypes.data if P else None, P, row_off.data_ptr(), *(out[k].data_ptr() for k in ROW_NAMES), status.data_ptr(),
                                    ws.data_ptr(), need, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    rows = dict(row_off=cut(row_off, n + 1, "row_off"))
    for k in ROW_NAMES:
        a = cut(out[k], sizes[k], k)
        rows[k] = a.view(np.uint64) if k.startswith("sum") else a
    assert (status.cpu().numpy() == 0).all()
    return rows


def check_rows(rows, want, what):
    for name in ("row_off", "count", "min", "max", "no_key", "not_number", "overflow"):
        g, e = np.asarray(rows[name]), np.asarray(getattr(want, name))
        assert g.shape == e.shape and (g == e).all(), "%s: %s %r, expected %r" % (what, name, g[:8], e[:8])
    sums = [(int(hi) << 64) | int(lo) for lo, hi in zip(rows["sum_lo"], rows["sum_hi"])]
    assert sums == want.sums and (np.asarray(rows["pct"]).reshape(len(want.count), want.P) == want.pct).all(), what


def host_pairs(fm, w, m, pairs, by_of, stop, max_len, permille=(500, 950), frac_digits=0):
    kch, koff = ia.pack_patterns(w.patterns[:m])
    nch, noff = ia.pack_patterns(w.patterns[m:])
    return fm.number_stats_by_pair_batch(kch, koff, nch, noff, by_of, [p[0] for p in pairs], [p[1] for p in pairs], *w.term_arrays(), w.query_off, w.kinds,
                                         w.where_of[:m], w.where_of[m:], stop, max_len, None if w.window == EVERY_LINE else w.window, permille, frac_digits)


def check_host(got, w, want, what):
    m = want.m
    check_pairs(got, want, what)
    assert (got["kept"] == want.kept).all() and (got["key_kept"] == want.key_kept).all() and (got["occurrences"] == w.occurrences[m:]).all(), what
    assert (got["key_occurrences"] == w.occurrences[:m]).all() and (got["status"] == 0).all() and (got["key_status"] == 0).all(), what
    assert (got["term_status"] == w.term_status).all(), what
    for i in range(want.n):  # the invariant
        rows = got["count"][got["row_off"][i]:got["row_off"][i + 1]]
        assert rows.sum() + got["no_key"][i] + got["not_number"][i] + got["overflow"][i] == got["kept"][i], what
    for j in range(want.c):  # Σ pair_lines of pair j = the lines with both keys
        assert got["pair_lines"][got["pair_off"][j]:got["pair_off"][j + 1]].sum() == want.joined_off[j + 1] - want.joined_off[j], what


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


@pytest.fixture(scope="module")
def edge_want(edge):
    """the edge call of tests/test_field_pairs_cpu.py, judged once"""
    text, o, fm, T = edge
    return edge_case(o, T)


# ---- 1. the stage over the judge's arrays ----
def test_join_stage_over_the_judges_lists(edge, edge_want):
    """one call with every pair of EDGE_PAIRS: b has one group; as many pairs as lines; a == b; b without a hit (an empty entry between
    two that are not); an empty a; lines with a and not b and the reverse.  n_slots larger than the real slots, entries in front of
    first_off[0]; then exactly the slots"""
    text, o, fm, T = edge
    w, want = edge_want
    base = want.base
    for lead, extra in ((3, 70), (0, 0), (1025, 1023)):
        rc, got = dev_join(fm, base.first_off, base.first_lines, base.group_of_first, base.val_off, EDGE_PAIRS, lead, extra)
        assert rc == 0, last_error()
        check_join(got, want, "edge lists, %d in front, %d slots more" % (lead, extra))
    assert want.pair_off[3] == want.pair_off[5] < want.pair_off[6] and want.pair_off[2] - want.pair_off[1] > EDGE_LINES - 10
    # no pair at all and no slot at all
    rc, got = dev_join(fm, base.first_off, base.first_lines, base.group_of_first, base.val_off, [(0, 3), (3, 3)], extra=5)
    assert rc == 0 and got["pair_off"].tolist() == [0, 0, 0] and got["joined_off"].tolist() == [0, 0, 0]
    rc, got = dev_join(fm, base.first_off, base.first_lines, base.group_of_first, base.val_off, [(3, 0)], extra=0)
    assert rc == 0 and got["pair_off"].tolist() == [0, 0] and got["joined_off"].tolist() == [0, 0]


def test_join_stage_refusals(edge, edge_want):
    """each returns before a launch and leaves every output untouched (dev_join asserts the sentinels)"""
    text, o, fm, T = edge
    w, want = edge_want
    base = want.base
    lists = (base.first_off, base.first_lines, base.group_of_first)
    rc, _ = dev_join(fm, *lists, base.val_off, EDGE_PAIRS, short=1)
    assert rc == E_ARG and "fmx_pairs_of_first_hits_scratch_bytes" in last_error()
    for pairs, word in (([(0, 5)], "pair_a or pair_b"), ([(-1, 0)], "pair_a or pair_b")):
        rc, _ = dev_join(fm, *lists, base.val_off, [(0, 0)] + pairs)
        assert rc == E_ARG and word in last_error(), (pairs, last_error())
    down = base.val_off.copy()
    down[2] = down[1] - 1
    rc, _ = dev_join(fm, *lists, down, EDGE_PAIRS)
    assert rc == E_ARG and "val_off" in last_error()
    wide = np.array([0, 2 ** 31 - 1, 2 ** 32 - 2, 2 ** 32 - 2, 2 ** 32 - 2, 2 ** 32 - 2], np.int64)  # 31 + 31 bits of groups: c <= 3
    rc, _ = dev_join(fm, *lists, wide, [(0, 1)] * 4)
    assert rc == E_ARG and "64 bits" in last_error()
    torch = _torch()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, voff, one = t.data_ptr(), np.array([0, 1, 2], np.int64), np.zeros(1, np.int32)
    assert ia.lib.fmx_pairs_of_first_hits_dev(fm.handle, 2, voff.ctypes.data, 1, one.ctypes.data, one.ctypes.data, p, p, p, 2 ** 31, p, p, p, p, p, p, p, p,
                                              1 << 40, stream()) == E_ARG and "2^31 - 1 slots" in last_error()
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    try:
        sa.construct()
        for h, code in ((host_only.handle, E_NO_DEVICE), (sa._h, E_ARG)):
            assert ia.lib.fmx_pairs_of_first_hits_dev(h, 2, voff.ctypes.data, 1, one.ctypes.data, one.ctypes.data, p, p, p, 4, p, p, p, p, p, p, p, p, 1 << 20,
                                                      stream()) == code
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0).all()
    finally:
        host_only.close()


# ---- 2. stage c over the joined lists ----
def test_stage_c_over_the_joined_lists(edge, edge_want):
    """fmx_numbers_by_key_dev, unchanged, with m := c and val_off := pair_off: rows, no_key, 128-bit sums and percentiles against
    judge_pairs; numbers n= by (k=, c=), zzq# (no hit) by (k=, id=), m= by (k=, m=)"""
    text, o, fm, T = edge
    w, want = edge_want
    base = want.base
    rc, got = dev_join(fm, base.first_off, base.first_lines, base.group_of_first, base.val_off, EDGE_PAIRS)
    assert rc == 0, last_error()
    rows = dev_rows(fm, w, len(PAIR_KEYS), got, want.by_of, (0, 500, 950, 1000), 0)
    check_rows(rows, want, "stage c over the joined lists")
    assert max(want.sums) > 2 ** 63 and want.no_key[0] == 4 and want.kept[1] == 0 and want.row_off[2] - want.row_off[1] > EDGE_LINES - 10
    # a by_of that sends every number pattern to a pair without pairs: every kept hit is no_key
    w2, none = edge_case(o, T, by_of=(3, 4, 3))
    rows = dev_rows(fm, w2, len(PAIR_KEYS), got, none.by_of, (0, 500, 950, 1000), 0)
    check_rows(rows, none, "pairs without pairs")
    assert (none.no_key == none.kept).all() and none.row_off[-1] == 0


# ---- 3. the host forms, whole call ----
def test_fixture_figures(hd):
    """the issue's figures through the host form and the Python conveniences, each against the judge"""
    o, fm, T = hd

    def get(number, where, window):
        w, want = fixture_case(o, T, number, where, window)
        got = host_pairs(fm, w, 2, [(0, 1)], [0] * want.n, FIX_STOP, FIX_MAX_LEN)
        check_host(got, w, want, "hd16 pairs %r %r %r" % (number, where, window))
        table = {(a, b): c for a, b, c in fm.field_value_pairs(*FIX_KEYS, FIX_STOP, FIX_MAX_LEN, where, window)}
        assert table == want.table()
        rows, info = {}, dict(no_key=0, not_number=0, kept=0, key_lines=(int(got["lines"][:got["val_off"][1]].sum()), int(got["lines"][got["val_off"][1]:].sum())))
        if number:
            s = fm.number_stats_by_pair(number, *FIX_KEYS, FIX_STOP, FIX_MAX_LEN, where, window)
            assert [(g["values"], g["lines"]) for g in s.groups] == want.values() and [g["pct"] for g in s.groups] == want.pct.tolist()
            rows = {g["values"]: (g["count"], g["sum"], g["min"], g["max"]) for g in s.groups}
            assert rows == want.rows()
            info.update(no_key=s.no_key, not_number=s.not_number, kept=s.kept)
        return table, rows, info

    assert_pair_figures(get)
    top = fm.field_value_pairs(*FIX_KEYS, FIX_STOP, FIX_MAX_LEN, top=3)
    assert top == [("10", "DataNode", 354), ("11", "DataNode", 344), ("11", "FSNamesystem", 251)]
    s = fm.number_stats_by_pair("size ", *FIX_KEYS, FIX_STOP, FIX_MAX_LEN, top=2)
    assert [(g["values"], g["lines"], g["count"]) for g in s.groups] == [(("10", "DataNode"), 354, 75), (("11", "DataNode"), 344, 87)]
    assert abs(s.groups[0]["mean"] - 4_724_082_131 / 75) < 1e-6
    assert fm.field_value_pairs("0811", "zzqq#") == [] and fm.field_value_pairs("zzqq#", "0811") == []
    none = fm.number_stats_by_pair("size ", "0811", "zzqq#")
    assert none.groups == [] and none.no_key == 608 == none.kept
    empty = fm.number_stats_by_pair("zzqq#", *FIX_KEYS, FIX_STOP, FIX_MAX_LEN)
    assert len(empty.groups) == 11 and all(g["count"] == 0 and np.isnan(g["mean"]) for g in empty.groups) and empty.kept == 0


def test_edge_text_host_form(edge, edge_want):
    """the edge call, whole; the pivot alone (n == 0); a filter that keeps no key hit of one side; one that keeps nothing; a window"""
    text, o, fm, T = edge
    w, want = edge_want
    nk = len(PAIR_KEYS)
    check_host(host_pairs(fm, w, nk, EDGE_PAIRS, want.by_of, " \n", 32, (0, 500, 950, 1000)), w, want, "edge, host form")
    w0, pivot = edge_case(o, T, by_of=(), numbers=())
    got = host_pairs(fm, w0, nk, EDGE_PAIRS, [], " \n", 32, (0, 500, 950, 1000))
    check_host(got, w0, pivot, "edge, n == 0")
    assert len(got["row_off"]) == 1 and len(got["count"]) == 0 and got["pair_off"][-1] == want.pair_off[-1]
    q = [dict(all=["nokey"]), dict(all=["k=far"]), dict(all=["zzqq%"])]
    for what, kw in (("no kept hit of one side", dict(where_of=[-1, -1, -1, -1, 0] + [-1] * 3)), ("nothing kept", dict(where_of=[2] * (nk + 3))),
                     ("keys on two lines", dict(where_of=[1] * nk + [-1] * 3)), ("no kept number hit", dict(where_of=[-1] * nk + [2] * 3))):
        wf, wantf = edge_case(o, T, queries=q, **kw)
        check_host(host_pairs(fm, wf, nk, EDGE_PAIRS, wantf.by_of, " \n", 32, (0, 500, 950, 1000)), wf, wantf, "edge, " + what)
    wc, cut2 = edge_case(o, T, window=(150, 2101), frac_digits=3, max_len=1)
    check_host(host_pairs(fm, wc, nk, EDGE_PAIRS, cut2.by_of, " \n", 1, (0, 500, 950, 1000), 3), wc, cut2, "edge, window")
    # no key pattern at all: nothing is searched
    out = fm.number_stats_by_pair_batch(*ia.pack_patterns([]), *ia.pack_patterns([]), [], [], [], *ia.pack_patterns([ia.as_chars("zz")]), [0, 1], [0], [], [], " ", 8)
    assert out["val_off"].tolist() == [0] and out["pair_off"].tolist() == [0] and out["row_off"].tolist() == [0] and out["term_status"].tolist() == [0]


def test_pair_of_one_key_is_stats_by(hd):
    """the (k, k) call equals number_stats_by_batch array for array; so does (a, b) when b has one group and a key on every line that
    has one of a: "08" opens every line of the fixture and, with "1" in the stop set, its value is the empty string everywhere"""
    o, fm, T = hd
    keys, numbers, none = ia.pack_patterns([ia.as_chars("INFO "), ia.as_chars("08")]), ia.pack_patterns([ia.as_chars("size "), ia.as_chars("blk_")]), ia.pack_patterns([])
    tail = (*none, [0], [], [-1, -1], [-1, -1], " :1", 32, None, (0, 500, 1000))
    one = fm.number_stats_by_batch(*keys, *numbers, [0, 0], *tail)
    G = int(one["val_off"][1])
    assert G > 10 and one["val_off"][2] - G == 1 and one["lines"][G] == 2000 and one["count"].sum() > 300
    for pair in ((0, 0), (0, 1)):
        two = fm.number_stats_by_pair_batch(*keys, *numbers, [0, 0], [pair[0]], [pair[1]], *tail)
        for name in ("val_off", "lines", "text_off", "chars", "row_off", "count", "sum_lo", "sum_hi", "min", "max", "pct", "no_key", "not_number", "overflow", "kept",
                     "key_kept", "occurrences", "key_occurrences", "status", "key_status"):
            assert one[name].shape == two[name].shape and (one[name] == two[name]).all(), (pair, name)
        assert (two["pair_group_a"] == np.arange(G)).all() and (two["pair_lines"] == one["lines"][:G]).all()
        assert (two["pair_group_b"] == (np.arange(G) if pair == (0, 0) else 0)).all()


def test_class_form_and_ignore_case(hd):
    """class patterns of one spelling give the literal form's answer on the fixture; on a text of mixed case ignore_case= joins the
    spellings of both key patterns, the number pattern and the filter term (figures read off the text)"""
    o, fm, T = hd
    w, want = fixture_case(o, T, "size ", dict(all=["blk_"], none=["PacketResponder"]), None)
    single = lambda ps: ia.pack_class_patterns([list(p) for p in ps])  # noqa: E731
    got = fm.number_stats_by_pair_class_batch(*single(FIX_KEYS), *single(["size "]), [0], [0], [1], *single(["blk_", "PacketResponder"]), [0, 2], [0, 2], [0, 0], [0],
                                              FIX_STOP, FIX_MAX_LEN)
    check_pairs(got, want, "class patterns of one spelling, filtered")
    assert (got["kept"] == want.kept).all() and (got["key_kept"] == want.key_kept).all() and (got["status"] == 0).all()
    with pytest.raises(ia.FmxError) as err:
        fm.number_stats_by_pair_class_batch(*single(FIX_KEYS), *single(["size "]), [0], [0], [1], *single([]), [0], [], [-1, -1], [-1], " :", 32, max_ranges=0)
    assert err.value.code == E_ARG
    with pytest.raises(ia.FmxError) as err:
        fm.number_stats_by_pair_class_batch(*single(FIX_KEYS), *single(["size "]), [0], [0], [2], *single([]), [0], [], [-1, -1], [-1], " :", 32)
    assert err.value.code == E_ARG and "pair_a or pair_b" in str(err.value)
    text = ("Host=a Status=200 Bytes=10 ok\nhost=a status=200 bytes=5 OK\nHOST=b STATUS=404 BYTES=7 ok\nhost=b status=404 none\nstatus=200 bytes=9 nohost\n"
            "host=a status=404 bytes=x Ok\nhost=c bytes=3 nostatus\n")
    mixed = ia.FmIndex(text, 4, True, device=0)
    try:
        mixed.build_line_table("\n")
        s = mixed.number_stats_by_pair("bytes=", "host=", "status=", ignore_case=True)
        assert [(g["values"], g["lines"], g["count"], g["sum"], g["min"], g["max"]) for g in s.groups] == [
            (("a", "200"), 2, 2, 15, 5, 10), (("a", "404"), 1, 0, 0, 0, 0), (("b", "404"), 2, 1, 7, 7, 7)]
        assert (s.no_key, s.not_number, s.kept, s.key_kept) == (2, 1, 6, (6, 6))
        assert mixed.field_value_pairs("host=", "status=", ignore_case=True) == [("a", "200", 2), ("a", "404", 1), ("b", "404", 2)]
        assert mixed.field_value_pairs("host=", "status=") == [("a", "200", 1), ("a", "404", 1), ("b", "404", 1)]
        assert mixed.field_value_pairs("host=", "status=", where=dict(all=["OK"]), ignore_case=True, top=1) == [("a", "200", 2)]
        assert mixed.field_value_pairs("status=", "host=", lines=(1, 4), ignore_case=True) == [("200", "a", 1), ("404", "b", 2)]
    finally:
        mixed.close()


def test_refusals_and_indexes_without(hd):
    """an index without a line table is refused; one without extraction answers FMX_ST_NOT_ENABLED; a handle that is not resident;
    the refusals of the host arrays on a resident handle"""
    o, fm, T = hd
    keys, numbers, none = ia.pack_patterns([ia.as_chars(k) for k in FIX_KEYS]), ia.pack_patterns([ia.as_chars("size ")]), ia.pack_patterns([])

    def call(index=fm, by_of=(0,), pair_a=(0,), pair_b=(1,), max_len=8, permille=(500,), numbers=numbers):
        try:
            return 0, index.number_stats_by_pair_batch(*keys, *numbers, by_of, pair_a, pair_b, *none, [0], [], [-1, -1], [-1] * (len(numbers[1]) - 1), FIX_STOP,
                                                       max_len, None, permille)
        except ia.FmxError as e:
            return e.code, str(e)

    assert call()[0] == 0
    for kw, word in ((dict(by_of=(1,)), "by_of"), (dict(pair_a=(2,)), "pair_a or pair_b"), (dict(pair_b=(-1,)), "pair_a or pair_b"),
                     (dict(pair_a=(), pair_b=()), "n_pairs == 0"), (dict(max_len=65), "max_len"), (dict(permille=(1001,)), "permille")):
        code, msg = call(**kw)
        assert code == E_ARG and word in msg, (kw, code, msg)
    bare = ia.FmIndex(HD[:4000], 16, True, device=0)
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    plain = ia.FmIndex(edge_text()[:6000], 8, False, device=0)
    try:
        code, msg = call(index=bare)
        assert code == E_ARG and "fmx_line_table_build" in msg
        code, msg = call(index=bare, by_of=(), numbers=none)  # (the pivot needs the line table too)
        assert code == E_ARG and "fmx_line_table_build" in msg
        assert call(index=host_only)[0] == E_NO_DEVICE
        plain.build_line_table("\n")
        text = edge_text()[:6000]
        out = plain.number_stats_by_pair_batch(*ia.pack_patterns([ia.as_chars("k="), ia.as_chars("c=")]), *ia.pack_patterns([ia.as_chars("n=")]), [0], [0], [1], *none,
                                               [0], [], [-1, -1], [-1], " \n", 32)
        assert out["val_off"].tolist() == [0, 0, 0] and out["pair_off"].tolist() == [0, 0] and out["row_off"].tolist() == [0, 0] and len(out["count"]) == 0
        assert (out["status"] == ST_NOT_ENABLED).all() and (out["key_status"] == ST_NOT_ENABLED).all()
        assert out["kept"].tolist() == [text.count("n=")] and out["key_kept"].tolist() == [text.count("k="), text.count("c=")] and out["no_key"].tolist() == [0]
        out = plain.number_stats_by_pair_batch(*ia.pack_patterns([ia.as_chars("k="), ia.as_chars("c=")]), *none, [], [0], [1], *none, [0], [], [-1, -1], [], " \n", 32)
        assert out["pair_off"].tolist() == [0, 0] and (out["key_status"] == ST_NOT_ENABLED).all()
    finally:
        bare.close()
        host_only.close()
        plain.close()


# ---- 4. launch shapes ----
def made_up_lists(rng, per, n_lines, groups):
    """per[k] distinct lines of [0, n_lines) for key pattern k, ascending, each with a group of [0, groups[k])"""
    first_off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    first_lines = np.concatenate([np.sort(rng.choice(n_lines, p, replace=False)) for p in per] + [np.zeros(0, np.int64)]).astype(np.int32)
    group = np.concatenate([rng.integers(0, max(g, 1), p) for p, g in zip(per, groups)] + [np.zeros(0, np.int64)]).astype(np.int32)
    val_off = np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)
    return first_off, first_lines, group, val_off


def test_launch_shapes_slots(hd):
    """made-up first-hit lists large enough for a second and a third pass of every loop over the slots (k_pair_keys, k_pair_heads,
    k_pair_store, k_pair_back, k_pair_compact): the sizes come from fmx_hit_lines_geometry and the pass counts are asserted first.
    One a-side of few groups and one whose groups are as many as its lines; an empty key pattern.  The stage's kernels have 256 lanes
    and fmx_hit_lines_geometry's grid whatever the options say, so the run with block = 1024 set must give the default's arrays:
    the option does not reach this stage, and the comparison holds it to that"""
    o, fm, T = hd
    KEY, FLAT = caps(fm)
    rng = np.random.default_rng(20241022)
    A, B = FLAT + FLAT // 3, FLAT + 1
    n_lines = 2 * A
    first_off, first_lines, group, val_off = made_up_lists(rng, [A, 0, B], n_lines, [A, 7, 50])
    group[:A] = rng.permutation(A)  # as many groups as lines on the first a-side
    pairs = [(0, 2), (1, 0), (2, 0), (0, 0)]
    n_slots = 2 * A + B + 70
    assert_loops("pairs, slots", k_pair_keys=flat_passes(fm, n_slots), k_pair_heads=flat_passes(fm, n_slots + 1, grid_of=n_slots),
                 k_pair_store=flat_passes(fm, n_slots), k_pair_back=flat_passes(fm, n_slots + 1, grid_of=n_slots), k_pair_compact=flat_passes(fm, n_slots))
    want = np_join(first_off, first_lines, group, val_off, pairs)
    assert want["pair_off"][1] > B // 4 and want["pair_off"][2] == want["pair_off"][1] and want["pair_off"][4] - want["pair_off"][3] == A
    runs = []
    for kw in (dict(block=1024), dict()):
        with options(**kw):
            rc, got = dev_join(fm, first_off, first_lines, group, val_off, pairs, lead=3, extra=70)
        assert rc == 0, last_error()
        check_whole(got, type("Want", (), want), JOIN_NAMES, "three passes over the slots, %r" % kw)
        runs.append(got)
    for name in JOIN_NAMES:
        assert (runs[0][name] == runs[1][name]).all(), name


def test_launch_shapes_pairs(hd):
    """more pairs of the call than three grids of lanes: the loops over j <= c of k_pair_lens, k_pair_store and k_pair_compact, with few
    slots (most a-sides are empty key patterns), so that the grid is small and the offsets hold long runs of equal entries; with
    block = 1024 set and with the default, which must not differ (no option reaches this stage)"""
    o, fm, T = hd
    rng = np.random.default_rng(20241023)
    first_off, first_lines, group, val_off = made_up_lists(rng, [3, 0, 2, 0, 0, 4, 0, 0], 40, [3, 1, 2, 1, 1, 2, 1, 1])
    c = 20_000
    empty, full = np.array([1, 3, 4, 6, 7]), np.array([0, 2, 5])
    pa = np.where(rng.random(c) < 0.9, empty[rng.integers(0, 5, c)], full[rng.integers(0, 3, c)])
    pb = rng.integers(0, 8, c)
    pairs = list(zip(pa.tolist(), pb.tolist()))
    n_slots = int((first_off[pa + 1] - first_off[pa]).sum()) + 70
    assert_loops("pairs, pairs of the call", k_pair_lens=flat_passes(fm, c + 1, grid_of=n_slots), k_pair_store=flat_passes(fm, c + 1, grid_of=n_slots),
                 k_pair_compact=flat_passes(fm, c + 1, grid_of=n_slots))
    want = np_join(first_off, first_lines, group, val_off, pairs)
    assert 0 < want["pair_off"][-1] < n_slots and (np.diff(want["pair_off"]) == 0).sum() > c // 2
    runs = []
    for kw in (dict(block=1024), dict()):
        with options(**kw):
            rc, got = dev_join(fm, first_off, first_lines, group, val_off, pairs, lead=3, extra=70)
        assert rc == 0, last_error()
        check_whole(got, type("Want", (), want), JOIN_NAMES, "three passes over the pairs, %r" % kw)
        runs.append(got)
    for name in JOIN_NAMES:
        assert (runs[0][name] == runs[1][name]).all(), name


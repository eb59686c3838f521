"""Statistics of the number behind a pattern, grouped by the value of a field of the same line, on the GPU: the three device stages
(fmx_first_hits_of_lines_dev: fmx_hit_first.hip; fmx_values_of_hits_groups_dev: the twin launcher of fmx_hit_values.hip;
fmx_numbers_by_key_dev: the "by" kernels of fmx_hit_numbers.hip), the host form fmx_number_stats_by_batch and the Python
convenience FmIndex.number_stats_by.

The judge is judge_by (tests/test_number_stats_by_cpu.py), computed once per case and shared; on the edge text the regular
expressions of that file judge the judge.  The device stages run over the judge's KEPT hits, uploaded as a packed block with slots
in front of and behind the hits; the host form runs the whole call.  Every output is prefilled with a sentinel and padded, and what
lies behind the answer must keep it.  Options are set inside the tests and put back in `finally`.  Every refused call returns before
a launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_where_cpu import EVERY_LINE, Where
from test_gpu_field_values import ST_NOT_ENABLED, last_error
from test_gpu_locate_rows import _torch, options
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_stats_by_cpu import EDGE_KEYS, EDGE_LINES, EDGE_NUMBERS, assert_fixture_figures, assert_regex, check_by, edge_text, judge_by

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel
E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
ROW_NAMES = ("count", "sum_lo", "sum_hi", "min", "max", "pct", "no_key", "not_number", "overflow")


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def filled(count, dtype):
    torch = _torch()
    return torch.full((count + PAD,), SENT, dtype=dtype, device="cuda")


def cut(t, count, what):
    a = t.cpu().numpy()
    assert (a[count:] == SENT).all(), "stored beyond the answer: " + what
    return a[:count]


class Block:
    """the judge's kept hits of a Where (m key patterns, then the number patterns) as ONE packed block on the device: `lead` slots in
    front that hold no hit (hit_off[0] = lead), `extra` behind"""

    def __init__(self, w, lead=0, extra=0):
        torch = _torch()
        self.hit_off = torch.from_numpy((w.kept_off + lead).astype(np.int64)).cuda()
        self.locs = torch.from_numpy(np.concatenate([np.full(lead, -5, np.int32), w.kept_locs, np.full(extra, -5, np.int32)]).astype(np.int32)).cuda()
        self.slots = lead + int(w.kept_off[-1]) + extra


def dev_by(fm, w, m, by_of, stop, max_len, permille=(500, 950), frac_digits=0, lead=0, extra=0, short=None):
    """the three stages and the fill over a Block; rc of the stage that refused (and its name), or 0 and a dict under the judge's
    names.  short = (stage, bytes): that stage gets a workspace that many bytes too small"""
    torch = _torch()
    lib, n, st = ia.lib, w.n - m, stream()
    b = Block(w, lead, extra)
    key_end = int(w.kept_off[m]) + lead
    a_slots = min(b.slots, key_end + extra)  # (slots behind hit_off[m] — number hits, or nothing — are no hits to stage a)
    K = max(int(w.kept_off[m]), 1)

    def ws_of(stage, need):
        use = need - (short[1] if short and short[0] == stage else 0)
        return torch.empty(max(use, 1), dtype=torch.uint8, device="cuda"), use

    # stage a over the slots [0, key_end) and up to `extra` behind them
    first_off, first_lines, first_locs = filled(m + 1, torch.int64), filled(K, torch.int32), filled(K, torch.int32)
    ws, use = ws_of("a", lib.fmx_first_hits_of_lines_scratch_bytes(m, a_slots))
    rc = lib.fmx_first_hits_of_lines_dev(fm.handle, m, b.hit_off.data_ptr(), b.locs.data_ptr(), a_slots, first_off.data_ptr(), first_lines.data_ptr(),
                                         first_locs.data_ptr(), ws.data_ptr(), use, st)
    torch.cuda.synchronize()
    if rc:
        assert all((t.cpu().numpy() == SENT).all() for t in (first_off, first_lines, first_locs))
        return rc, "a"
    got = dict(first_off=cut(first_off, m + 1, "first_off"))
    F = int(got["first_off"][m])
    got.update(first_lines=cut(first_lines, F, "first_lines"), first_locs=cut(first_locs, F, "first_locs"))
    # stage b over the first hits: K slots, those behind first_off[m] are no hits
    val_off, lines, text_off, group = filled(m + 1, torch.int64), filled(K, torch.int32), filled(K + 1, torch.int64), filled(K, torch.int32)
    status = torch.zeros(m + n + 1, dtype=torch.int32, device="cuda")
    tl, sp = np.array(w.lens[:m], np.int32), ia.as_chars(stop).astype(np.uint16)
    ws_b, use = ws_of("b", lib.fmx_values_of_hits_groups_scratch_bytes(m, K, max_len))
    rc = lib.fmx_values_of_hits_groups_dev(fm.handle, m, tl.ctypes.data, sp.ctypes.data if len(sp) else None, len(sp), max_len, first_off.data_ptr(),
                                           first_locs.data_ptr(), K, val_off.data_ptr(), lines.data_ptr(), text_off.data_ptr(), group.data_ptr(),
                                           status.data_ptr(), ws_b.data_ptr(), use, st)
    tl[:] = -9  # (the call has copied what it needs before it returns)
    sp[:] = 9
    torch.cuda.synchronize()
    if rc:
        assert all((t.cpu().numpy() == SENT).all() for t in (val_off, lines, text_off, group))
        return rc, "b"
    got["val_off"] = cut(val_off, m + 1, "val_off")
    G = int(got["val_off"][m])
    got.update(lines=cut(lines, G, "lines"), text_off=cut(text_off, G + 1, "text_off"))
    g_all = group.cpu().numpy()
    assert (g_all[F:K] == -1).all() and (g_all[K:] == SENT).all(), "the groups of the slots behind the first hits"
    got["group_of_first"] = g_all[:F]
    units = int(got["text_off"][G]) if G else 0
    chars = torch.full((units + PAD,), 0x7A7A, dtype=torch.int16, device="cuda")
    assert lib.fmx_values_fill_dev(fm.handle, G, text_off.data_ptr(), chars.data_ptr(), ws_b.data_ptr(), max(use, 0), st) == 0, last_error()
    torch.cuda.synchronize()
    c = chars.cpu().numpy()
    assert (c[units:] == 0x7A7A).all(), "stored beyond the answer: chars"
    got["chars"] = c[:units].view(np.uint16)
    # stage c over the numbers' part: hit_off + m, the slots [0, all_end + extra)
    voff = got["val_off"].astype(np.int64).copy()
    groups = np.diff(voff)
    R, P = int(groups[np.asarray(by_of, np.int64)].sum()) if n else 0, len(permille)
    sizes = dict(count=R, sum_lo=R, sum_hi=R, min=R, max=R, pct=R * P, no_key=n, not_number=n, overflow=n)
    out = {k: filled(sizes[k], torch.int32 if k in ("count", "no_key", "not_number", "overflow") else torch.int64) for k in ROW_NAMES}
    row_off = filled(n + 1, torch.int64)
    tl, bo, pm = np.array(w.lens[m:], np.int32), np.array(by_of, np.int32), np.array(permille, np.int32)
    ws_c, use = ws_of("c", lib.fmx_numbers_by_key_scratch_bytes(n, b.slots, P))
    rc = lib.fmx_numbers_by_key_dev(fm.handle, n, tl.ctypes.data, bo.ctypes.data, m, voff.ctypes.data, b.hit_off.data_ptr() + 8 * m, b.locs.data_ptr(),
                                    b.slots, first_off.data_ptr(), first_lines.data_ptr(), group.data_ptr(), frac_digits, pm.ctypes.data if P else None, P,
                                    row_off.data_ptr(), *(out[k].data_ptr() for k in ROW_NAMES), status.data_ptr() + 4 * m, ws_c.data_ptr(), use, st)
    for a in (tl, bo, pm, voff):
        a[:] = -9
    torch.cuda.synchronize()
    if rc:
        assert all((t.cpu().numpy() == SENT).all() for t in list(out.values()) + [row_off])
        return rc, "c"
    got["row_off"] = cut(row_off, n + 1, "row_off")
    for k in ROW_NAMES:
        a = cut(out[k], sizes[k], k)
        got[k] = a.view(np.uint64) if k.startswith("sum") else a
    assert (status.cpu().numpy() == 0).all()
    return 0, got


def host_by(fm, w, m, by_of, stop, max_len, permille=(500, 950), frac_digits=0):
    kch, koff = ia.pack_patterns(w.patterns[:m])
    nch, noff = ia.pack_patterns(w.patterns[m:])
    return fm.number_stats_by_batch(kch, koff, nch, noff, by_of, *w.term_arrays(), w.query_off, w.kinds, w.where_of[:m], w.where_of[m:], stop, max_len,
                                    None if w.window == EVERY_LINE else w.window, permille, frac_digits)


_JUDGED = {}


def case(tag, fm, o, T, keys, numbers, by_of, stop, max_len, queries=(), key_where=None, where=None, window=EVERY_LINE, permille=(500, 950), frac_digits=0,
         device=True, lead=3, extra=70):
    """the judge (once per case), the host form and — where the call does not filter through its own queries only — the device stages"""
    m = len(keys)
    where_of = list(key_where or [-1] * m) + list(where or [-1] * len(numbers))
    key = (tag, tuple(keys), tuple(numbers), tuple(by_of), stop, max_len, repr(queries), tuple(where_of), window, tuple(permille), frac_digits)
    if key not in _JUDGED:
        w = Where(tag, o, T, list(keys) + list(numbers), list(queries), where_of, window)
        _JUDGED[key] = w, judge_by(o, w, T, m, by_of, stop, max_len, permille, frac_digits)
    w, want = _JUDGED[key]
    what = "%s %r by %r" % (tag, numbers, keys)
    got = host_by(fm, w, m, by_of, stop, max_len, permille, frac_digits)
    check_by(got, want, what + ", host form")
    assert (got["kept"] == want.kept).all() and (got["key_kept"] == want.key_kept).all() and (got["occurrences"] == w.occurrences[m:]).all(), what
    assert (got["key_occurrences"] == w.occurrences[:m]).all() and (got["status"] == 0).all() and (got["key_status"] == 0).all(), what
    assert (got["term_status"] == w.term_status).all(), what
    for i in range(want.n):  # the invariant
        rows = got["count"][got["row_off"][i]:got["row_off"][i + 1]]
        assert rows.sum() + got["no_key"][i] + got["not_number"][i] + got["overflow"][i] == got["kept"][i], what
    if device and w.kept[:m].sum() > 0:
        rc, dev = dev_by(fm, w, m, by_of, stop, max_len, permille, frac_digits, lead, extra)
        assert rc == 0, (dev, last_error())
        check_by(dev, want, what + ", device stages", stages=True)
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


def fixture_get(hd):
    o, fm, T = hd

    def get(number, key, stop, where):
        q = dict(queries=[where], key_where=[0], where=[0]) if where else {}
        want = case("hd16 by", fm, o, T, [key], [number], [0], stop, 32, **q)
        s = fm.number_stats_by(number, key, stop, 32, where)  # the convenience: the same groups
        assert [g["value"] for g in s.groups] == want.strings() and [g["lines"] for g in s.groups] == want.lines.tolist()
        assert [(g["count"], g["sum"], g["min"], g["max"]) for g in s.groups] == [want.row(0, v) for v in want.strings()]
        assert [g["pct"] for g in s.groups] == want.pct.tolist()
        assert (s.no_key, s.not_number, s.overflow, s.kept) == (int(want.no_key[0]), int(want.not_number[0]), int(want.overflow[0]), int(want.kept[0]))
        return want

    return get


# ---- 1. the fixture's figures ----
def test_fixture_figures(hd):
    """the issue's figures through the host form, the Python convenience and the three device stages, each against the judge"""
    assert_fixture_figures(fixture_get(hd))
    o, fm, T = hd
    s = fm.number_stats_by("size ", "updated: 10.", ".:", top=1)
    assert [(g["value"], g["lines"], g["count"]) for g in s.groups] == [("251", 210, 176)] and abs(s.groups[0]["mean"] - 11_326_104_278 / 176) < 1e-6
    assert fm.number_stats_by("size ", "zzqq#").groups == [] and fm.number_stats_by("size ", "zzqq#").no_key == 608
    empty = fm.number_stats_by("zzqq#", "INFO ", " :")
    assert len(empty.groups) > 60  # (the groups are the key's, whatever the number pattern finds)
    assert all(g["count"] == 0 and np.isnan(g["mean"]) for g in empty.groups) and empty.kept == 0


# ---- 2. cross-checks on the fixture ----
def test_fixture_cross_checks(hd):
    o, fm, T = hd
    # one hit of "INFO " per line: the groups and their lines are field_values' values and counts
    want = case("hd16 by", fm, o, T, ["INFO "], ["size "], [0], " :", 32)
    chars, text_off, counts, val_off = fm.field_values_where_batch(*ia.pack_patterns([ia.as_chars("INFO ")]), *ia.pack_patterns([]), [0], [], [-1], " :", 32)[:4]
    assert (val_off == want.val_off).all() and (counts == want.lines).all() and (chars == want.chars).all() and (text_off == want.text_off).all()
    # three groups against number_stats under a filter term that selects the group's lines
    by = fm.number_stats_by("size ", "updated: 10.", ".:").by_value()
    for value, where in (("250", dict(all=["updated: 10.250"])), ("251", dict(all=["updated: 10.251"]))):
        s = fm.number_stats("size ", where=where)
        g = by[value]
        assert (g["count"], g["sum"], g["min"], g["max"], g["pct"]) == (int(s.count[0]), s.sum[0], int(s.min[0]), int(s.max[0]), s.pct[0].tolist())
    g = fm.number_stats_by("size ", "INFO ", " :", where=dict(all=["addStoredBlock"])).by_value()["dfs.FSNamesystem"]
    s = fm.number_stats("size ", where=dict(all=["addStoredBlock", "INFO dfs.FSNamesystem:"]))
    assert (g["count"], g["sum"], g["min"], g["max"], g["pct"]) == (int(s.count[0]), s.sum[0], int(s.min[0]), int(s.max[0]), s.pct[0].tolist())
    # two number patterns on one key, two keys in one call: what the single calls give
    both = case("hd16 by", fm, o, T, ["INFO ", "updated: 10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, permille=(0, 500, 1000))
    for i, (number, key) in enumerate((("size ", "INFO "), ("blk_", "INFO "), ("size ", "updated: 10."))):
        alone = case("hd16 by", fm, o, T, [key], [number], [0], " :.", 16, permille=(0, 500, 1000))
        a, b = int(both.row_off[i]), int(both.row_off[i + 1])
        assert (both.count[a:b] == alone.count).all() and both.sums[a:b] == alone.sums and (both.pct[a:b] == alone.pct).all()
        assert both.strings(int(both.by_of[i])) == alone.strings(0)


# ---- 3. the edge text ----
def test_edge_text(edge):
    """every case of the edge text (tests/test_number_stats_by_cpu.py names them) through the device stages and the host form"""
    text, o, fm, T = edge
    for stop, max_len in ((" \n", 32), (" ", 32), (" \n", 1), (" \n", 64)):
        want = case("edge", fm, o, T, EDGE_KEYS, EDGE_NUMBERS, [0, 0, 0], stop, max_len, permille=(0, 500, 950, 1000))
        assert_regex(want, 0, 0, text, "k=", "n=", stop, max_len)
    vals = want.strings(0)
    assert "" in vals and "b" in vals and "a" not in vals and want.lines_of("far") == 2 and want.row(0, "last")[:2] == (1, 42)
    assert want.row(0, "zz9") == (0, 0, 0, 0) and want.lines_of("zz9") == 1 and int(want.no_key[0]) == 4
    assert vals[vals.index("ab"):vals.index("ab") + 3] == ["ab", "ab\0", "ab\0\0"] and want.row(0, "ab\0")[:2] == (1, 51) and want.lines_of("ab") == 2
    nl = case("edge", fm, o, T, ["k="], ["n="], [0], " ", 32)
    assert nl.row(0, "\ntail21")[:2] == (1, 3)
    for F in (0, 3, 9):  # a permuting by_of, a key pattern without a hit, one group only, as many groups as lines
        want = case("edge", fm, o, T, EDGE_KEYS, EDGE_NUMBERS, [3, 1, 2], " \n", 32, permille=(500,), frac_digits=F)
        assert want.no_key[0] == want.kept[0] > EDGE_LINES and want.val_off[2] - want.val_off[1] == EDGE_LINES and want.val_off[3] - want.val_off[2] == 1
    s = fm.number_stats_by("n=", "k=", " \n", frac_digits=3).by_value()
    assert s["v3"]["min"] == 123 and s["b"]["count"] == 1 and s["b"]["sum"] == 5000
    big = fm.number_stats_by("n=", "k=", " \n").by_value()["v3"]
    assert big["max"] == 2 ** 63 - 1 and big["sum"] > 2 ** 63  # the sum runs past 64 bits' signed half
    one = fm.number_stats_by("m=", "c=", " \n")
    assert len(one.groups) == 1 and one.groups[0]["lines"] == EDGE_LINES
    # no slots in front, none behind; exactly the hits
    case("edge", fm, o, T, ["k="], ["n="], [0], " \n", 32, lead=0, extra=0)


# ---- 4. geometry ----
def test_geometry(hd, edge):
    """1,024-lane workgroups and grids that loop: the packed extract of stages b and c honours them"""
    o, fm, T = hd
    text, eo, efm, eT = edge
    for kw in (dict(block=1024), dict(groups_per_cu=1), dict(block=1024, groups_per_cu=1)):
        with options(**kw):
            case("hd16 by", fm, o, T, ["INFO ", "updated: 10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, permille=(0, 500, 1000))
            case("edge", efm, eo, eT, EDGE_KEYS, EDGE_NUMBERS, [0, 0, 0], " \n", 32, permille=(0, 500, 950, 1000))


# ---- 5. filters ----
def test_filters(edge):
    """a window that cuts a group in two, a filter that keeps no key hit, one that keeps no number hit, key_where_of different
    from where_of (a line that passes for the number and not for the key gives no_key).  The entry point takes no ranged terms."""
    text, o, fm, T = edge
    cut2 = case("edge", fm, o, T, ["k="], ["n="], [0], " \n", 32, window=(150, 2101))
    assert cut2.lines_of("far") == 1 and cut2.lines_of("nb") == 3
    q = [dict(all=["nokey"]), dict(all=["k=far"]), dict(all=["only"])]
    none = case("edge", fm, o, T, ["k="], ["n="], [0], " \n", 32, queries=q, key_where=[0], where=[-1])
    assert none.val_off[1] == 0 and none.no_key[0] == none.kept[0] > EDGE_LINES
    empty = case("edge", fm, o, T, ["k="], ["n="], [0], " \n", 32, queries=q, key_where=[-1], where=[2])
    assert empty.kept[0] == 0 and empty.val_off[1] > 10 and sum(empty.count) == 0
    mixed = case("edge", fm, o, T, ["k="], ["n="], [0], " \n", 32, queries=q, key_where=[1], where=[-1])
    assert mixed.strings(0) == ["far"] and mixed.row(0, "far")[:2] == (2, 2200) and mixed.no_key[0] == mixed.kept[0] - 2
    s = fm.number_stats_by("n=", "k=", " \n", where=dict(all=["k=far"]), lines=(0, 2000))
    assert [(g["value"], g["lines"], g["sum"]) for g in s.groups] == [("far", 1, 100)] and s.no_key == 0 and s.kept == 1
    for kw in (dict(), dict(where=dict(all=["k=far"]))):  # neither pattern has a hit, without a filter and with one
        s = fm.number_stats_by("zzqq%", "zzqq#", " \n", **kw)
        assert s.groups == [] and (s.no_key, s.not_number, s.overflow, s.kept, s.key_kept) == (0, 0, 0, 0, 0)


# ---- 6. refusals ----
def test_refusals(hd):
    """each returns before a launch and leaves every output untouched (dev_by asserts the sentinels)"""
    o, fm, T = hd
    w = Where("hd16 by", o, T, ["INFO ", "size "], [], [-1, -1])
    keys, numbers, none = ia.pack_patterns([ia.as_chars("INFO ")]), ia.pack_patterns([ia.as_chars("size ")]), ia.pack_patterns([])

    def call(index=fm, by_of=(0,), stop=" :", max_len=8, permille=(500,), frac_digits=0, keys=keys):
        try:
            index.number_stats_by_batch(*keys, *numbers, by_of, *none, [0], [], [-1] * (len(keys[1]) - 1), [-1], stop, max_len, None, permille, frac_digits)
        except ia.FmxError as e:
            return e.code, str(e)
        return 0, ""

    assert call()[0] == 0
    for kw, word in ((dict(by_of=(1,)), "by_of[0]"), (dict(keys=none), "m == 0"), (dict(max_len=0), "max_len"), (dict(max_len=65), "max_len"),
                     (dict(stop="x" * 65), "stop set"), (dict(frac_digits=10), "frac_digits"), (dict(permille=(1001,)), "permille"),
                     (dict(permille=tuple(range(17))), "n_permille")):
        code, msg = call(**kw)
        assert code == E_ARG and word in msg, (kw, code, msg)
    # a workspace one byte too small, for each device stage
    for stage, word in (("a", "fmx_first_hits_of_lines_scratch_bytes"), ("b", "fmx_values_of_hits_groups_scratch_bytes"), ("c", "fmx_numbers_by_key_scratch_bytes")):
        rc, where = dev_by(fm, w, 1, [0], " :", 8, short=(stage, 1))
        assert rc == E_ARG and where == stage and word in last_error(), (stage, rc, where, last_error())
    # no line table; a handle that is not resident; a SuffixArray handle
    bare = ia.FmIndex(HD[:4000], 16, True, device=0)
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    try:
        sa.construct()
        code, msg = call(index=bare)
        assert code == E_ARG and "fmx_line_table_build" in msg
        assert call(index=host_only)[0] == E_NO_DEVICE
        torch = _torch()
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        p, one = t.data_ptr(), np.zeros(4, np.int32)
        voff = np.array([0, 1], np.int64)
        for h, code, word in ((bare.handle, E_ARG, "fmx_line_table_build"), (host_only.handle, E_NO_DEVICE, ""), (sa._h, E_ARG, "")):
            assert ia.lib.fmx_first_hits_of_lines_dev(h, 1, p, p, 4, p, p, p, p, 1 << 20, stream()) == code and word in last_error()
            assert ia.lib.fmx_numbers_by_key_dev(h, 1, one.ctypes.data, one.ctypes.data, 1, voff.ctypes.data, p, p, 4, p, p, p, 0, None, 0, p, p, p, p, p, p,
                                                 p, p, p, p, p, p, 1 << 20, stream()) == code and word in last_error()
        for h, code in ((host_only.handle, E_NO_DEVICE), (sa._h, E_ARG)):
            assert ia.lib.fmx_values_of_hits_groups_dev(h, 1, one.ctypes.data, None, 0, 8, p, p, 4, p, p, p, p, p, p, 1 << 20, stream()) == code
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0).all()
        # more than 2^27 rows: two number patterns on a key pattern of 2^26 + 1 groups (the HOST array decides: nothing is launched)
        wide = np.array([0, 2 ** 26 + 1], np.int64)
        two = np.zeros(2, np.int32)
        assert ia.lib.fmx_numbers_by_key_dev(fm.handle, 2, two.ctypes.data, two.ctypes.data, 1, wide.ctypes.data, p, p, 4, p, p, p, 0, None, 0, p, p, p, p, p,
                                             p, p, p, p, p, p, p, 1 << 20, stream()) == E_ARG and "2^27 rows" in last_error()
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0).all()
    finally:
        bare.close()
        host_only.close()


def test_index_without_extraction():
    """FMX_ST_NOT_ENABLED, no groups, no rows; occurrences and kept are still filled"""
    text = edge_text()[:6000]
    fm = ia.FmIndex(text, 8, False, device=0)
    try:
        fm.build_line_table("\n")
        out = fm.number_stats_by_batch(*ia.pack_patterns([ia.as_chars("k=")]), *ia.pack_patterns([ia.as_chars("n="), ia.as_chars("m=")]), [0, 0],
                                       *ia.pack_patterns([]), [0], [], [-1], [-1, -1], " \n", 32)
        assert out["val_off"].tolist() == [0, 0] and out["row_off"].tolist() == [0, 0, 0] and len(out["count"]) == 0
        assert (out["status"] == ST_NOT_ENABLED).all() and (out["key_status"] == ST_NOT_ENABLED).all()
        assert out["kept"].tolist() == [text.count("n="), text.count("m=")] == out["occurrences"].tolist() and out["key_kept"].tolist() == [text.count("k=")]
        assert out["no_key"].tolist() == [0, 0] and out["not_number"].tolist() == [0, 0]
        # neither the key pattern nor the number pattern has a hit: nothing runs, the statuses still say why there are no groups
        out = fm.number_stats_by_batch(*ia.pack_patterns([ia.as_chars("zzqq#")]), *ia.pack_patterns([ia.as_chars("zzqq%")]), [0],
                                       *ia.pack_patterns([]), [0], [], [-1], [-1], " \n", 32)
        assert out["val_off"].tolist() == [0, 0] and out["row_off"].tolist() == [0, 0] and len(out["count"]) == 0
        assert (out["status"] == ST_NOT_ENABLED).all() and (out["key_status"] == ST_NOT_ENABLED).all()
        assert out["kept"].tolist() == [0] == out["occurrences"].tolist() and out["key_kept"].tolist() == [0] and out["no_key"].tolist() == [0]
    finally:
        fm.close()


# ---- 7. the old entry points ----
def test_values_of_hits_is_what_it_was(hd):
    """fmx_values_of_hits_scratch_bytes keeps its size (the twin's is its own, larger one) and fmx_values_of_hits_dev its answers:
    over the same hits the twin gives the same groups (tests/test_gpu_field_values.py holds the old entry point to the judge)"""
    o, fm, T = hd
    w = Where("hd16 by", o, T, ["INFO ", "blk_"], [], [-1, -1], EVERY_LINE, " :", 32)
    torch = _torch()
    n, H = 2, int(w.kept_off[-1])
    need_old, need_new = ia.lib.fmx_values_of_hits_scratch_bytes(n, H, 32), ia.lib.fmx_values_of_hits_groups_scratch_bytes(n, H, 32)
    assert need_new - need_old == (4 * (H + 1) + 255) // 256 * 256 + 256
    hit_off, locs = torch.from_numpy(np.array(w.kept_off)).cuda(), torch.from_numpy(np.array(w.kept_locs)).cuda()
    tl, sp = np.array(w.lens, np.int32), ia.as_chars(" :").astype(np.uint16)
    outs = []
    for twin in (False, True):
        val_off, count, text_off, group = filled(n + 1, torch.int64), filled(H, torch.int32), filled(H + 1, torch.int64), filled(H, torch.int32)
        ws = torch.empty(need_new if twin else need_old, dtype=torch.uint8, device="cuda")
        head = (fm.handle, n, tl.ctypes.data, sp.ctypes.data, len(sp), 32, hit_off.data_ptr(), locs.data_ptr(), H, val_off.data_ptr(), count.data_ptr(),
                text_off.data_ptr())
        tail = (None, ws.data_ptr(), ws.numel(), stream())
        rc = ia.lib.fmx_values_of_hits_groups_dev(*head, group.data_ptr(), *tail) if twin else ia.lib.fmx_values_of_hits_dev(*head, *tail)
        assert rc == 0, last_error()
        torch.cuda.synchronize()
        outs.append((cut(val_off, n + 1, "val_off"), count.cpu().numpy(), text_off.cpu().numpy(), group.cpu().numpy()))
    old, new = outs
    G = int(w.values.val_off[-1])
    assert (old[0] == w.values.val_off).all() and (old[1][:G] == w.values.counts).all() and (old[3] == SENT).all()
    assert all((a == b).all() for a, b in zip(old[:3], new[:3]))
    # the group of every hit: the hits of group g are counts[g] many
    for p in range(n):
        a, b = int(w.kept_off[p]), int(w.kept_off[p + 1])
        groups = new[3][a:b]
        assert (np.bincount(groups, minlength=int(old[0][p + 1] - old[0][p])) == old[1][old[0][p]:old[0][p + 1]]).all()


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_number_stats_by_mirror.cpp prints what numberStatsByBatch returns, and holds numberStatsBy to the fixture's figures"""
    o, fm, T = hd
    exe = str(tmp_path / "test_number_stats_by_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_number_stats_by_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    w = Where("hd16 by mirror", o, T, ["INFO ", "updated: 10.", "size ", "blk_", "size "], [dict(all=["addStoredBlock"])], [-1, -1, 0, -1, -1])
    want = judge_by(o, w, T, 2, [0, 0, 1], " :.", 16, (0, 500, 1000), 0)
    assert out["val_off"] == want.val_off.tolist() and out["row_off"] == want.row_off.tolist() and out["lines"] == want.lines.tolist()
    assert out["count"] == want.count.tolist() and out["min"] == want.min.tolist() and out["max"] == want.max.tolist() and out["pct"] == want.pct.ravel().tolist()
    sums = [(hi << 64) | lo for lo, hi in zip(out["sum_lo"], out["sum_hi"])]
    assert sums == want.sums and max(sums) > 2 ** 64
    assert out["no_key"] == want.no_key.tolist() and out["not_number"] == want.not_number.tolist() and out["overflow"] == want.overflow.tolist()
    assert out["kept"] == want.kept.tolist() and out["key_kept"] == want.key_kept.tolist() and out["occurrences"] == [608, 2468, 608] and out["status"] == [0] * 3
    values = [u for k in range(2) for v in want.strings(k) for u in [ord(c) for c in v] + [0xFFFF]]
    assert out["values"] == values


# ---- the class form ----
def test_class_form(hd):
    """fmx_number_stats_by_class_batch: class patterns of one spelling give the literal form's answer on the fixture; on a text of
    mixed case ignore_case= joins the spellings of key pattern, number pattern and filter term (figures read off the text)"""
    o, fm, T = hd
    want = case("hd16 by", fm, o, T, ["INFO ", "updated: 10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, permille=(0, 500, 1000))
    single = lambda ps: ia.pack_class_patterns([list(p) for p in ps])  # noqa: E731
    got = fm.number_stats_by_class_batch(*single(["INFO ", "updated: 10."]), *single(["size ", "blk_", "size "]), [0, 0, 1], *single([]), [0], [], [-1, -1],
                                         [-1, -1, -1], " :.", 16, None, (0, 500, 1000), 0)
    check_by(got, want, "class patterns of one spelling")
    assert (got["kept"] == want.kept).all() and (got["key_kept"] == want.key_kept).all() and (got["status"] == 0).all()
    filtered = case("hd16 by", fm, o, T, ["INFO "], ["size "], [0], " :", 32, queries=[dict(all=["addStoredBlock"])], key_where=[0], where=[0])
    got = fm.number_stats_by_class_batch(*single(["INFO "]), *single(["size "]), [0], *single(["addStoredBlock"]), [0, 1], [0], [0], [0], " :", 32)
    check_by(got, filtered, "class patterns of one spelling, filtered")
    with pytest.raises(ia.FmxError) as err:
        fm.number_stats_by_class_batch(*single(["INFO "]), *single(["size "]), [0], *single([]), [0], [], [-1], [-1], " :", 32, max_ranges=0)
    assert err.value.code == E_ARG
    with pytest.raises(ia.FmxError) as err:
        fm.number_stats_by_class_batch(*single(["INFO "]), *single(["size "]), [1], *single([]), [0], [], [-1], [-1], " :", 32)
    assert err.value.code == E_ARG and "by_of[0]" in str(err.value)
    text = "Status=200 Bytes=10 ok\nstatus=200 bytes=5 OK\nSTATUS=404 BYTES=7 ok\nstatus=404 none\nbytes=9 missing\nstatus=200 bytes=x Ok\n"
    mixed = ia.FmIndex(text, 4, True, device=0)
    try:
        mixed.build_line_table("\n")
        s = mixed.number_stats_by("bytes=", "status=", ignore_case=True)
        assert [(g["value"], g["lines"], g["count"], g["sum"], g["min"], g["max"]) for g in s.groups] == [("200", 3, 2, 15, 5, 10), ("404", 2, 1, 7, 7, 7)]
        assert (s.no_key, s.not_number, s.kept, s.key_kept) == (1, 1, 5, 5)
        exact = mixed.number_stats_by("bytes=", "status=")
        assert [(g["value"], g["lines"], g["count"], g["sum"]) for g in exact.groups] == [("200", 2, 1, 5), ("404", 1, 0, 0)] and exact.no_key == 1
        w = mixed.number_stats_by("bytes=", "status=", where=dict(all=["OK"]), ignore_case=True)  # the term in any case: four lines
        assert [(g["value"], g["lines"], g["sum"]) for g in w.groups] == [("200", 3, 15), ("404", 1, 7)] and (w.kept, w.not_number, w.no_key) == (4, 1, 0)
    finally:
        mixed.close()


# ---- more than 4,096 lines, more than 2,048 hitless patterns in a tile ----
def test_deep_line_table_and_wide_batches():
    """8,300 lines: the fences of k_first_lines and k_by_ranges no longer hold every entry of the line table (shift > 0), and the hits
    fill several tiles; 2,100 key patterns without a hit between two that have hits, and as many number patterns: a tile's slice of
    hit_off no longer fits the LDS copy.  The judge is the regular expressions of tests/test_number_stats_by_cpu.py"""
    from test_number_stats_by_cpu import regex_judge
    N = 8300
    text = "\n".join("id=%d k=v%d n=%d" % (i, i % 13, (i * 7919) % 1009) if i % 50 else "n=%d nokey%d" % (i, i) for i in range(N))
    fm = ia.FmIndex(text, 8, True, device=0)
    try:
        assert fm.build_line_table("\n") == N

        def judged(key, number):
            groups, no_key, nn, ov = regex_judge(text, key, number, " \n", 32)
            values = sorted(groups, key=lambda v: [ord(c) for c in v])
            return [(v, groups[v][0], len(groups[v][1]), sum(groups[v][1]), min(groups[v][1], default=0), max(groups[v][1], default=0)) for v in values], no_key

        def rows(s):
            return [(g["value"], g["lines"], g["count"], g["sum"], g["min"], g["max"]) for g in s.groups]

        for key in ("k=", "id="):
            s = fm.number_stats_by("n=", key, " \n")
            want, no_key = judged(key, "n=")
            assert rows(s) == want and s.no_key == no_key == N // 50 and s.kept == N
        absent = ["zq#%d" % j for j in range(2100)]
        keys, numbers = ["k="] + absent + ["id="], ["n="] + absent + ["n="]
        out = fm.number_stats_by_batch(*ia.pack_patterns([ia.as_chars(p) for p in keys]), *ia.pack_patterns([ia.as_chars(p) for p in numbers]),
                                       [0] + [1] * 2100 + [2101], *ia.pack_patterns([]), [0], [], [-1] * len(keys), [-1] * len(numbers), " \n", 32)
        assert (out["status"] == 0).all() and (out["key_status"] == 0).all() and (out["kept"][1:-1] == 0).all() and (out["no_key"][1:-1] == 0).all()
        assert int(out["row_off"][1]) == 13 == int(out["row_off"][2101]) and int(out["val_off"][1]) == 13 == int(out["val_off"][2101])
        assert rows(ia.NumberStatsBy(out, None, 0)) == judged("k=", "n=")[0]
        last = ia.NumberStatsBy(out, None, 2101)  # (its key pattern is by_of[2101] = 2101: "id=")
        assert rows(last) == judged("id=", "n=")[0] and last.key_kept == N - N // 50 and last.no_key == N // 50
    finally:
        fm.close()


# ---- the host forms' refusals leave the caller's arrays as they were ----
def test_host_form_refusals_leave_outputs_untouched(hd):
    o, fm, T = hd
    lib = ia.lib
    kch, koff = ia.pack_patterns([ia.as_chars("INFO ")])
    nch, noff = ia.pack_patterns([ia.as_chars("size ")])
    koff, noff = koff.astype(np.int32), noff.astype(np.int32)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    host_only = ia.FmIndex("k=a n=1\n", 4, True, device=None)
    bare = ia.FmIndex(HD[:4000], 16, True, device=0)

    def call(h=fm.handle, by_of=(0,), m=1, max_len=8, frac_digits=0, permille=(500,), key_where=(-1,), n_stop=2):
        ints = {k: np.full(4, SENT, np.int32) for k in ("no_key", "not_number", "overflow", "occurrences", "kept", "status", "key_occurrences", "key_kept",
                                                        "key_status")}
        val_off, row_off = np.full(4, SENT, np.int64), np.full(4, SENT, np.int64)
        ptrs = [C.c_void_p(0x5A5A) for _ in range(9)]
        bo, pm, kw, wo = np.array(by_of, np.int32), np.array(permille, np.int32), np.array(key_where, np.int32), np.array([-1], np.int32)
        stop, qoff, kinds = ia.as_chars(" :").astype(np.uint16), np.zeros(1, np.int32), np.zeros(1, np.uint8)
        tch, toff = np.zeros(1, np.uint16), np.zeros(1, np.int32)
        rc = lib.fmx_number_stats_by_batch(h, kch.ctypes.data, koff.ctypes.data, m, nch.ctypes.data, noff.ctypes.data, 1, bo.ctypes.data, tch.ctypes.data,
                                           toff.ctypes.data, 0, qoff.ctypes.data, kinds.ctypes.data, 0, kw.ctypes.data, wo.ctypes.data, 0, 2 ** 31 - 1, stop.ctypes.data, n_stop, max_len,
                                           frac_digits, pm.ctypes.data, len(pm), val_off.ctypes.data, C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ptrs[2]),
                                           row_off.ctypes.data, *(C.byref(x) for x in ptrs[3:]), *(ints[k].ctypes.data for k in ints), None)
        untouched = all((a == SENT).all() for a in list(ints.values()) + [val_off, row_off])
        return rc, untouched, [x.value for x in ptrs]

    try:
        rc, _, ptrs = call()
        assert rc == 0 and ptrs[0] not in (None, 0x5A5A), last_error()
        lib.fmx_free_buffer(C.c_void_p(ptrs[0]))
        for kw, code, word in ((dict(by_of=(1,)), E_ARG, "by_of[0]"), (dict(m=0), E_ARG, "m == 0"), (dict(max_len=65), E_ARG, "max_len"),
                               (dict(n_stop=65), E_ARG, "stop set"), (dict(frac_digits=10), E_ARG, "frac_digits"), (dict(permille=(1001,)), E_ARG, "permille"),
                               (dict(key_where=(0,)), E_ARG, "where_of"), (dict(h=bare.handle), E_ARG, "fmx_line_table_build"),
                               (dict(h=host_only.handle), E_NO_DEVICE, ""), (dict(h=sa._h), E_ARG, "")):
            rc, untouched, ptrs = call(**kw)
            # (the pointers to the ONE allocation are NULL on every failure, as fmx_field_values_batch leaves its own)
            assert rc == code and word in last_error() and untouched and all(p is None for p in ptrs), (kw, rc, last_error(), untouched, ptrs)
    finally:
        bare.close()
        host_only.close()

"""The top values of a field per bucket of lines, the stacked timeline (fmx_values_top_histogram_dev, fmx_values_gather_rows_dev,
fmx_field_values_histogram_where_batch; count by status over time where line has ...) on the CPU: the functions the kernels of
index4j_amd/csrc/fmx_value_hist.hip run — fm_vh_rank_key, fm_vh_rank, fm_vh_shape_bad, fm_vh_key, fm_vh_code, fm_vh_count,
fm_vh_counter, fm_vh_unit_row (index4j_amd/csrc/fmx_value_hist.hpp), with fm_hit_tile / fm_hit_pattern, fm_line_of over fences and
fm_hist_bucket — compiled for the host and driven by a mirror of the four stages (tests/value_hist_hostsim.cpp, a stand-alone
program: std::stable_sort for the rank sort, std::sort for the key sort, the counters checked against counters incremented hit by
hit), which is additionally built with -fsanitize=address,undefined and run as such, as a program.

The judge is plain numpy over the existing judges (judge_top_hist): Where's kept hits with the span of the edges as its window
(tests/test_field_values_where_cpu.py), the values judge over them (tests/test_field_values_cpu.py), judge_bins
(tests/test_line_histogram_cpu.py) and a stable sort by -count.  The GPU suite runs the kernels and the host forms themselves
(tests/test_gpu_field_values_histogram.py, which shares the helpers below)."""
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import judge_values
from test_field_values_where_cpu import EVERY_LINE, INT32_MAX, Where
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN, judge_bins
from test_match_lines_cpu import judge_n_lines, judge_table

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SIM_SENT, SIM_PAD = -77, 8  # value_hist_hostsim.cpp's kSentinel and kPad
EDGES_4097 = np.arange(4097, dtype=np.int32)  # more edges than a workgroup stages in LDS; the fixture's 2,000 lines fill the first 2,000 buckets


class Hits:
    """packed hits of n patterns that start at slot 0 (what the host form hands the stages: a Where's kept hits), or their first
    n_hits slots only"""

    def __init__(self, kept_off, kept_locs, lens, n_hits=None):
        total = int(kept_off[-1]) if n_hits is None else min(int(n_hits), int(kept_off[-1]))
        self.kept_off = np.minimum(np.asarray(kept_off, np.int64), total)
        self.kept_locs = np.asarray(kept_locs, np.int32)[:total]
        self.lens, self.n = np.asarray(lens, np.int32), len(kept_off) - 1
        self.kept = np.diff(self.kept_off).astype(np.int32)


class TopHist:
    """the judge's answer: the groups (val_off, counts, group_of_hit per kept hit) and the rows made of them"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def strings(self):
        return [self.chars[a:b].tobytes().decode("utf-16-le", "surrogatepass") for a, b in zip(self.text_off[:-1], self.text_off[1:])]

    def rows(self, i=0):
        """[(value, count, per bucket)] of pattern i"""
        s = self.strings()
        return [(s[r], int(self.row_count[r]), self.hist[r].tolist()) for r in range(int(self.row_off[i]), int(self.row_off[i + 1]))]


def hit_groups(values, hits, stop):
    """the group of every hit within its pattern: its window's text up to the first stop unit, looked up among the pattern's values"""
    stop_units = np.unique(ia.as_chars(stop))
    out = np.zeros(len(hits.kept_locs), np.int32)
    for i in range(hits.n):
        index = {v: g for g, (v, _) in enumerate(values.per[i])}
        for t in range(int(hits.kept_off[i]), int(hits.kept_off[i + 1])):
            row = values.rows[t][:int(values.lengths[t])]
            at = np.flatnonzero(np.isin(row, stop_units))
            out[t] = index[tuple(row[:at[0] if len(at) else len(row)].tolist())]
    return out


def judge_top_hist(o, T, hits, edges, top, stop, max_len):
    """by the definition: the values judge over the hits, per pattern a STABLE sort of its groups by -count cut at top, judge_bins
    over the lines of each row's hits and over the lines of the hits of no row.  edges None: one bucket, every line."""
    values = judge_values(o, hits.kept_locs, hits.kept_off, hits.lens, stop, max_len)
    group_of_hit = hit_groups(values, hits, stop)
    bins = np.array([0, INT32_MAX], np.int64) if edges is None else np.asarray(edges, np.int64)
    B = len(bins) - 1
    row_off, row_group, row_count, hist, other, text = [0], [], [], [], [], []
    for i in range(hits.n):
        a, b = int(hits.kept_off[i]), int(hits.kept_off[i + 1])
        counts = values.counts[values.val_off[i]:values.val_off[i + 1]]
        order = np.argsort(-counts.astype(np.int64), kind="stable")[:top]
        L = np.searchsorted(T, hits.kept_locs[a:b], side="left") if edges is not None else np.zeros(b - a, np.int64)
        mine = group_of_hit[a:b]
        for g in order:
            row_group.append(int(g))
            row_count.append(int(counts[g]))
            hist.append(judge_bins(bins, L[mine == g]))
            text.append(values.per[i][g][0])
        other.append(judge_bins(bins, L[~np.isin(mine, order)]))
        row_off.append(len(row_group))
    R = len(row_group)
    return TopHist(n=hits.n, B=B, top=top, val_off=values.val_off, counts=values.counts, group_of_hit=group_of_hit, values=values,
                   n_values=np.diff(values.val_off).astype(np.int32), kept=hits.kept, row_off=np.array(row_off, np.int64),
                   row_group=np.array(row_group, np.int32), row_count=np.array(row_count, np.int32),
                   hist=np.array(hist, np.int32).reshape(R, B), other=np.array(other, np.int32).reshape(hits.n, B),
                   text_off=np.concatenate([[0], np.cumsum([len(v) for v in text])]).astype(np.int64),
                   chars=np.array([u for v in text for u in v], np.uint16))


def span(edges):
    return EVERY_LINE if edges is None else (int(edges[0]), int(edges[-1]))


_JUDGED = {}


def judged(tag, o, T, patterns, queries, where_of, edges, top, stop, max_len):
    """(Where with the span of the edges as its window, the judge's answer over its kept hits), once per case"""
    key = (tag, tuple(patterns), repr(queries), tuple(where_of), None if edges is None else tuple(np.asarray(edges).tolist()), top, stop, max_len)
    if key not in _JUDGED:
        w = Where(tag, o, T, list(patterns), list(queries), list(where_of), span(edges))
        _JUDGED[key] = w, judge_top_hist(o, T, Hits(w.kept_off, w.kept_locs, w.lens), edges, top, stop, max_len)
    return _JUDGED[key]


def check_top_hist(got, want, what):
    """got: a dict under the judge's names (row_off, row_group, row_count, hist, other; text_off and chars where the text came down)"""
    assert (np.asarray(got["row_off"]) == want.row_off).all(), "%s: row_off %r, expected %r" % (what, got["row_off"], want.row_off)
    for name in ("row_group", "row_count", "hist", "other"):
        a, b = np.asarray(got[name]).ravel(), getattr(want, name).ravel()
        assert len(a) == len(b) and (a == b).all(), "%s: %s differs at %r" % (what, name, np.flatnonzero(a[:len(b)] != b[:len(a)])[:5])
    if "chars" in got:
        assert (np.asarray(got["text_off"]) == want.text_off).all() and (np.asarray(got["chars"]) == want.chars).all(), what + ": the rows' text"


def check_invariants(want, hit_hist=None):
    """the sums of the definition, on any answer under the judge's names"""
    assert (want.hist.sum(axis=1) <= want.row_count).all()
    for i in range(want.n):
        a, b = int(want.row_off[i]), int(want.row_off[i + 1])
        assert b - a == min(want.top, int(want.n_values[i]))
        total = want.hist[a:b].sum(axis=0) + want.other[i]
        if hit_hist is not None:
            assert (total == hit_hist[i]).all()
        assert (np.diff(want.row_count[a:b]) <= 0).all()  # descending
        ties = np.flatnonzero(np.diff(want.row_count[a:b]) == 0)
        assert (want.row_group[a:b][ties] < want.row_group[a:b][ties + 1]).all()  # equal counts: the smaller group first


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "value_hist_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "value_hist_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("value_hist_hostsim")


def run_hostsim(simdir, hits, want, T, edges, top, lead=0, extra=0, max_fences=4096, sanitize=False):
    """the stages' mirror over packed hits with `lead` slots in front that hold no hit (hit_off[0] = lead) and `extra` behind; a dict
    under the judge's names.  The groups (val_off, counts, the group of every hit) are the judge's: the values stage has its own mirror."""
    n, total = hits.n, int(hits.kept_off[-1])
    n_hits = lead + total + extra
    edges = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32)
    B = max(len(edges) - 1, 1)
    locs = np.concatenate([np.full(lead, -5, np.int32), hits.kept_locs, np.full(extra, -5, np.int32)]).astype(np.int32)
    groups = np.concatenate([np.full(lead, -1, np.int32), want.group_of_hit, np.full(extra, -1, np.int32)]).astype(np.int32)
    G = int(want.val_off[-1])
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (np.array([n, n_hits, len(T), max_fences, len(edges), top, G], np.int64), np.asarray(T, np.int32), (hits.kept_off + lead).astype(np.int64),
                  locs, edges, want.val_off.astype(np.int64), want.counts.astype(np.int32), groups):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), "run", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.uint8)
    row_off = raw[:(n + 1) * 8].view(np.int64)
    R, at, out = int(row_off[n]), (n + 1) * 8, dict(row_off=row_off)
    for name, count in (("row_group", R), ("row_count", R), ("hist", R * B), ("other", n * B)):
        a = raw[at:at + (count + SIM_PAD) * 4].view(np.int32)
        assert (a[count:] == SIM_SENT).all(), name
        out[name], at = a[:count], at + (count + SIM_PAD) * 4
    out["hist"] = out["hist"].reshape(R, B)
    out["other"] = out["other"].reshape(n, B)
    assert len(raw) == at + (R + 1) * 8
    return out


def sim_case(simdir, tag, o, T, patterns, queries, where_of, edges, top, stop, max_len, what=None, **kw):
    w, want = judged(tag, o, T, patterns, queries, where_of, edges, top, stop, max_len)
    check_top_hist(run_hostsim(simdir, Hits(w.kept_off, w.kept_locs, w.lens), want, T, edges, top, **kw), want, what or "%s %r top %d" % (tag, patterns, top))
    check_invariants(want)
    return w, want


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


def assert_fixture_figures(get):
    """the issue's figures on the fixture (2,000 lines, edges 0, 250, ..., 2000; plain Python string search over the file gives
    them), on whatever get(pattern, stop, top, where) -> TopHist answers: the judge here, the device in the GPU suite"""
    a = get("INFO ", " :", 3, None)
    assert (int(a.kept[0]), int(a.n_values[0])) == (1920, 356)
    assert a.rows() == [("dfs.FSNamesystem", 525, [51, 69, 55, 73, 67, 63, 71, 76]),
                        ("dfs.DataNode$PacketResponder", 480, [82, 19, 75, 41, 56, 67, 73, 67]),
                        ("dfs.DataNode$DataXceiver", 283, [37, 27, 50, 34, 44, 34, 22, 35])]
    assert a.other[0].tolist() == [59, 109, 54, 92, 76, 86, 84, 72] and int(a.other.sum()) == 632
    b = get("INFO ", " :", 3, dict(all=["blk_"], none=["PacketResponder"]))
    assert (int(b.kept[0]), int(b.n_values[0])) == (1317, 248)
    assert b.rows() == [a.rows()[0], a.rows()[2], ("dfs.FSDataset", 221, [0, 55, 5, 43, 28, 29, 38, 23])]
    assert b.other[0].tolist() == [30, 48, 35, 39, 38, 36, 33, 29] and int(b.other.sum()) == 288
    c = get(" from /10.", ".", 5, None)
    assert (int(c.kept[0]), int(c.n_values[0])) == (222, 2)
    assert c.rows() == [("251", 181, [35, 5, 34, 16, 19, 22, 23, 27]), ("250", 41, [7, 1, 6, 4, 6, 8, 5, 4])] and not c.other.any()
    d = get("WARN ", " :", 4, None)
    assert (int(d.kept[0]), int(d.n_values[0])) == (80, 19)
    assert d.rows()[0] == ("dfs.DataNode$DataXceiver", 62, [15, 20, 14, 9, 4, 0, 0, 0])
    assert [r[1] for r in d.rows()[1:]] == [1, 1, 1] and d.row_group[1:].tolist() == sorted(d.row_group[1:].tolist())  # the tie rule
    ones = [g for g in range(19) if g != int(d.row_group[0])]
    assert d.row_group[1:].tolist() == ones[:3]  # the three smallest values of count 1 in code-unit order
    assert d.other[0].tolist() == [4, 5, 2, 1, 3, 0, 0, 0] and int(d.other.sum()) == 15


def fixture_get(simdir, o, T):
    def get(pattern, stop, top, where):
        q = dict(queries=[where], where_of=[0]) if where else dict(queries=[], where_of=[-1])
        w, want = sim_case(simdir, "hd16 top", o, T, [pattern], q["queries"], q["where_of"], EDGES_250, top, stop, 64, lead=3, extra=70)
        return want

    return get


def test_per_item_functions(simdir):
    """the rank key and the slot key at their widest widths, rank = top - 1 / top, the shape's limits, an empty pattern range, the
    counter's decoding, the row of a code unit and one small call: value_hist_hostsim.cpp's self_checks, plain and under
    AddressSanitizer and UBSan"""
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_fixture_figures(simdir, hd):
    """the named figures: the judge gives them, the stages' mirror gives the judge's answer, and a plain string scan of the fixture
    gives the first case's rows"""
    o, T = hd
    assert judge_n_lines(T, len(HD)) == 2000
    assert_fixture_figures(fixture_get(simdir, o, T))
    lines = HD.split("\n")
    for value, per_bucket in (("dfs.FSNamesystem", [51, 69, 55, 73, 67, 63, 71, 76]), ("dfs.DataNode$DataXceiver", [37, 27, 50, 34, 44, 34, 22, 35])):
        scan = [sum(ln.count("INFO " + value + ":") for ln in lines[a:b]) for a, b in zip(EDGES_250[:-1], EDGES_250[1:])]
        assert scan == per_bucket


def test_group_shapes(simdir, hd):
    """G of 0, 1, top - 1, top and top + 1; every hit one value; every hit its own value (the whole selection is the tie rule); ties
    across the cut; top = 1 and top >= G; a pattern without hits between two with hits; under the sanitizers too"""
    o, T = hd
    w, want = sim_case(simdir, "hd16 top", o, T, [" from /10."], [], [-1], EDGES_250, 5, ".", 64)
    assert want.n_values[0] == 2  # G = 2
    for top in (1, 2, 3):  # top - 1, top, top + 1 around G = 2 ... and G = 1 below
        _, t = sim_case(simdir, "hd16 top", o, T, [" from /10."], [], [-1], EDGES_250, top, ".", 64, sanitize=top == 2)
        assert t.row_off[1] == min(top, 2) and (t.other.sum() == 0) == (top >= 2)
    _, one = sim_case(simdir, "hd16 top", o, T, [" from /10.25", "zzzq#", "INFO dfs.FSNamesystem"], [], [-1, -1, -1], EDGES_250, 3, "01:", 64)
    assert one.n_values.tolist() == [1, 0, 1] and one.row_off.tolist() == [0, 1, 1, 2] and one.row_count.tolist() == [222, 525]  # every hit one value
    _, own = sim_case(simdir, "hd16 top", o, T, ["blk_"], [dict(all=["terminating"])], [0], EDGES_250, 7, " \t\r\n", 32, lead=5, extra=1030, sanitize=True)
    assert own.n_values[0] == 310 and own.row_count.tolist() == [1] * 7 and own.row_group.tolist() == list(range(7)) and own.other.sum() == 303
    _, ties = sim_case(simdir, "hd16 top", o, T, ["WARN "], [], [-1], EDGES_250, 4, " :", 64)
    assert ties.row_count.tolist() == [62, 1, 1, 1]
    for top in (1, 19, 20, 65536):
        _, t = sim_case(simdir, "hd16 top", o, T, ["WARN ", "INFO "], [], [-1, -1], EDGES_250, top, " :", 64)
        assert t.row_off.tolist() == [0, min(top, 19), min(top, 19) + min(top, 356)]
        if top >= 356:  # the rows, sorted back by row_group, are the values and their counts; nothing is "other"
            for i in range(2):
                a, b = int(t.row_off[i]), int(t.row_off[i + 1])
                back = np.argsort(t.row_group[a:b])
                assert (t.row_group[a:b][back] == np.arange(b - a)).all() and (t.row_count[a:b][back] == t.counts[t.val_off[i]:t.val_off[i + 1]]).all()
            assert not t.other.any()


def test_edge_shapes_and_packed_blocks(simdir, hd):
    """no edges, uneven edges with empty buckets, edges beyond the line count, 4,097 edges; hits in no bucket (the stage alone: the
    host form's window keeps none); slots in front and behind, few fences, fewer slots than hits at the tile's edges"""
    o, T = hd
    batch = [" ", "blk_", "zzzq#", "", "1"]
    for edges in (None, EDGES_250, EDGES_UNEVEN, EDGES_BEYOND, EDGES_4097):
        _, t = sim_case(simdir, "hd16 top", o, T, batch, [dict(all=["terminating"])], [-1, 0, -1, -1, 0], edges, 6, " \n", 16, lead=7, extra=9, max_fences=3)
        assert (t.hist.sum(axis=1) == t.row_count).all()  # the window is the span: every kept hit has a bucket
        assert t.n_values[2] == 0 and t.row_off[2] == t.row_off[3]
    # the stage over hits that were NOT cut to the span: they are in their row's count and in no counter
    w = Where("hd16 top", o, T, ["INFO ", "WARN "], [], [-1, -1], EVERY_LINE)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    want = judge_top_hist(o, T, hits, EDGES_UNEVEN, 3, " :", 64)
    assert (want.hist.sum(axis=1) < want.row_count).any()
    check_top_hist(run_hostsim(simdir, hits, want, T, EDGES_UNEVEN, 3, lead=2, extra=3, sanitize=True), want, "hits outside the span")
    # fewer slots than hits: 0, 1 and the edges of a tile of 1,024
    for n_hits in (0, 1, 1023, 1024, 1025, 2049):
        cut = Hits(w.kept_off, w.kept_locs, w.lens, n_hits)
        want = judge_top_hist(o, T, cut, EDGES_250, 2, " :", 64)
        assert int(want.kept.sum()) == min(n_hits, 2000)
        check_top_hist(run_hostsim(simdir, cut, want, T, EDGES_250, 2, lead=1 if n_hits else 0, extra=2), want, "%d slots" % n_hits)


def test_error_returns_without_a_device():
    """the checks of the HOST arrays come first: a refused call never reaches the device and stores nothing"""
    import ctypes as C

    fm = ia.FmIndex("k=a k=b k=a\nk=c\n", 4, True, device=None)
    pat, off = ia.pack_patterns([ia.as_chars("k=")])
    off = off.astype(np.int32)
    stop, qoff, kinds, where_of = ia.as_chars(" \n").astype(np.uint16), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.array([-1], np.int32)
    tch, toff = np.zeros(1, np.uint16), np.zeros(1, np.int32)

    def call(top=3, edges=(0, 1, 2), max_len=8, n_stop=2, n=1):
        e = np.asarray(edges, np.int32)
        ints = {k: np.full(4, -9, np.int32) for k in ("n_values", "other", "occurrences", "kept", "status")}
        row_off = np.full(4, -9, np.int64)
        ptrs = [C.c_void_p(0x5A5A) for _ in range(5)]
        rc = ia.lib.fmx_field_values_histogram_where_batch(fm.handle, pat.ctypes.data, off.ctypes.data, n, tch.ctypes.data, toff.ctypes.data, 0, qoff.ctypes.data,
                                                           kinds.ctypes.data, 0, where_of.ctypes.data, e.ctypes.data if len(e) else None, len(e), top,
                                                           stop.ctypes.data, n_stop, max_len, ints["n_values"].ctypes.data, row_off.ctypes.data,
                                                           *(C.byref(p) for p in ptrs), ints["other"].ctypes.data, ints["occurrences"].ctypes.data,
                                                           ints["kept"].ctypes.data, ints["status"].ctypes.data, None)
        untouched = all((a == -9).all() for a in list(ints.values()) + [row_off])
        return rc, untouched, [p.value for p in ptrs], ia.lib.fmx_last_error().decode()

    for kw, word in ((dict(top=0), "top"), (dict(top=65537), "top"), (dict(edges=(0, 2, 1)), "edges"), (dict(edges=(0,)), "edges"),
                     (dict(max_len=65), "max_len"), (dict(n_stop=65), "stop set"), (dict(top=65536, edges=tuple(range(2050))), "2^27")):
        rc, untouched, ptrs, msg = call(**kw)
        assert rc == ia._lib.E_ARG and word in msg and untouched and all(p is None for p in ptrs), (kw, rc, msg, untouched, ptrs)
    rc, untouched, ptrs, msg = call()  # a good call on a handle that is not resident: no CPU fallback
    assert rc == ia._lib.E_NO_DEVICE and untouched and all(p is None for p in ptrs)
    try:
        fm.field_values_histogram("k=", top=0)
        raise AssertionError("top=0 was accepted")
    except ia.FmxError as e:
        assert e.code == ia._lib.E_ARG
    fm.close()

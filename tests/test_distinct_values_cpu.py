"""The distinct values of a field per bucket of lines, dc over time (fmx_values_distinct_histogram_dev,
fmx_distinct_values_histogram_where_batch) on the CPU: the functions the kernels of index4j_amd/csrc/fmx_distinct.hip run — fm_dv_key,
fm_dv_hit_key, fm_dv_is_head, fm_dv_is_first, fm_dv_head_of, fm_dv_counts, fm_dv_shape_bad (index4j_amd/csrc/fmx_distinct.hpp), with
fm_hit_tile / fm_hit_pattern, fm_line_of over fences and fm_hist_bucket — compiled for the host and driven by a mirror of the five
steps (tests/distinct_hostsim.cpp, a stand-alone program: std::stable_sort for the two radix sorts, the counters checked against a set
filled hit by hit), which is additionally built with -fsanitize=address,undefined and run as such, as a program.

Two judges.  judge_distinct is by the definition, over the existing judges: Where's kept hits with the span of the edges as its window
(tests/test_field_values_where_cpu.py), the values judge over them (tests/test_field_values_cpu.py), hit_groups
(tests/test_field_values_histogram_cpu.py), then a set of values per bucket and the smallest bucket of every value.
judge_distinct_slots (tests/distinct_judges.py) is numpy over what the stage takes and so judges made-up hits too; it is held to the
first on the fixture.  The GPU suite runs the kernels and the host forms themselves (tests/test_gpu_distinct_values.py, which shares
the helpers below)."""
import bisect
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from distinct_judges import judge_distinct_slots
from test_field_values_cpu import judge_values
from test_field_values_histogram_cpu import EDGES_4097, Hits, hit_groups, span
from test_field_values_where_cpu import EVERY_LINE, Where
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN
from test_match_lines_cpu import judge_n_lines, judge_table

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SIM_SENT, SIM_PAD = -77, 8  # distinct_hostsim.cpp's kSentinel and kPad
EDGES_EQUAL = np.array([0, 0, 3, 3, 1000, 5000], np.int32)  # empty buckets in front and in the middle, the last edge beyond the lines
EDGES_MIDDLE = np.array([500, 1000, 1500], np.int32)


class Distinct:
    """a judge's answer: distinct and first_seen (n, B), and the groups they were made of"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def judge_distinct(o, T, hits, edges, stop, max_len):
    """by the definition: the values judge over the hits and the group of every hit; per pattern a set of values per bucket, and per
    value the smallest bucket it has a hit in.  A hit whose line lies in no bucket counts nowhere.  edges None: one bucket."""
    values = judge_values(o, hits.kept_locs, hits.kept_off, hits.lens, stop, max_len)
    group_of_hit = hit_groups(values, hits, stop)
    e = None if edges is None else [int(x) for x in edges]
    B = 1 if e is None else len(e) - 1
    distinct, first_seen = np.zeros((hits.n, B), np.int32), np.zeros((hits.n, B), np.int32)
    for i in range(hits.n):
        seen, first = [set() for _ in range(B)], {}
        for t in range(int(hits.kept_off[i]), int(hits.kept_off[i + 1])):
            b = 0
            if e is not None:
                L = int(np.searchsorted(T, hits.kept_locs[t], side="left"))  # a hit belongs to the line of its first character
                b = bisect.bisect_right(e, L) - 1  # edges[b] <= L < edges[b + 1]; of equal edges the last
                if b < 0 or b >= B:
                    continue
            g = int(group_of_hit[t])
            seen[b].add(g)
            first[g] = min(first.get(g, B), b)
        distinct[i] = [len(s) for s in seen]
        for b in first.values():
            first_seen[i, b] += 1
    return Distinct(n=hits.n, B=B, distinct=distinct, first_seen=first_seen, val_off=values.val_off, group_of_hit=group_of_hit,
                    n_values=np.diff(values.val_off).astype(np.int32), kept=hits.kept)


_JUDGED = {}


def judged(tag, o, T, patterns, queries, where_of, edges, stop, max_len):
    """(Where with the span of the edges as its window, the judge's answer over its kept hits), once per case"""
    key = (tag, tuple(patterns), repr(queries), tuple(where_of), None if edges is None else tuple(np.asarray(edges).tolist()), stop, max_len)
    if key not in _JUDGED:
        w = Where(tag, o, T, list(patterns), list(queries), list(where_of), span(edges))
        want = judge_distinct(o, T, Hits(w.kept_off, w.kept_locs, w.lens), edges, stop, max_len)
        want.occurrences = w.occurrences
        for a in (want.distinct, want.first_seen):
            a.setflags(write=False)
        _JUDGED[key] = w, want
    return _JUDGED[key]


def check_distinct(got, want, what):
    """got: a dict with distinct and first_seen"""
    for name in ("distinct", "first_seen"):
        a, b = np.asarray(got[name]).ravel(), getattr(want, name).ravel()
        assert len(a) == len(b) and (a == b).all(), "%s: %s differs at %r: %r, expected %r" % (
            what, name, np.flatnonzero(a[:len(b)] != b[:len(a)])[:5], a[:16], b[:16])


def check_invariants(a, hit_hist=None):
    """what follows from the definition, on any answer with distinct, first_seen and n_values; hit_hist: the hits per bucket"""
    d, f = np.asarray(a.distinct, np.int64), np.asarray(a.first_seen, np.int64)
    assert (f.sum(axis=1) <= a.n_values).all() and (f <= d).all() and (f >= 0).all()
    assert (d.max(axis=1) <= a.n_values).all()
    if hit_hist is not None:  # every kept hit has a bucket
        assert (f.sum(axis=1) == a.n_values).all() and (a.n_values <= d.sum(axis=1)).all()
        assert (d <= hit_hist).all() and ((d == 0) == (np.asarray(hit_hist) == 0)).all()
    if d.shape[1] == 1:
        assert (d[:, 0] == f[:, 0]).all()


def slots_of(hits, want, lead, extra):
    """the packed block the stage gets: `lead` slots in front that hold no hit (hit_off[0] = lead) and `extra` behind, their group -1"""
    locs = np.concatenate([np.full(lead, -5, np.int32), hits.kept_locs, np.full(extra, -5, np.int32)]).astype(np.int32)
    groups = np.concatenate([np.full(lead, -1, np.int32), want.group_of_hit, np.full(extra, -1, np.int32)]).astype(np.int32)
    return (hits.kept_off + lead).astype(np.int64), locs, groups


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "distinct_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "distinct_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("distinct_hostsim")


def run_hostsim_slots(simdir, hit_off, locs, groups, val_off, T, edges, max_fences=4096, sanitize=False):
    """the steps' mirror over a packed block; a dict with distinct and first_seen"""
    n, n_hits = len(hit_off) - 1, len(locs)
    edges = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32)
    B = max(len(edges) - 1, 1)
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (np.array([n, n_hits, len(T), max_fences, len(edges), int(val_off[-1])], np.int64), np.asarray(T, np.int32), np.asarray(hit_off, np.int64),
                  np.asarray(locs, np.int32), edges, np.asarray(val_off, np.int64), np.asarray(groups, np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), "run", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.int32)
    assert len(raw) == 2 * (n * B + SIM_PAD)
    out = {}
    for k, name in enumerate(("distinct", "first_seen")):
        a = raw[k * (n * B + SIM_PAD):(k + 1) * (n * B + SIM_PAD)]
        assert (a[n * B:] == SIM_SENT).all(), name
        out[name] = a[:n * B].reshape(n, B)
    return out


def run_hostsim(simdir, hits, want, T, edges, lead=0, extra=0, **kw):
    """... over a judge's hits and groups (the values stage has its own mirror)"""
    hit_off, locs, groups = slots_of(hits, want, lead, extra)
    return run_hostsim_slots(simdir, hit_off, locs, groups, want.val_off, T, edges, **kw)


def sim_case(simdir, tag, o, T, patterns, queries, where_of, edges, stop, max_len, what=None, lead=3, extra=70, **kw):
    """the judge, the numpy judge over the judge's groups and the steps' mirror: all three agree"""
    w, want = judged(tag, o, T, patterns, queries, where_of, edges, stop, max_len)
    what = what or "%s %r" % (tag, patterns)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    hit_off, locs, groups = slots_of(hits, want, lead, extra)
    d, f = judge_distinct_slots(hit_off, locs, len(locs), groups, want.val_off, T, edges)
    check_distinct(dict(distinct=d, first_seen=f), want, what + ", the numpy judge")
    check_distinct(run_hostsim_slots(simdir, hit_off, locs, groups, want.val_off, T, edges, **kw), want, what + ", the steps' mirror")
    check_invariants(want)
    return w, want


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


FIGURES = (
    # pattern, stop, max_len, where, edges, (occurrences, kept, values), distinct, first_seen; None: not named
    ("blk_", " \t\r\n", 32, None, EDGES_250, (2468, 2468, 2199), [249, 249, 250, 250, 250, 248, 446, 258], [249, 249, 250, 250, 249, 248, 446, 258]),
    ("blk_", " \t\r\n", 32, dict(all=["terminating"]), EDGES_250, (None, 310, 310), [54, 14, 40, 26, 33, 51, 47, 45], [54, 14, 40, 26, 33, 51, 47, 45]),
    ("INFO ", " :", 64, None, EDGES_250, (1920, 1920, 356), [56, 52, 49, 48, 47, 56, 44, 49], [56, 46, 42, 41, 41, 50, 37, 43]),
    ("INFO ", " :", 64, dict(all=["blk_"], none=["PacketResponder"]), EDGES_250, (None, 1317, 248), [29, 45, 35, 38, 36, 36, 33, 30],
     [29, 41, 30, 33, 31, 31, 28, 25]),
    ("INFO ", " :", 64, None, EDGES_EQUAL, (None, None, None), [0, 3, 0, 184, 178], [0, 3, 0, 182, 171]),
    ("INFO ", " :", 64, None, EDGES_MIDDLE, (None, 967, 181), [90, 97], [90, 91]),
    ("INFO ", " :", 64, None, None, (None, None, None), [356], [356]),
    (" from /10.", ".", 64, None, EDGES_250, (None, 222, 2), [2] * 8, [2, 0, 0, 0, 0, 0, 0, 0]),
    ("src: /10.", ".:", 64, None, EDGES_250, (None, 235, 2), [2, 1, 2, 2, 2, 2, 2, 2], [2, 0, 0, 0, 0, 0, 0, 0]),
    ("WARN ", " :", 64, None, EDGES_250, (None, 80, 19), [7, 7, 3, 2, 4, 0, 0, 0], [7, 6, 2, 1, 3, 0, 0, 0]),
    ("size ", " ", 64, None, EDGES_250, (None, 608, 139), [24, 3, 29, 16, 15, 24, 16, 26], [24, 2, 26, 14, 13, 22, 14, 24]),
)


def assert_fixture_figures(get):
    """the issue's figures on the fixture (2,000 lines; plain Python string search over the file gives them), on whatever
    get(pattern, stop, max_len, where, edges) answers with distinct, first_seen, n_values, kept and occurrences of ONE pattern: the judge
    here, the device in the GPU suite"""
    for pattern, stop, max_len, where, edges, (occurrences, kept, values), distinct, first_seen in FIGURES:
        a = get(pattern, stop, max_len, where, edges)
        what = (pattern, where, None if edges is None else len(edges))
        assert np.asarray(a.distinct)[0].tolist() == distinct and np.asarray(a.first_seen)[0].tolist() == first_seen, what
        for got, want in ((a.occurrences, occurrences), (a.kept, kept), (a.n_values, values)):
            assert want is None or int(got[0]) == want, what
    assert sum(FIGURES[0][6]) == 2200 and sum(FIGURES[2][6]) == 401  # (the sums the issue names)


def fixture_get(simdir, o, T):
    def get(pattern, stop, max_len, where, edges):
        q = dict(queries=[where], where_of=[0]) if where else dict(queries=[], where_of=[-1])
        return sim_case(simdir, "hd16 dc", o, T, [pattern], q["queries"], q["where_of"], edges, stop, max_len)[1]

    return get


def test_per_item_functions(simdir):
    """the keys at n * B = 2^27 and G = 2^31 - 1, the head and first rules at j = 0 and across pattern and group borders, the three
    bounds of a counter over an empty bucket, all firsts and no first, the last bucket's key + 1, one small call:
    distinct_hostsim.cpp's self_checks, plain and under AddressSanitizer and UBSan"""
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_fixture_figures(simdir, hd):
    """the named figures: the judge gives them, the numpy judge and the steps' mirror give the judge's answer, and a plain string scan
    of the fixture gives one case's"""
    o, T = hd
    assert judge_n_lines(T, len(HD)) == 2000
    assert_fixture_figures(fixture_get(simdir, o, T))
    lines, seen, distinct, first = HD.split("\n"), set(), [], []
    for a, b in zip(EDGES_250[:-1], EDGES_250[1:]):
        here = {ln[at + 5:].split(" ")[0].split(":")[0] for ln in lines[a:b] for at in range(len(ln)) if ln.startswith("WARN ", at)}
        distinct.append(len(here))
        first.append(len(here - seen))
        seen |= here
    assert distinct == [7, 7, 3, 2, 4, 0, 0, 0] and first == [7, 6, 2, 1, 3, 0, 0, 0] and len(seen) == 19


def test_group_and_edge_shapes(simdir, hd):
    """every hit one value, every hit its own value, a value in every bucket, a pattern without hits between two with hits, the empty
    pattern; no edges, uneven edges with empty buckets, edges beyond the line count, 4,097 edges; few fences; under the sanitizers too"""
    o, T = hd
    _, one = sim_case(simdir, "hd16 dc", o, T, [" from /10.25", "zzzq#", "INFO dfs.FSNamesystem"], [], [-1, -1, -1], EDGES_250, "01:", 64)
    assert one.n_values.tolist() == [1, 0, 1] and (one.distinct[0] == 1).all() and one.first_seen.tolist()[0] == [1, 0, 0, 0, 0, 0, 0, 0] and not one.distinct[1].any()
    _, own = sim_case(simdir, "hd16 dc", o, T, ["blk_"], [dict(all=["terminating"])], [0], EDGES_250, " \t\r\n", 32, lead=5, extra=1030, sanitize=True)
    assert own.n_values[0] == 310 and (own.distinct == own.first_seen).all() and own.distinct.sum() == 310
    batch = [" ", "blk_", "zzzq#", "", "1"]
    for edges in (None, EDGES_250, EDGES_UNEVEN, EDGES_BEYOND, EDGES_4097):
        w, t = sim_case(simdir, "hd16 dc", o, T, batch, [dict(all=["terminating"])], [-1, 0, -1, -1, 0], edges, " \n", 16, lead=7, extra=9, max_fences=3,
                        sanitize=edges is EDGES_UNEVEN)
        assert (t.first_seen.sum(axis=1) == t.n_values).all()  # the window is the span: every kept hit has a bucket
        assert t.n_values[2] == 0 and w.kept[1] > 0 and w.kept[4] > 0
    _, m = sim_case(simdir, "hd16 dc", o, T, ["INFO "], [], [-1], EDGES_4097, " :", 64)
    assert m.distinct.shape == (1, 4096) and m.first_seen.sum() == m.n_values[0]


def test_packed_blocks_and_made_up_hits(simdir, hd):
    """the stage alone over hits outside the span (they count nowhere; a group without a hit in a bucket is no first anywhere); fewer
    slots than hits at the tile's edges with slots in front and behind; slots whose group is -1 or beyond the pattern's groups; G = 0;
    a made-up block against the numpy judge"""
    o, T = hd
    w = Where("hd16 dc", o, T, ["INFO ", "zzzq#", "WARN "], [], [-1, -1, -1], EVERY_LINE)
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    want = judge_distinct(o, T, hits, EDGES_UNEVEN, " :", 64)
    assert (want.first_seen.sum(axis=1) < want.n_values).any()
    check_distinct(run_hostsim(simdir, hits, want, T, EDGES_UNEVEN, lead=2, extra=3, sanitize=True), want, "hits outside the span")
    for n_hits, lead, extra in ((0, 0, 0), (0, 2, 5), (1, 1, 0), (1023, 0, 1), (1024, 3, 0), (1025, 1023, 1025), (3073, 5, 70), (int(w.kept_off[-1]), 1, 1)):
        cut = Hits(w.kept_off, w.kept_locs, w.lens, n_hits)
        want = judge_distinct(o, T, cut, EDGES_250, " :", 64)
        assert int(want.kept.sum()) == min(n_hits, 2000)
        if n_hits + lead + extra:
            check_distinct(run_hostsim(simdir, cut, want, T, EDGES_250, lead, extra), want, "%d slots, %d in front, %d behind" % (n_hits, lead, extra))
    # groups taken away: the numpy judge says what is left
    want = judge_distinct(o, T, hits, EDGES_250, " :", 64)
    hit_off, locs, groups = slots_of(hits, want, 4, 6)
    groups = groups.copy()
    groups[4::3] = -1
    groups[5::7] = 2 ** 31 - 1
    d, f = judge_distinct_slots(hit_off, locs, len(locs), groups, want.val_off, T, EDGES_250)
    assert 0 < d.sum() < want.distinct.sum()
    check_distinct(run_hostsim_slots(simdir, hit_off, locs, groups, want.val_off, T, EDGES_250), Distinct(distinct=d, first_seen=f), "slots without a group")
    # G = 0: a whole call whose hits have no group at all
    none = run_hostsim_slots(simdir, hit_off, locs, np.full(len(locs), -1, np.int32), np.zeros(len(hit_off), np.int64), T, EDGES_250, sanitize=True)
    assert none["distinct"].shape == (3, 8) and not none["distinct"].any() and not none["first_seen"].any()
    hit_off, locs, groups, val_off = made_up_block(5 * 1024 + 1, T)
    for edges in (EDGES_UNEVEN, None):
        d, f = judge_distinct_slots(hit_off, locs, len(locs), groups, val_off, T, edges)
        assert d.sum() > f.sum() > 0 or edges is None
        check_distinct(run_hostsim_slots(simdir, hit_off, locs, groups, val_off, T, edges, sanitize=edges is None), Distinct(distinct=d, first_seen=f), "made-up hits")


def made_up_block(slots, T, n=5, seed=7):
    """a packed block of `slots` slots that needs no index: n patterns, the second without hits, 11 slots in front and 13
    behind; positions anywhere in the text, groups in [-1, G_i] (both ends count nowhere) with G of 1, 40 and thousands"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(11, slots - 13, n - 2))
    hit_off = np.array([11, cuts[0], cuts[0]] + cuts[1:].tolist() + [slots - 13], np.int64)
    G = np.array([1, 40, 7, 3000, 100000], np.int64)[:n]
    val_off = np.concatenate([[0], np.cumsum(G)]).astype(np.int64)
    locs = rng.integers(0, int(T[-1]) + 50, slots).astype(np.int32)
    groups = np.full(slots, -1, np.int32)
    for i in range(n):
        a, b = int(hit_off[i]), int(hit_off[i + 1])
        groups[a:b] = rng.integers(-1, int(G[i]) + 1, b - a)
    return hit_off, locs, groups, val_off


def test_error_returns_without_a_device():
    """the new names are exported; the checks of the HOST arrays come first: a refused call never reaches the device and stores nothing"""
    for name in ("fmx_values_distinct_histogram_scratch_bytes", "fmx_values_distinct_histogram_dev", "fmx_distinct_values_histogram_where_batch",
                 "fmx_distinct_values_histogram_where_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    assert ia.lib.fmx_values_distinct_histogram_scratch_bytes(0, 0, 5, 0) == 0 and ia.lib.fmx_values_distinct_histogram_scratch_bytes(1, 0, 5, 1) == 0
    assert ia.lib.fmx_values_distinct_histogram_scratch_bytes(1, 3, 5, 0) >= 4 * 5 * 8
    fm = ia.FmIndex("k=a k=b k=a\nk=c\n", 4, True, device=None)
    stop, qoff, kinds = ia.as_chars(" \n").astype(np.uint16), np.zeros(1, np.int32), np.zeros(1, np.uint8)
    tch, toff = np.zeros(1, np.uint16), np.zeros(1, np.int32)

    def call(edges=(0, 1, 2), max_len=8, n_stop=2, n=1):
        pat, off = ia.pack_patterns([ia.as_chars("k")] * n)
        pat, off, where_of = np.ascontiguousarray(pat), off.astype(np.int32), np.full(n, -1, np.int32)
        e = np.asarray(edges, np.int32)
        ints = {k: np.full(max(n, 4), -9, np.int32) for k in ("distinct", "first_seen", "n_values", "occurrences", "kept", "status")}
        rc = ia.lib.fmx_distinct_values_histogram_where_batch(fm.handle, pat.ctypes.data, off.ctypes.data, n, tch.ctypes.data, toff.ctypes.data, 0, qoff.ctypes.data,
                                                              kinds.ctypes.data, 0, where_of.ctypes.data, e.ctypes.data if len(e) else None, len(e), stop.ctypes.data,
                                                              n_stop, max_len, ints["distinct"].ctypes.data, ints["first_seen"].ctypes.data,
                                                              ints["n_values"].ctypes.data, ints["occurrences"].ctypes.data, ints["kept"].ctypes.data,
                                                              ints["status"].ctypes.data, None)
        return rc, all((a == -9).all() for a in ints.values()), ia.lib.fmx_last_error().decode()

    for kw, word in ((dict(edges=(0, 2, 1)), "edges"), (dict(edges=(0,)), "edges"), (dict(edges=(-1, 4)), "edge"), (dict(max_len=65), "max_len"),
                     (dict(n_stop=65), "stop set"), (dict(n=65536, edges=tuple(range(2050))), "2^27")):
        rc, untouched, msg = call(**kw)
        assert rc == ia._lib.E_ARG and word in msg and untouched, (kw, rc, msg, untouched)
    rc, untouched, msg = call()  # a good call on a handle that is not resident: no CPU fallback
    assert rc == ia._lib.E_NO_DEVICE and untouched
    with pytest.raises(ia.FmxError) as err:
        fm.distinct_values("k=", edges=[3, 2])
    assert err.value.code == ia._lib.E_ARG
    fm.close()

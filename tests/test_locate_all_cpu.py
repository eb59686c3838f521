""""All occurrences", packed (fmx_locate_all_*; FM:487-552) on the CPU: the functions k_locate_all runs — fm_locate_all_hits,
fm_hit_pattern, fm_locate_all_resolve, fm_locate_hit / fm_rows_hit — compiled for the host and driven by a mirror of the kernel's
tile loop (tests/locate_all_hostsim.cpp), against the oracle, which is the judge of every position, offset, status and of the
LF-step total.  The GPU suite runs the kernels themselves (tests/test_gpu_locate_all.py, which shares the helpers below)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_gpu_locate_rows import run_block_text
from test_locate_rows_cpu import RowsSim, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SENT = -0x3C3C3C3D
ABSENT = 0x7A7B  # a character no text of the suite holds
_SIM = {}


def all_lib(tmpdir):
    if "lib" not in _SIM:
        so = os.path.join(str(tmpdir), "liblocateallhostsim.so")
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "locate_all_hostsim.cpp")])
        L = C.CDLL(so)
        L.sim_locate_all.restype = C.c_int64
        L.sim_locate_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.sim_hit_offsets.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.sim_hit_patterns.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.sim_rows_fill.restype = C.c_int64
        L.sim_win_attach.restype = C.c_int64
        L.sim_set_entry_bytes.argtypes = [C.c_int]
        L.sim_rows_size.restype = C.c_int64
        _SIM["lib"] = L
    return _SIM["lib"]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("locate_all_hostsim")


class AllSim(RowsSim):
    """RowsSim (image, directory forms, row table) over tests/locate_all_hostsim.cpp, which includes rows_hostsim.cpp"""

    def __init__(self, simdir, text, sr):
        self.fm = ia.FmIndex(text, sr, True, device=None)
        self.blob = self.fm.blob()
        self.L = all_lib(simdir)
        self.p = C.c_void_p(self.blob.ctypes.data)
        self.n = int(self.L.sim_rows_size(self.p))
        self.attached = False

    def locate_all(self, rows, ch, off, mm, block=512, grid=3, slice_max=None, first=0, hits=None, out=None, carry=None):
        """the count phase, the packed layout, then k_locate_all's mirror; returns (locs, hit_off, status, lf, tiles that searched hit_off
        where it lies)"""
        counts, st, lf, rng = self.count(ch, off) if carry is None else carry
        n = len(counts)
        hit_off = np.full(n + 1, SENT, np.int64)
        self.L.sim_hit_offsets(ptr(rng), n, int(mm), ptr(hit_off))
        total = int(hit_off[n])
        hits = total if hits is None else hits
        locs = np.full(max(min(hits, max(total - first, 0)), 0) + 8, SENT, np.int32) if out is None else out
        g = self.L.sim_locate_all(self.p, ptr(rows), ptr(rng), ptr(hit_off), n, first, hits, ptr(locs), ptr(lf), ptr(st), block, grid,
                                  int(self.L.sim_locate_all_slice()) if slice_max is None else slice_max)
        return locs, hit_off, st, lf, int(g)


def corner_batch(t16, rng, n_random, heavy=(" ", "1", "0", "INFO"), min_len=1):
    """a batch with the corner cases of the packed layout: the first and the last pattern without hits, 75 consecutive patterns
    without hits (longer than a wave) between two heavy ones, one empty pattern, patterns of exactly one hit, heavy patterns, and
    random substrings (every 7th with a character the text does not hold, met last)"""
    def absent(m=4):
        s = int(rng.integers(0, len(t16) - m - 1))
        p = t16[s:s + m].copy()
        p[0] = ABSENT
        return p

    def random(k):
        out = []
        for j in range(k):
            s, m = int(rng.integers(0, len(t16) - 13)), int(rng.integers(min_len, 13))
            out.append(absent(m) if j % 7 == 3 else t16[s:s + m])
        return out

    hv = [ia.as_chars(h) for h in heavy]
    third = n_random // 3
    long_ones = [t16[s:s + 40] for s in rng.integers(0, len(t16) - 41, 12)]  # (mostly unique: asserted on the oracle below)
    pats = [absent()] + random(third) + [hv[0]] + [absent() for _ in range(75)] + [hv[1]] + random(third) + [np.zeros(0, np.uint16)]
    pats += hv[2:] + long_ones + random(n_random - 2 * third) + [absent()]
    ch, off = ia.pack_patterns(pats)
    return np.ascontiguousarray(ch), off.astype(np.int32)


def assert_corner_cases(counts, status, heavy_min=3):
    """on the ORACLE's answer, before anything else runs"""
    assert counts[0] == 0 and counts[-1] == 0
    assert int((status == 9).sum()) == 1 and (status[status != 9] == 0).all()
    assert (counts == 1).any()
    big = np.sort(counts)[::-1]
    assert (big[:heavy_min] > 1000).all(), big[:5]
    zero = np.concatenate([[0], (counts == 0).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(zero))
    runs = [(a, b) for a, b in zip(edges[0::2], edges[1::2]) if a > 0 and b < len(counts)]  # runs with hits on both sides
    assert max(b - a for a, b in runs) >= 70


_EXPECTED = {}


def expected_packed(key, o, ch, off, mm, threads=16):
    """the oracle's packed answer: locate_batch with loc_cap = the largest count, each row's first found[i] entries concatenated;
    (locs, hit_off, status, LF-steps of the whole call).  Computed once per (key, mm) and never changed."""
    if (key, mm) not in _EXPECTED:
        counts, _ = o.count_batch(ch, off, threads=threads)
        cap = int(counts.max()) if len(counts) else 0
        if mm > 0:
            cap = min(cap, mm)
        orc.counters_reset()
        locs, found, status = o.locate_batch(ch, off, mm, cap, threads=threads, fill=SENT)
        steps = orc.counters()["lf_steps"]
        assert (status[status != 0] == 9).all()
        want = counts if mm <= 0 else np.minimum(counts, mm)
        assert (found == want).all()  # (loc_cap is the largest count: no pattern overruns `locations`)
        hit_off = np.concatenate([[0], np.cumsum(found, dtype=np.int64)]).astype(np.int64)
        keep = np.arange(locs.shape[1])[None, :] < found[:, None] if locs.shape[1] else np.zeros(locs.shape, bool)
        packed = locs[keep]
        assert len(packed) == hit_off[-1] and (packed != SENT).all()
        for a in (packed, hit_off, status):
            a.setflags(write=False)
        _EXPECTED[key, mm] = (packed, hit_off, status, steps, counts)
    return _EXPECTED[key, mm]


def check(res, exp, what, lf_total=True):
    locs, hit_off, st, lf = res[:4]
    packed, ehit, est, esteps = exp[:4]
    assert (hit_off == ehit).all(), what + ": hit_off"
    total = int(ehit[-1])
    bad = np.flatnonzero(locs[:total] != packed)
    assert len(bad) == 0, "%s: %d positions differ, first at hit %r" % (what, len(bad), bad[:5])
    assert (locs[total:] == SENT).all(), what + ": stored beyond hit_off[n]"
    assert (st == est).all(), what + ": status"
    if lf_total:
        assert int(lf.astype(np.int64).sum()) == esteps, what + ": LF-step total"


def test_hit_pattern_skips_runs_of_equal_offsets(simdir):
    """the search alone, on layouts with empty patterns at both ends and in runs, against a plain scan"""
    L = all_lib(simdir)
    rng = np.random.default_rng(1)
    for trial in range(40):
        n = int(rng.integers(1, 300))
        counts = rng.integers(0, 4, n) * (rng.random(n) < 0.3)
        if trial % 3 == 0:
            counts[int(rng.integers(0, n))] = 700
        hit_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total = int(hit_off[-1])
        got = np.full(total + 1, SENT, np.int32)
        L.sim_hit_patterns(ptr(hit_off), n, ptr(got))
        want = np.repeat(np.arange(n), counts.astype(np.int64))
        assert (got[:total] == want).all() and got[total] == SENT


@pytest.mark.parametrize("sr", [4, 32])
def test_fixture_over_tree_directory_forms_and_row_table(simdir, sr):
    t16 = ia.as_chars(HD)
    sim = AllSim(simdir, HD, sr)
    o = orc.OracleFmIndex(HD, sr, True)
    ch, off = corner_batch(t16, np.random.default_rng(sr), 150, min_len=2)
    oc, ost = o.count_batch(ch, off)
    assert_corner_cases(oc, ost)
    tile, slice_full = int(sim.L.sim_locate_all_tile()), int(sim.L.sim_locate_all_slice())
    assert tile % 512 == 0 and tile % 1024 == 0 and slice_full >= 76  # (the run of 75 fits the slice; slice_max below forces the other route)
    rows_tree, replay = sim.fill()
    assert replay == 0
    first = True
    for form in (None, 4, 6, -1, "rows"):
        sim.directory(None if form == "rows" else form)
        rows = rows_tree if form == "rows" else None
        for mm in (-1, 0, 1, 16, 1000) if first else (-1, 16):
            exp = expected_packed(("hd", sr), o, ch, off, mm)
            shapes = ((512, 3, None), (1024, 2, 8)) if (first or mm == 16) else ((512, 7, None),)
            for block, grid, slice_max in shapes:
                res = sim.locate_all(rows, ch, off, mm, block=block, grid=grid, slice_max=slice_max)
                check(res, exp, "sr %d form %r mm %d block %d slice %r" % (sr, form, mm, block, slice_max))
                if slice_max is None:
                    assert res[4] == 0  # every tile's patterns fit the slice the kernel keeps in LDS
        first = False
    sim.directory(None)
    # the route that searches hit_off where it lies was taken where asked for
    res = sim.locate_all(None, ch, off, 1, block=512, grid=3, slice_max=8)
    assert res[4] > 0
    check(res, expected_packed(("hd", sr), o, ch, off, 1), "bounded global search")


def test_paging_tiles_once(simdir):
    """stage 2 in windows: positions equal the one-shot fill, LF-steps and statuses equal it once the windows have tiled the hits"""
    sr = 8
    t16 = ia.as_chars(HD)
    sim = AllSim(simdir, HD, sr)
    o = orc.OracleFmIndex(HD, sr, True)
    ch, off = corner_batch(t16, np.random.default_rng(2), 90)
    exp = expected_packed(("hd", sr, "paging"), o, ch, off, -1)
    total = int(exp[1][-1])
    for w in (63, 4097):
        carry = sim.count(ch, off)
        out = np.full(total + 8, SENT, np.int32)
        for at in range(0, total, w):
            view = out[at:]
            _, hit_off, st, lf, _ = sim.locate_all(None, ch, off, -1, first=at, hits=w, out=view, carry=carry)
        check((out, hit_off, st, lf), exp, "windows of %d" % w)
    carry = sim.count(ch, off)
    out = np.full(total + 8, SENT, np.int32)
    res = sim.locate_all(None, ch, off, -1, first=total - 100, hits=5000, out=out, carry=carry)  # overhangs the end
    assert (out[:100] == exp[0][total - 100:]).all() and (out[100:] == SENT).all()
    out = np.full(8, SENT, np.int32)
    sim.locate_all(None, ch, off, -1, first=total, hits=5, out=out, carry=sim.count(ch, off))  # starts at the end: nothing
    assert (out == SENT).all()


def test_replay_rows_of_the_run_block_text(simdir):
    """every single-symbol pattern without a limit — all rows but the sentinel's, the derailed walks of quirk Q1 and the rows a
    word cannot carry included — with the table and without"""
    text = run_block_text()
    t16 = ia.as_chars(text)
    sim = AllSim(simdir, text, 16)
    o = orc.OracleFmIndex(text, 16, True)
    sim.directory(-1)
    rows, replay = sim.fill()
    assert 0 < replay < sim.n
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in np.unique(t16)])
    off = off.astype(np.int32)
    exp = expected_packed(("runblocks", 16), o, ch, off, -1)
    assert int(exp[1][-1]) == len(t16)  # every row but the sentinel's
    for table in (rows, None):
        check(sim.locate_all(table, ch, off, -1, block=1024, grid=5), exp, "run blocks, table %s" % (table is not None))
    sim.directory(None)


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_locate_all_batch", "fmx_locate_all_ranges_dev", "fmx_locate_all_fill_dev"):
        assert name in ia.SYMBOLS
    fm = ia.FmIndex("This is a long string\0", 4, True, device=None)
    ch, off = ia.pack_patterns(["is", "long"])
    off = off.astype(np.int32)
    hit_off = np.full(3, SENT, np.int64)
    buf = C.c_void_p(0x1234)
    call = ia.lib.fmx_locate_all_batch
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, 2, -1, hit_off.ctypes.data, C.byref(buf), None, None) == E_NO_DEVICE
    assert buf.value is None and (hit_off == SENT).all()  # *locs = NULL on every failure, nothing written
    assert call(None, ch.ctypes.data, off.ctypes.data, 2, -1, hit_off.ctypes.data, C.byref(buf), None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, -1, -1, hit_off.ctypes.data, C.byref(buf), None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, None, 2, -1, hit_off.ctypes.data, C.byref(buf), None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, 2, -1, None, C.byref(buf), None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, 2, -1, hit_off.ctypes.data, None, None, None) == E_ARG
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert call(h, ch.ctypes.data, off.ctypes.data, 2, -1, hit_off.ctypes.data, C.byref(buf), None, None) == E_ARG
        assert ia.lib.fmx_locate_all_ranges_dev(h, None, off.ctypes.data, 2, -1, hit_off.ctypes.data, None, None, off.ctypes.data, None) == E_ARG
        assert ia.lib.fmx_locate_all_fill_dev(h, 2, hit_off.ctypes.data, off.ctypes.data, 0, 1, off.ctypes.data, None, None, None) == E_ARG
    # the device forms: arguments first, then residency
    assert ia.lib.fmx_locate_all_ranges_dev(fm._h, None, off.ctypes.data, 2, -1, hit_off.ctypes.data, None, None, off.ctypes.data, None) == E_NO_DEVICE
    assert ia.lib.fmx_locate_all_ranges_dev(fm._h, None, off.ctypes.data, 2, -1, None, None, None, off.ctypes.data, None) == E_ARG
    assert ia.lib.fmx_locate_all_ranges_dev(fm._h, None, off.ctypes.data, -2, -1, hit_off.ctypes.data, None, None, off.ctypes.data, None) == E_ARG
    assert ia.lib.fmx_locate_all_fill_dev(fm._h, 2, hit_off.ctypes.data, off.ctypes.data, 0, 1, off.ctypes.data, None, None, None) == E_NO_DEVICE
    assert ia.lib.fmx_locate_all_fill_dev(fm._h, 2, hit_off.ctypes.data, off.ctypes.data, -1, 1, off.ctypes.data, None, None, None) == E_ARG
    assert ia.lib.fmx_locate_all_fill_dev(fm._h, 2, hit_off.ctypes.data, off.ctypes.data, 0, -1, off.ctypes.data, None, None, None) == E_ARG
    assert ia.lib.fmx_locate_all_fill_dev(fm._h, 2, None, off.ctypes.data, 0, 1, off.ctypes.data, None, None, None) == E_ARG
    with pytest.raises(IndexError):
        fm.locate_all("")
    with pytest.raises(IndexError):
        fm.locate_all("long", offset=2, length=5)

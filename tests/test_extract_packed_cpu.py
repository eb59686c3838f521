"""Extract, packed (fmx_extract_packed_*, fmx_line_text_batch; FM:564-608) on the CPU: the functions the three kernels of
index4j_amd/csrc/fmx_extract_packed.hip run — fm_extract_packed_status, fm_piece_len / _count / _bounds, fm_seek_at_or_after,
fm_extract_piece, fm_redo_once and the literal fm_extract — compiled for the host and driven by mirrors of the sizes pass, the
fill kernel's tile loop and the redo pass (tests/extract_packed_hostsim.cpp), over the tree and both directory forms.  The oracle
(orc.OracleFmIndex.extract_batch) judges every character, offset and status: the expected packed array is the concatenation of
its rows cut to length.  The GPU suite runs the kernels themselves (tests/test_gpu_extract_packed.py, which shares the helpers
below)."""
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
SENT16 = 0xFFFE  # a noncharacter no test text holds
PAD = 64  # code units behind text_off[n] that must keep the sentinel
ST_NOT_ENABLED, ST_POS_NEGATIVE, ST_STOP_TOO_LONG, ST_AIOOBE = 1, 2, 3, 9
_SIM = {}


def packed_lib(tmpdir, compact=False):
    if compact not in _SIM:
        so = os.path.join(str(tmpdir), "libextractpackedhostsim%s.so" % ("_compact" if compact else ""))
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared"] + (["-DFMX_COMPACT=1"] if compact else []) +
                              ["-o", so, os.path.join(HERE, "extract_packed_hostsim.cpp")])
        L = C.CDLL(so)
        L.sim_win_attach.restype = C.c_int64
        L.sim_set_entry_bytes.argtypes = [C.c_int]
        L.sim_packed_seek.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.sim_packed_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sim_packed_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sim_packed_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        _SIM[compact] = L
    return _SIM[compact]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("extract_packed_hostsim")


class PackedSim(RowsSim):
    """RowsSim's image and directory forms over tests/extract_packed_hostsim.cpp"""

    def __init__(self, simdir, text, sr, extract=True, compact=False):
        if compact:
            assert ia.lib.fmx_set_option(b"image_compact", 1) == 0
        try:
            self.fm = ia.FmIndex(text, sr, extract, device=None)
            self.blob = self.fm.blob()
        finally:
            ia.lib.fmx_set_option(b"image_compact", 0)
        self.L = packed_lib(simdir, compact)
        self.p = C.c_void_p(self.blob.ctypes.data)
        self.attached = False
        self.P = int(self.L.sim_piece_len(self.p))

    def offsets(self, starts, stops):
        n = len(starts)
        text_off, piece_off = np.full(n + 1, SENT, np.int64), np.full(n + 1, SENT, np.int64)
        status = np.full(max(n, 1), SENT, np.int32)
        self.L.sim_packed_offsets(self.p, ptr(starts), ptr(stops), n, ptr(text_off), ptr(piece_off), ptr(status))
        return text_off, piece_off, status[:n]

    def pieces(self, starts, stops, piece_off):
        total = int(piece_off[-1])
        ab, range_of = np.full(2 * total + 2, SENT, np.int32), np.full(total + 1, SENT, np.int32)
        self.L.sim_packed_pieces(self.p, ptr(starts), ptr(stops), len(starts), ptr(piece_off), ptr(ab), ptr(range_of))
        return ab[:2 * total].reshape(total, 2), range_of[:total]

    def packed(self, starts, stops, block=512, grid=3, slice_max=2048):
        """both stages; (chars with PAD sentinels behind, text_off, status, info)"""
        starts, stops = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(stops, np.int32)
        n = len(starts)
        text_off, piece_off, status = self.offsets(starts, stops)
        chars = np.full(int(text_off[n]) + PAD, SENT16, np.uint16)
        redo, flags, info = np.full(n + 4, -1, np.int32), np.full(max(n, 1), -1, np.int32), np.zeros(6, np.int64)
        st = status.copy() if n else np.zeros(1, np.int32)
        self.L.sim_packed_fill(self.p, ptr(starts), ptr(stops), n, ptr(text_off), ptr(piece_off), ptr(chars), ptr(st), ptr(redo), ptr(flags),
                               block, grid, slice_max, ptr(info))
        return chars, text_off, st[:n], info


def piece_len(sr):
    """P: the smallest multiple of the sample rate that is >= 32"""
    return -(-32 // sr) * sr


def corner_ranges(text_len, sr, rng, n_random=150, long_len=5000):
    """the ranges of the issue, for a text of text_len characters (the index's length is text_len + 1): lengths 0, 1, P - 1, P,
    P + 1; start and stop each on a sample, one before it, one after it; a range to the text's last character; the whole text as
    ONE range; 75 consecutive empty ranges (longer than a wave) between two long ones; the first and the last range empty; every
    status; random ranges"""
    P = piece_len(sr)
    L = text_len
    long_len = min(long_len, L // 3)
    rs = [(7, 7)]  # the first range: empty
    for ln in (0, 1, P - 1, P, P + 1):
        for s0 in (0, 3 * P, 3 * P + 1, 5 * sr - 1, int(rng.integers(0, L - P - 2))):
            if s0 + ln <= L:
                rs.append((s0, s0 + ln))
    k = max(2, (L // 2) // sr)
    for da in (-1, 0, 1):
        for db in (-1, 0, 1):
            for span in (0, 1, 3, P // sr + 2):
                a, b = k * sr + da, (k + span) * sr + db
                if 0 <= a and b <= L:
                    rs.append((a, b))
    rs += [(L - min(50, L), L), (L - 1, L), (0, L)]  # to the last character; the whole text
    rs.append((0, long_len))
    rs += [(int(x), int(x)) for x in rng.integers(0, L, 40)] + [(int(x), int(x) - 3) for x in rng.integers(3, L, 35)]  # 75 empty ranges
    rs.append((L - long_len, L))
    rs += [(-1, 5), (-7, -3), (10, L + 1), (10, L + 5), (L, L + 1), (0, -2 ** 31 + 5), (5, -2 ** 31), (0, L), (L, L)]  # statuses (FM's order), then two more
    for _ in range(n_random):
        a = int(rng.integers(0, L))
        rs.append((a, min(L, a + int(rng.integers(0, 4 * P)))))
    rs.append((L // 2, L // 2))  # the last range: empty
    a = np.array(rs, np.int64)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)


_EXPECTED = {}


def expected_packed(key, o, sr, starts, stops, enabled=True, threads=16, small=4096):
    """the oracle's packed answer: extract_batch with dst_len = the longest range (long ranges one by one, so that the oracle's
    rows stay small), each row cut to stop - start — 0 for a range with a status or with stop <= start — and concatenated;
    (chars, text_off, status, LF-steps of all calls).  Computed once per key and never changed.
    One kind of range is not shown to the oracle: FM:580 reads positions[stop / sampleRate + 1], and for a stop so far below 0
    that this index is negative Java throws ArrayIndexOutOfBounds where the oracle's C would read in front of its array.  Such
    a range (past the three checks of FM:566-576) is ST_JAVA_AIOOBE with length 0 by that rule."""
    if key not in _EXPECTED:
        n = len(starts)
        ln = np.maximum(stops.astype(np.int64) - starts, 0)
        status = np.zeros(n, np.int32)
        rows = [None] * n
        orc.counters_reset()
        trunc = -((-stops.astype(np.int64)) // sr)  # Java's stop / sampleRate for stop < 0
        negative_index = enabled & (starts >= 0) & (stops < 0) & (trunc + 1 < 0)
        status[negative_index] = ST_AIOOBE
        for i in np.flatnonzero(negative_index):
            rows[i] = np.zeros(0, np.uint16)
        few = np.flatnonzero((ln <= small) & ~negative_index)
        if len(few):
            dst, _, st = o.extract_batch(starts[few], stops[few], int(ln[few].max()) if len(few) else 0, 0, threads=threads, fill=SENT16)
            status[few] = st
            for j, i in enumerate(few):
                rows[i] = dst[j, :ln[i]]
        for i in np.flatnonzero(ln > small):
            dst, _, st = o.extract_batch(starts[i:i + 1], stops[i:i + 1], int(ln[i]), 0, fill=SENT16)
            status[i] = st[0]
            rows[i] = dst[0]
        steps = orc.counters()["lf_steps"]
        early = np.isin(status, (ST_NOT_ENABLED, ST_POS_NEGATIVE, ST_STOP_TOO_LONG))
        for i in np.flatnonzero(early):
            rows[i] = rows[i][:0]  # (a range FM:566-576 turn away has length 0)
        text_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        chars = np.concatenate(rows) if n else np.zeros(0, np.uint16)
        for a in (chars, text_off, status):
            a.setflags(write=False)
        _EXPECTED[key] = (chars, text_off, status, steps)
    return _EXPECTED[key]


def check(res, exp, what):
    chars, text_off, status = res[:3]
    echars, eoff, est = exp[:3]
    assert (text_off == eoff).all(), what + ": text_off"
    assert (status == est).all(), "%s: status differs at %r" % (what, np.flatnonzero(status != est)[:5])
    total = int(eoff[-1])
    bad = np.flatnonzero(chars[:total] != echars)
    assert len(bad) == 0, "%s: %d characters differ, first at %r" % (what, len(bad), bad[:5])
    assert len(chars) > total and (chars[total:] == SENT16).all(), what + ": stored behind text_off[n]"


def assert_corner_cases(starts, stops, status, sr, L):
    """on the ORACLE's answer, before anything else runs"""
    P = piece_len(sr)
    ln = np.where(status == 0, np.maximum(stops.astype(np.int64) - starts, 0), 0)
    assert ln[0] == 0 and ln[-1] == 0
    assert {0, 1, P - 1, P, P + 1} <= set(ln.tolist())
    assert ((stops == L) & (ln > 0)).any() and ((starts == 0) & (stops == L)).any()
    assert -(-L // P) > 1024 or L < 1024 * P  # (the whole text crosses tiles where the text is long enough)
    seen = [s for s in status.tolist() if s]
    assert set(seen) == {ST_POS_NEGATIVE, ST_STOP_TOO_LONG, ST_AIOOBE}
    zero = np.concatenate([[0], (ln == 0).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(zero))
    runs = [(a, b) for a, b in zip(edges[0::2], edges[1::2]) if a > 0 and b < len(ln)]
    assert max(b - a for a, b in runs) >= 75
    for v, where in ((starts, "start"), (stops, "stop")):
        m = v[(status == 0) & (ln > 0)] % sr
        assert sr == 1 or {0, 1 % sr, sr - 1} <= set(m.tolist()), where


# ---- the geometry alone ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [1, 4, 5, 32, 33, 64, 100])
def test_pieces_tile_every_range_and_end_on_samples(simdir, sr):
    text = HD[:20000]
    sim = PackedSim(simdir, text, sr)
    P = piece_len(sr)
    assert sim.P == P and P % sr == 0 and P >= 32 and P - sr < 32
    starts, stops = corner_ranges(len(text), sr, np.random.default_rng(sr))
    text_off, piece_off, status = sim.offsets(starts, stops)
    ln = np.where(status == 0, np.maximum(stops.astype(np.int64) - starts, 0), 0)
    assert text_off[0] == 0 and (np.diff(text_off) == ln).all() and piece_off[0] == 0
    ab, range_of = sim.pieces(starts, stops, piece_off)
    assert (np.repeat(np.arange(len(starts)), np.diff(piece_off)) == range_of).all()
    for r in np.flatnonzero(ln > 0):
        mine = ab[piece_off[r]:piece_off[r + 1]]
        assert mine[0, 0] == starts[r] and mine[-1, 1] == stops[r]
        assert (mine[1:, 0] == mine[:-1, 1]).all()  # one after the other
        assert (mine[:-1, 1] % P == 0).all()  # every piece but the last ends on a multiple of P: on a sample
        assert (mine[:, 1] > mine[:, 0]).all() and (mine[:, 1] - mine[:, 0] <= P).all()
    assert (np.diff(piece_off)[ln == 0] == 0).all()


@pytest.mark.parametrize("sr,text_len", [(1, 300), (4, 4095), (4, 4096), (32, 4095), (32, 4096), (32, 4107), (64, 4095), (64, 4100), (7, 700)])
def test_seek_at_or_after_lands_where_seek_after_does(simdir, sr, text_len):
    """the index's length (text + terminator) a multiple of the sample rate, and not: from the sample AT or after x, `skip` clean
    steps lead to the very row the reference's seek leads to — with skip 0 on a sample and never a whole interval"""
    sim = PackedSim(simdir, HD[:text_len], sr)
    length = text_len + 1
    out = np.zeros(6, np.int32)
    for x in range(0, length):  # every stop FM:574-576 let through
        sim.L.sim_packed_seek(sim.p, x, ptr(out))
        at_row, at_skip, ref_row, ref_skip, at_end, ref_end = out.tolist()
        assert 0 <= at_skip < sr and at_skip <= length - x, x
        assert at_skip == min((-x) % sr, length - x), x
        assert (at_skip == 0) == (x % sr == 0), x
        assert ref_skip == at_skip + (sr if x % sr == 0 and x + sr <= length else (length - x if x % sr == 0 else 0)), x
        assert at_end == ref_end and at_end >= 0, x


# ---- the three passes against the oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [1, 4, 32, 64])
def test_fixture_over_tree_and_directory_forms(simdir, sr):
    t16 = ia.as_chars(HD)
    L = len(t16)
    sim = PackedSim(simdir, HD, sr)
    o = orc.OracleFmIndex(HD, sr, True)
    starts, stops = corner_ranges(L, sr, np.random.default_rng(100 + sr))
    exp = expected_packed(("hd", sr), o, sr, starts, stops)
    assert_corner_cases(starts, stops, exp[2], sr, L)
    whole = t16  # what the text itself holds (the fixture has no quirk rows: asserted by the empty redo list)
    i = int(np.flatnonzero((starts == 0) & (stops == L))[0])
    assert (exp[0][exp[1][i]:exp[1][i + 1]] == whole).all()
    first = True
    for form in (None, 4, 6, -1):
        sim.directory(form)
        for block, grid, slice_max in (((512, 3, 2048), (1024, 2, 8), (512, 7, 2048)) if first else ((1024, 5, 2048),)):
            res = sim.packed(starts, stops, block=block, grid=grid, slice_max=slice_max)
            what = "sr %d form %r block %d grid %d slice %d" % (sr, form, block, grid, slice_max)
            check(res, exp, what)
            info = res[3]
            assert info[0] == 0 and info[4] == 0, what  # a clean index: nothing is redone
            assert info[3] <= sim.P + sr, what  # no chain longer than a piece and one sample interval
            assert info[2] == exp[3], what  # the reference's LF-steps in total: each range's trailing skip is paid once
            assert (info[1] > 0) == (slice_max == 8), what
            if grid <= 3:
                assert info[5] >= 3 * grid, what  # (every workgroup's tile loop ran three times at least)
        first = False
    sim.directory(None)


@pytest.mark.parametrize("sr,text_len", [(32, 4095), (32, 4107), (4, 4095), (4, 4098), (64, 8191), (64, 8200)])
def test_length_a_multiple_of_the_sample_rate_and_not(simdir, sr, text_len):
    text = HD[:text_len]
    sim = PackedSim(simdir, text, sr)
    o = orc.OracleFmIndex(text, sr, True)
    starts, stops = corner_ranges(text_len, sr, np.random.default_rng(text_len), n_random=60)
    exp = expected_packed(("cut", sr, text_len), o, sr, starts, stops)
    for form in (None, 6, -1):
        sim.directory(form)
        res = sim.packed(starts, stops, block=512, grid=2)
        check(res, exp, "sr %d length %d form %r" % (sr, text_len + 1, form))
        assert res[3][0] == 0
    sim.directory(None)


def test_compact_image(simdir):
    sr = 32
    L = len(ia.as_chars(HD))
    sim = PackedSim(simdir, HD, sr, compact=True)
    o = orc.OracleFmIndex(HD, sr, True)
    starts, stops = corner_ranges(L, sr, np.random.default_rng(100 + sr))
    exp = expected_packed(("hd", sr), o, sr, starts, stops)
    for form in (None, -1):
        sim.directory(form)
        check(sim.packed(starts, stops, block=1024, grid=3), exp, "compact, form %r" % form)
    sim.directory(None)


def test_extract_not_enabled_and_empty_batch(simdir):
    sim = PackedSim(simdir, HD[:5000], 8, extract=False)
    o = orc.OracleFmIndex(HD[:5000], 8, False)
    starts, stops = corner_ranges(5000, 8, np.random.default_rng(3), n_random=20)
    exp = expected_packed(("off", 8), o, 8, starts, stops, enabled=False)
    assert (exp[2] == ST_NOT_ENABLED).all() and exp[1][-1] == 0  # the first check of FM:566-576 wins over every other
    check(sim.packed(starts, stops), exp, "enableExtract = false")
    sim = PackedSim(simdir, HD[:5000], 8)
    chars, text_off, status, info = sim.packed(np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert text_off.tolist() == [0] and len(status) == 0 and (chars == SENT16).all() and info[5] == 0


def run_block_ranges(text_len, sr, rng):
    """ranges over the run-block text: the corner cases, and ranges inside and across the runs of wide symbols, where quirk Q1
    derails the reference's walks"""
    starts, stops = corner_ranges(text_len, sr, rng, n_random=80, long_len=3000)
    a = rng.integers(0, text_len - 400, 200)
    b = a + rng.integers(1, 400, 200)
    return (np.concatenate([starts[:-1], a.astype(np.int32), starts[-1:]]),  # (the last range stays the empty one)
            np.concatenate([stops[:-1], b.astype(np.int32), stops[-1:]]))


@pytest.mark.parametrize("sr", [16, 5])
def test_quirk_rows_are_redone_literally(simdir, sr):
    """the run-block text (quirk Q1): pieces that meet a step that is not clean put their range on the redo list, once, and the
    literal walk's characters — which are NOT the text's — are what the oracle returns"""
    text = run_block_text()
    t16 = ia.as_chars(text)
    L = len(t16)
    sim = PackedSim(simdir, text, sr)
    o = orc.OracleFmIndex(text, sr, True)
    starts, stops = run_block_ranges(L, sr, np.random.default_rng(sr))
    exp = expected_packed(("runblocks", sr), o, sr, starts, stops)
    i = int(np.flatnonzero((starts == 0) & (stops == L))[0])
    assert (exp[0][exp[1][i]:exp[1][i + 1]] != t16).any()  # the reference's own answer differs from the text here
    for form in (None, -1, 4):
        sim.directory(form)
        res = sim.packed(starts, stops, block=1024, grid=5)
        check(res, exp, "run blocks, form %r" % form)
        n_redo = int(res[3][0])
        assert 0 < n_redo < len(starts), n_redo
    sim.directory(None)


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    names = ("fmx_extract_packed_batch", "fmx_line_text_batch", "fmx_extract_packed_scratch_bytes", "fmx_extract_packed_offsets_dev",
             "fmx_extract_packed_fill_dev", "fmx_extract_packed_last_redo")
    for name in names:
        assert name in ia.SYMBOLS
    fm = ia.FmIndex("This is a long string\0", 4, True, device=None)
    a, b = np.array([0, 5], np.int32), np.array([4, 7], np.int32)
    text_off = np.full(3, SENT, np.int64)
    buf = C.c_void_p(0x1234)
    call = ia.lib.fmx_extract_packed_batch
    assert call(fm._h, a.ctypes.data, b.ctypes.data, 2, text_off.ctypes.data, C.byref(buf), None) == E_NO_DEVICE
    assert buf.value is None and (text_off == SENT).all()  # *chars = NULL on every failure, nothing written
    assert call(None, a.ctypes.data, b.ctypes.data, 2, text_off.ctypes.data, C.byref(buf), None) == E_ARG
    assert call(fm._h, a.ctypes.data, b.ctypes.data, -1, text_off.ctypes.data, C.byref(buf), None) == E_ARG
    assert call(fm._h, None, b.ctypes.data, 2, text_off.ctypes.data, C.byref(buf), None) == E_ARG
    assert call(fm._h, a.ctypes.data, b.ctypes.data, 2, None, C.byref(buf), None) == E_ARG
    assert call(fm._h, a.ctypes.data, b.ctypes.data, 2, text_off.ctypes.data, None, None) == E_ARG
    lines = ia.lib.fmx_line_text_batch
    assert lines(fm._h, a.ctypes.data, 2, text_off.ctypes.data, C.byref(buf), None) == E_NO_DEVICE
    assert lines(fm._h, None, 2, text_off.ctypes.data, C.byref(buf), None) == E_ARG
    nbytes = C.c_size_t(0)
    assert ia.lib.fmx_extract_packed_scratch_bytes(fm._h, 1000, C.byref(nbytes)) == 0 and nbytes.value >= 2 * 8 * 1001 + 2 * 4 * 1000
    assert ia.lib.fmx_extract_packed_scratch_bytes(fm._h, -1, C.byref(nbytes)) == E_ARG
    assert ia.lib.fmx_extract_packed_scratch_bytes(fm._h, 1, None) == E_ARG
    p = a.ctypes.data  # (any non-null pointer: the arguments are judged before anything is touched)
    off = ia.lib.fmx_extract_packed_offsets_dev
    fill = ia.lib.fmx_extract_packed_fill_dev
    assert off(fm._h, p, p, 2, p, p, p, p, nbytes.value, None) == E_NO_DEVICE
    assert off(fm._h, p, p, -2, p, p, p, p, nbytes.value, None) == E_ARG
    assert off(fm._h, None, p, 2, p, p, p, p, nbytes.value, None) == E_ARG
    assert off(fm._h, p, p, 2, None, p, p, p, nbytes.value, None) == E_ARG
    assert fill(fm._h, p, p, 2, p, p, p, p, p, nbytes.value, None) == E_NO_DEVICE
    assert fill(fm._h, p, p, 2, p, p, None, p, p, nbytes.value, None) == E_ARG
    assert fill(fm._h, p, p, 2, p, None, p, p, p, nbytes.value, None) == E_ARG
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert call(h, a.ctypes.data, b.ctypes.data, 2, text_off.ctypes.data, C.byref(buf), None) == E_ARG
        assert lines(h, a.ctypes.data, 2, text_off.ctypes.data, C.byref(buf), None) == E_ARG
        assert off(h, p, p, 2, p, p, p, p, nbytes.value, None) == E_ARG
        assert fill(h, p, p, 2, p, p, p, p, p, nbytes.value, None) == E_ARG
    with pytest.raises(ValueError):
        fm.extract_packed_batch([0, 1], [2])
    with pytest.raises(ValueError):
        fm.grep("is", all=["long"])


def test_host_simulation_is_sanitizer_clean(tmp_path):
    """tests/cpp/san_extract_packed.cpp: the host simulation as a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer, every array exactly as large as the contract makes it"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "index4j_amd", "csrc")
    exe = str(tmp_path / "san_extract_packed")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + csrc, "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "san_extract_packed.cpp")]
    cmd += [os.path.join(csrc, f) for f in ("fmx_build.cpp", "fmx_serial.cpp", "fmx_blob.cpp", "fmx_synth.cpp")]
    cmd += ["-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.count(" ok: ") == 8

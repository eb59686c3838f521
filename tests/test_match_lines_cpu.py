"""The lines that match (fmx_line_table_build, fmx_lines_of_hits_dev, fmx_match_lines_batch) on the CPU: the functions the kernels of
fmx_hit_lines.hip run — fm_line_of over its fences, fm_line_total, fm_line_bounds, the key pack / unpack, fm_line_head — compiled
for the host and driven by a mirror of the stages (tests/match_lines_hostsim.cpp; the device-wide sort = std::sort).

The judge is the oracle plus numpy, never the code under test: T = the oracle's locate() of the boundary, sorted; the lines of a
pattern = np.unique(np.searchsorted(T, the oracle's hits, "left")).  The GPU suite (tests/test_gpu_match_lines.py) shares the
helpers below."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_locate_all_cpu import SENT, assert_corner_cases, corner_batch, expected_packed

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
INT32_MAX = 2**31 - 1
MAX_LINES = (0, -1, 1, 16, 5000)
_SIM = {}


def ptr(a):
    return C.c_void_p(a.ctypes.data)


# ---- the judge -------------------------------------------------------------------------------------------------------------
def judge_table(o, boundary):
    """T: what the oracle's locate(new char[]{boundary}, locations) returns, sorted ascending"""
    b = np.array([boundary if isinstance(boundary, (int, np.integer)) else ord(boundary)], np.uint16)
    k = o.count(b)
    n, locs = o.locate(b, max_matches=-1, cap=k + 1)
    assert n == k
    return np.sort(locs).astype(np.int32)


def judge_lines(T, packed, hit_off, max_lines):
    """(lines, line_off, line_count) of a batch from the oracle's packed hits (test_locate_all_cpu.expected_packed)"""
    per = [np.unique(np.searchsorted(T, packed[hit_off[i]:hit_off[i + 1]], side="left")) for i in range(len(hit_off) - 1)]
    line_count = np.array([len(u) for u in per], np.int32)
    kept = [u[:max_lines] if max_lines > 0 else u for u in per]
    line_off = np.concatenate([[0], np.cumsum([len(u) for u in kept])]).astype(np.int64)
    lines = np.concatenate(kept).astype(np.int32) if kept and line_off[-1] else np.zeros(0, np.int32)
    return lines, line_off, line_count


def judge_n_lines(T, text_len):
    return len(T) + (1 if text_len > 0 and not np.isin(text_len - 1, T) else 0)


def judge_bounds(T, n_lines, text_len, ids):
    start, stop = np.full(len(ids), -1, np.int32), np.full(len(ids), -1, np.int32)
    for j, k in enumerate(ids):
        if 0 <= k < n_lines:
            start[j] = 0 if k == 0 else T[k - 1] + 1
            stop[j] = T[k] if k < len(T) else text_len
    return start, stop


def with_boundary_patterns(t16, ch, off, T, boundary, more=()):
    """the batch + a pattern that starts at a boundary position, one that ends in the boundary, and the boundary itself (+ `more`)"""
    pats = [ch[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    s = int(T[len(T) // 2])
    assert t16[s] == boundary and s + 6 < len(t16)
    extra = [t16[s:s + 6], t16[s - 5:s + 1], np.array([boundary], np.uint16)] + [ia.as_chars(m) for m in more]
    ch2, off2 = ia.pack_patterns(pats[:-1] + extra + pats[-1:])  # (the last pattern stays one without hits)
    return np.ascontiguousarray(ch2), off2.astype(np.int32)


def check_lines(got, exp, what, tail=None):
    lines, line_off, line_count = got
    elines, eoff, ecount = exp
    assert (line_off == eoff).all(), what + ": line_off"
    assert (line_count == ecount).all(), what + ": line_count"
    total = int(eoff[-1])
    bad = np.flatnonzero(lines[:total] != elines)
    assert len(bad) == 0, "%s: %d line ids differ, first at %r" % (what, len(bad), bad[:5])
    if tail is not None:
        assert (lines[total:] == tail).all(), what + ": stored beyond line_off[n]"


# ---- the host build --------------------------------------------------------------------------------------------------------
def sim_lib(tmpdir):
    if "lib" not in _SIM:
        so = os.path.join(str(tmpdir), "libmatchlineshostsim.so")
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "match_lines_hostsim.cpp")])
        L = C.CDLL(so)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.sim_line_of.argtypes = [vp, i32, i32, vp, i32, vp, vp]
        L.sim_line_total.restype = i64
        L.sim_line_total.argtypes = [vp, i32, i32]
        L.sim_line_bounds.argtypes = [vp, i32, i64, i32, vp, i32, vp, vp]
        L.sim_bits.argtypes = [C.c_uint32]
        L.sim_lines_of_hits.argtypes = [vp, i32, i32, i32, vp, vp, i64, i32, vp, vp, vp]
        _SIM["lib"] = L
    return _SIM["lib"]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return sim_lib(tmp_path_factory.mktemp("match_lines_hostsim"))


def fence_depths(count):
    """max_fences from "no fences" over every shift the table can take to "more fences than entries\""""
    out = [0, 1, 2, 3, 5]
    s = 0
    while (count >> s) > 0:
        out.append(max((count + (1 << s) - 1) >> s, 1))
        s += 1
    return sorted(set(out + [count, count + 1, count + 9, 4096]))


def probe_positions(T, n):
    ps = [-1, 0, n - 1, n, INT32_MAX, -INT32_MAX - 1]
    t = T.astype(np.int64)
    return np.unique(np.clip(np.concatenate([ps, t, t - 1, t + 1]), -INT32_MAX - 1, INT32_MAX)).astype(np.int32)


def sim_lines(L, T, fences, hit_off, packed, n_hits, max_lines, pad=8):
    n = len(hit_off) - 1
    T_ = np.ascontiguousarray(T if len(T) else np.zeros(1, np.int32))
    locs = np.concatenate([packed, np.full(max(n_hits - len(packed), 0) + 1, SENT, np.int32)]).astype(np.int32)
    line_off = np.full(n + 1, SENT, np.int64)
    lines = np.full(n_hits + pad, SENT, np.int32)
    line_count = np.full(max(n, 1), SENT, np.int32)
    bits = L.sim_lines_of_hits(ptr(T_), len(T), fences, n, ptr(np.ascontiguousarray(hit_off)), ptr(locs), n_hits, max_lines, ptr(line_off), ptr(lines),
                               ptr(line_count))
    return (lines, line_off, line_count[:n]), bits


def texts():
    small = lambda s: (s, "\n")
    no_boundary = "".join(chr(97 + (i * 7) % 5) for i in range(300))
    return {
        "hdfs": (HD, "\n"),
        "hdfs, last line unterminated": (HD[:-10], "\n"),
        "empty lines": small("a\n\nb\n\n\nab"),
        "boundary at both ends": small("\nab\n"),
        "no boundary": (no_boundary, "\n"),
    }


def batch_for(name, text, t16, T, boundary):
    if name.startswith("hdfs"):
        ch, off = corner_batch(t16, np.random.default_rng(5), 150, min_len=2)
        return with_boundary_patterns(t16, ch, off, T, ord(boundary))
    pats = [np.array([0x7A7B], np.uint16)] + [np.array([s], np.uint16) for s in np.unique(t16)]
    pats += [ia.as_chars(p) for p in ("ab", "a\n", "\nb", "\n\n", "\na", "b\n\n\na", "bca", "zz")] + [np.zeros(0, np.uint16), np.array([0x7A7B], np.uint16)]
    ch, off = ia.pack_patterns(pats)
    return np.ascontiguousarray(ch), off.astype(np.int32)


@pytest.mark.parametrize("name", list(texts()))
def test_line_functions_and_stages_against_the_judge(L, name):
    text, boundary = texts()[name]
    t16 = ia.as_chars(text)
    n = len(t16)
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, boundary)
    truth = np.flatnonzero(t16 == ord(boundary)).astype(np.int32)
    assert (T == truth).all()  # (none of these texts derails a walk: the oracle's table is the text's)
    if name == "no boundary":
        assert len(T) == 0
    T_ = np.ascontiguousarray(T if len(T) else np.zeros(1, np.int32))
    # fm_line_of at every fence depth
    ps = probe_positions(T, n)
    want = np.searchsorted(T, ps, side="left").astype(np.int32)
    seen_shifts = set()
    for fences in fence_depths(len(T)):
        got = np.full(len(ps), SENT, np.int32)
        nf = C.c_int32(-1)
        shift = L.sim_line_of(ptr(T_), len(T), fences, ptr(ps), len(ps), ptr(got), C.byref(nf))
        assert (got == want).all(), "%s: line() with at most %d fences (shift %d)" % (name, fences, shift)
        assert nf.value <= max(fences, 0) and (nf.value == 0 or (nf.value - 1) << shift < len(T))
        if fences > len(T) > 0:
            assert shift == 0 and nf.value == len(T)  # more fences than entries: every level in the fences
        seen_shifts.add((shift, nf.value > 0))
    if len(T) > 64:
        assert len(seen_shifts) > 8
    # the lines of the text, and their bounds
    n_lines = judge_n_lines(T, n)
    assert n_lines == len(text.split(boundary)) - (1 if text.endswith(boundary) else 0)
    assert L.sim_line_total(ptr(T_), len(T), n) == n_lines
    assert L.sim_line_total(ptr(T_), len(T), 0) == len(T)
    ids = np.concatenate([[-1, n_lines, n_lines + 1, INT32_MAX, -INT32_MAX - 1], np.arange(n_lines)]).astype(np.int32)
    start, stop = np.full(len(ids), SENT, np.int32), np.full(len(ids), SENT, np.int32)
    L.sim_line_bounds(ptr(T_), len(T), n_lines, n, ptr(ids), len(ids), ptr(start), ptr(stop))
    es, ee = judge_bounds(T, n_lines, n, ids)
    assert (start == es).all() and (stop == ee).all()
    assert [text[a:b] for a, b in zip(start[5:], stop[5:])] == text.split(boundary)[:n_lines]
    # the stages over the oracle's packed hits
    ch, off = batch_for(name, text, t16, T, boundary)
    packed, hit_off, status, _, counts = expected_packed(("match lines cpu", name), o, ch, off, -1)
    if name.startswith("hdfs"):
        assert_corner_cases(counts, status)
    assert (status == 9).sum() == 1 and counts[0] == 0 and counts[-1] == 0
    total = int(hit_off[-1])
    for max_lines in MAX_LINES:
        exp = judge_lines(T, packed, hit_off, max_lines)
        if max_lines <= 0 and name.startswith("hdfs"):
            assert (exp[2] < np.diff(hit_off)).any()  # a pattern with two hits on one line
        for fences, n_hits in ((4096, total), (0, total), (3, total + 37)):
            got, bits = sim_lines(L, T, fences, hit_off, packed, n_hits, max_lines)
            assert bits == L.sim_bits(len(off) - 1) + L.sim_bits(len(T)) <= 62
            check_lines(got, exp, "%s max_lines %d fences %d n_hits %d" % (name, max_lines, fences, n_hits), tail=SENT)
    if name == "no boundary":
        assert (judge_lines(T, packed, hit_off, 0)[0] == 0).all()  # every hit is on line 0


def test_a_hit_belongs_to_the_line_of_its_first_character(L):
    """patterns that hold the boundary, and the boundary itself, on the hand-made text"""
    text = "a\n\nb\n\n\nab"
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    assert list(T) == [1, 2, 4, 5, 6]
    ch, off = ia.pack_patterns(["\n", "a\n", "\nb", "\n\n", "ab", "a", "b"])
    off = off.astype(np.int32)
    packed, hit_off = expected_packed(("first char", 0), o, ch, off, -1)[:2]
    lines, line_off, line_count = sim_lines(L, T, 4096, hit_off, packed, int(hit_off[-1]), 0)[0]
    per = [list(lines[line_off[i]:line_off[i + 1]]) for i in range(len(off) - 1)]
    #        "\n": a boundary at T[k] is on line k;  "a\n" line 0;  "\nb" starts at 2: line 1;  "\n\n" at 1, 4, 5
    assert per == [[0, 1, 2, 3, 4], [0], [1], [0, 2, 3], [5], [0, 5], [2, 5]]
    assert list(line_count) == [5, 1, 1, 3, 1, 2, 2]


def test_bits_and_keys(L):
    for v, b in ((0, 1), (1, 1), (2, 2), (3, 2), (4, 3), (2000, 11), (2**31 - 1, 31), (2**31, 32)):
        assert L.sim_bits(v) == b


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    names = ("fmx_line_table_build", "fmx_line_table_info", "fmx_line_bounds_batch", "fmx_line_bounds_batch_dev", "fmx_lines_of_hits_scratch_bytes",
             "fmx_lines_of_hits_dev", "fmx_match_lines_batch")
    for name in names:
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("This is a long string\n", 4, True, device=None)
    assert fm.line_table_info() == (-1, 0, 0)
    n_lines = C.c_int64(SENT)
    assert ia.lib.fmx_line_table_build(fm._h, 10, C.byref(n_lines)) == E_NO_DEVICE and n_lines.value == SENT
    assert ia.lib.fmx_line_table_build(None, 10, C.byref(n_lines)) == E_ARG
    ch, off = ia.pack_patterns(["is", "long"])
    off = off.astype(np.int32)
    line_off = np.full(3, SENT, np.int64)
    buf = C.c_void_p(0x1234)
    call = ia.lib.fmx_match_lines_batch
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, 2, 0, line_off.ctypes.data, C.byref(buf), None, None, None) == E_NO_DEVICE
    assert buf.value is None and (line_off == SENT).all()  # *lines = NULL on every failure, nothing written
    assert call(None, ch.ctypes.data, off.ctypes.data, 2, 0, line_off.ctypes.data, C.byref(buf), None, None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, -1, 0, line_off.ctypes.data, C.byref(buf), None, None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, None, 2, 0, line_off.ctypes.data, C.byref(buf), None, None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, 2, 0, None, C.byref(buf), None, None, None) == E_ARG
    assert call(fm._h, ch.ctypes.data, off.ctypes.data, 2, 0, line_off.ctypes.data, None, None, None, None) == E_ARG
    ids = np.zeros(2, np.int32)
    assert ia.lib.fmx_line_bounds_batch(fm._h, ids.ctypes.data, 2, ids.ctypes.data, ids.ctypes.data) == E_NO_DEVICE
    assert ia.lib.fmx_line_bounds_batch(fm._h, None, 2, ids.ctypes.data, ids.ctypes.data) == E_ARG
    assert ia.lib.fmx_lines_of_hits_dev(fm._h, 2, line_off.ctypes.data, ids.ctypes.data, 2, 0, line_off.ctypes.data, ids.ctypes.data, None, None, 0,
                                        None) == E_NO_DEVICE
    assert ia.lib.fmx_lines_of_hits_dev(fm._h, 2, line_off.ctypes.data, ids.ctypes.data, 1 << 31, 0, line_off.ctypes.data, ids.ctypes.data, None,
                                        None, 0, None) == E_ARG  # more than 2^31 - 1 hits
    assert ia.lib.fmx_lines_of_hits_dev(fm._h, 2, line_off.ctypes.data, ids.ctypes.data, 2, 0, None, ids.ctypes.data, None, None, 0, None) == E_ARG
    assert ia.lib.fmx_lines_of_hits_scratch_bytes(0, 5) == 0 and ia.lib.fmx_lines_of_hits_scratch_bytes(5, 0) == 0
    assert ia.lib.fmx_lines_of_hits_scratch_bytes(5, 1 << 31) == 0
    assert ia.lib.fmx_lines_of_hits_scratch_bytes(3, 1000) >= 24 * 1000
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert ia.lib.fmx_line_table_build(h, 10, None) == E_ARG
        assert call(h, ch.ctypes.data, off.ctypes.data, 2, 0, line_off.ctypes.data, C.byref(buf), None, None, None) == E_ARG
        assert ia.lib.fmx_line_bounds_batch(h, ids.ctypes.data, 2, ids.ctypes.data, ids.ctypes.data) == E_ARG
        assert ia.lib.fmx_lines_of_hits_dev(h, 2, line_off.ctypes.data, ids.ctypes.data, 2, 0, line_off.ctypes.data, ids.ctypes.data, None, None, 0,
                                            None) == E_ARG
    with pytest.raises(IndexError):
        fm.match_lines("")

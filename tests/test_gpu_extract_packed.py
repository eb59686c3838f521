"""Extract, packed (fmx_extract_packed_batch / fmx_line_text_batch / fmx_extract_packed_offsets_dev / fmx_extract_packed_fill_dev:
the three kernels of index4j_amd/csrc/fmx_extract_packed.hip) on the GPU.

The oracle is the judge (tests/orc.py): the expected packed array is the concatenation of its extract rows cut to length
(test_extract_packed_cpu.expected_packed; computed once, read-only).  The index is the reference's 2,000-line fixture followed by
the run-block text, whose quirk-Q1 rows derail the reference's walks: the redo list must NOT be empty there (asserted, read back
through fmx_extract_packed_last_redo and the head of the device form's scratch).  Every array is prefilled with a sentinel and
padded with it; the ranges hold the corner cases of the layout — asserted on the oracle's answer before the GPU runs.  Options
are set inside the tests and put back in `finally`."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_extract_packed_cpu import PAD, SENT, SENT16, ST_NOT_ENABLED, ST_POS_NEGATIVE, assert_corner_cases, check, expected_packed, piece_len, run_block_ranges
from test_gpu_locate_rows import _torch, n_cu, run_block_text

pytestmark = pytest.mark.gpu

HD = hdfs_text()
SR = 16
TILE = 1024  # kLocateAllTile of index4j_amd/csrc/fmx_device.hpp: the pieces of one tile of k_extract_packed_fill
DEFAULTS = {"window_cells": 2, "window_entry_bytes": 0, "image_compact": 0, "block": 512, "groups_per_cu": 16}
# (window_cells, window_entry_bytes, image_compact): no directory, cells with entries of 4 and of 6 bytes, the flat form, compact
RESIDENCIES = [(0, 0, 0), (1, 4, 0), (1, 6, 0), (3, 0, 0), (2, 0, 1)]


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
        yield
    finally:
        for k in kw:
            ia.lib.fmx_set_option(k.encode(), ia._lib.ENV_OPTIONS.get(k, DEFAULTS[k]))


def ok(rc):
    assert rc == 0, (ia.lib.fmx_last_error() or b"").decode()


def host_packed(fm, starts, stops):
    chars, text_off, st = fm.extract_packed_batch(starts, stops)
    return np.concatenate([chars, np.full(PAD, SENT16, np.uint16)]), text_off, st, int(ia.lib.fmx_extract_packed_last_redo())


def dev_packed(fm, starts, stops, front=0):
    """the device form, two stages with the caller's allocation between them; front: code units of padding in front of d_chars
    (an odd number: a destination that is 2-byte aligned only).  Returns (chars + PAD, text_off, status, ranges redone, front pad)."""
    torch = _torch()
    n = len(starts)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_a = torch.from_numpy(np.ascontiguousarray(starts, np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_b = torch.from_numpy(np.ascontiguousarray(stops, np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    text_off = torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda")
    piece_off = torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda")
    st = torch.full((max(n, 1),), SENT, dtype=torch.int32, device="cuda")
    nbytes = C.c_size_t(0)
    ok(ia.lib.fmx_extract_packed_scratch_bytes(fm.handle, n, C.byref(nbytes)))
    scratch = torch.full((nbytes.value + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    ok(ia.lib.fmx_extract_packed_offsets_dev(fm.handle, d_a.data_ptr(), d_b.data_ptr(), n, text_off.data_ptr(), piece_off.data_ptr(),
                                             st.data_ptr(), scratch.data_ptr(), nbytes.value, stream))
    torch.cuda.synchronize()
    total = int(text_off[n].item())  # (the caller's allocate-between-stages)
    chars = torch.full((front + total + PAD,), SENT16 - 0x10000, dtype=torch.int16, device="cuda")
    ok(ia.lib.fmx_extract_packed_fill_dev(fm.handle, d_a.data_ptr(), d_b.data_ptr(), n, text_off.data_ptr(), piece_off.data_ptr(),
                                          chars.data_ptr() + 2 * front, st.data_ptr(), scratch.data_ptr(), nbytes.value, stream))
    torch.cuda.synchronize()
    redone = int(scratch[:4].cpu().numpy().view(np.int32)[0]) if n else 0
    out = chars.cpu().numpy().view(np.uint16)
    return out[front:], text_off.cpu().numpy(), st.cpu().numpy()[:n], redone, out[:front]


def same(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("chars", "text_off", "status")):
        assert x.shape == y.shape and (x == y).all(), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def world():
    """the fixture followed by the run-block text at sampleRate 16, its oracle, the corner-case ranges and the oracle's answer"""
    text = HD + run_block_text()
    t16 = ia.as_chars(text)
    L = len(t16)
    o = orc.OracleFmIndex(text, SR, True)
    starts, stops = run_block_ranges(L, SR, np.random.default_rng(SR))
    exp = expected_packed(("hd+runblocks", SR), o, SR, starts, stops)
    assert_corner_cases(starts, stops, exp[2], SR, L)
    assert -(-L // piece_len(SR)) > TILE  # the whole text as ONE range crosses tiles: its slice of piece_off is a single entry
    i = int(np.flatnonzero((starts == 0) & (stops == L))[0])
    assert (exp[0][exp[1][i]:exp[1][i + 1]] != t16).any()  # quirk Q1: the reference's own answer differs from the text
    return text, t16, o, starts, stops, exp


_FIRST = {}


@pytest.mark.parametrize("cells,entry,compact", RESIDENCIES)
def test_entry_points_and_residencies(world, cells, entry, compact):
    text, t16, o, starts, stops, exp = world
    what = "window_cells %d entry bytes %d compact %d" % (cells, entry, compact)
    with options(window_cells=cells, window_entry_bytes=entry, image_compact=compact):
        fm = ia.FmIndex(text, SR, True, device=None)
        fm.blob()  # flattened under the option
        fm.to_device(0)
    try:
        if cells != 2:
            assert (fm.window_cells_bytes() > 0) == (cells != 0)
        host = host_packed(fm, starts, stops)
        check(host, exp, what + " host")
        assert 0 < host[3] < len(starts), "%s: %d ranges redone" % (what, host[3])  # the redo list IS non-empty on this index
        dev = dev_packed(fm, starts, stops)
        check(dev, exp, what + " device")
        assert dev[3] == host[3]
        same(dev, host, what + ": device form vs host form")
        same(host, _FIRST.setdefault("ranges", host), what + ": vs the first residency")
        # repeatability: two runs, byte for byte (without the two whole-text ranges: quirk Q1 sends each of them through the
        # literal walk of ONE lane, a second per call; the ranges with a status stay, stops past the text among them)
        few = np.flatnonzero(~((starts == 0) & (stops == len(t16))))
        assert len(few) == len(starts) - 2 and (stops[few].astype(np.int64) - starts[few])[exp[2][few] == 0].max() < 100_000
        fexp = expected_packed(("hd+runblocks, short", SR), o, SR, starts[few], stops[few])
        runs = [host_packed(fm, starts[few], stops[few]), host_packed(fm, starts[few], stops[few]),
                dev_packed(fm, starts[few], stops[few]), dev_packed(fm, starts[few], stops[few], front=3)]
        for k, run in enumerate(runs):  # (the last: into a destination that is 2-byte aligned only, behind a guard)
            check(run, fexp, "%s: short ranges, run %d" % (what, k))
            same(run, runs[0], "%s: run %d vs run 0" % (what, k))
            assert run[3] > 0
        assert (runs[3][4] == SENT16).all(), what + ": stored in front of the destination"
        # the line form: every line of the text, ids -1 and n_lines among them, against the oracle's extract of the table's bounds
        n_lines = fm.build_line_table("\n")
        assert n_lines > 2000
        ids = np.concatenate([[-1], np.arange(n_lines), [n_lines]]).astype(np.int32)
        a, b = fm.line_bounds(ids)
        assert a[0] == -1 and b[-1] == -1
        lexp = expected_packed(("lines", SR), o, SR, a, b)
        assert lexp[2][0] == ST_POS_NEGATIVE and lexp[2][-1] == ST_POS_NEGATIVE and (lexp[2][1:-1] == 0).all()
        chars, text_off, st = fm.line_text_batch(ids)
        check((np.concatenate([chars, np.full(PAD, SENT16, np.uint16)]), text_off, st), lexp, what + " lines")
        lines = text.split("\n")
        got = fm.line_text(np.arange(2000))
        assert got == lines[:2000], what  # the fixture's 2,000 lines are the text's own
        with pytest.raises(Exception):
            fm.line_text([n_lines])
    finally:
        fm.close()


@pytest.fixture(scope="module")
def hd():
    fm = ia.FmIndex(HD, SR, True, device=0)
    yield fm, HD.split("\n")
    fm.close()


def test_grep_and_the_lines_of_a_pattern(hd):
    fm, lines = hd
    no_table = ia.lib.fmx_line_text_batch(fm.handle, np.zeros(1, np.int32).ctypes.data, 1, np.zeros(2, np.int64).ctypes.data,
                                          C.byref(C.c_void_p()), None)
    assert no_table == ia._lib.E_ARG and b"fmx_line_table_build" in ia.lib.fmx_last_error()
    assert fm.build_line_table("\n") == 2000
    ids = fm.match_lines(" ")
    assert len(ids) == 2000
    assert fm.line_text(ids) == [lines[i] for i in ids]
    got = fm.grep(all=["INFO", "PacketResponder", "terminating"])
    assert len(got) == 310
    for i, line in got:
        assert line == lines[i] and all(w in line for w in ("INFO", "PacketResponder", "terminating"))
    assert fm.grep("PacketResponder", max_lines=5) == [(i, lines[i]) for i in fm.match_lines("PacketResponder")[:5]]
    assert fm.grep(all=["INFO"], none=["INFO"]) == []
    chars, text_off, st = fm.line_text_batch([-1, 2000, 0])
    assert st.tolist() == [ST_POS_NEGATIVE, ST_POS_NEGATIVE, 0] and text_off.tolist() == [0, 0, 0, len(lines[0])]


def test_extract_not_enabled_and_empty_batches(hd):
    fm, _ = hd
    for starts, stops in ((np.zeros(0, np.int32), np.zeros(0, np.int32)),):
        chars, text_off, st = fm.extract_packed_batch(starts, stops)
        assert len(chars) == 0 and text_off.tolist() == [0] and len(st) == 0
        dev = dev_packed(fm, starts, stops)
        assert dev[1].tolist() == [0] and (dev[0] == SENT16).all()
    fm.build_line_table("\n")
    chars, text_off, st = fm.line_text_batch([])
    assert len(chars) == 0 and text_off.tolist() == [0]
    off = ia.FmIndex(HD[:5000], 8, False, device=0)
    try:
        a, b = np.array([0, 5, -1, 10], np.int32), np.array([10, 5, 4, 9000], np.int32)
        for res in (host_packed(off, a, b), dev_packed(off, a, b)):
            assert (res[2] == ST_NOT_ENABLED).all() and (res[1] == 0).all() and (res[0] == SENT16).all()
    finally:
        off.close()


def test_launch_shapes(hd):
    """block 1024 with one workgroup per CU: enough whole-text ranges that every workgroup's tile loop runs three times at least
    (the fixture alone: no quirk rows, so no range of a quarter of a million characters is redone by one lane)"""
    fm, _ = hd
    t16 = ia.as_chars(HD)
    L = len(t16)
    o = orc.OracleFmIndex(HD, SR, True)
    one = expected_packed(("hd whole", SR), o, SR, np.zeros(1, np.int32), np.full(1, L, np.int32))
    whole = one[0]
    assert len(whole) == L and (whole == t16).all()
    pieces = -(-L // piece_len(SR))
    assert pieces > TILE
    k = -(-3 * TILE * n_cu() // pieces) + 1
    a, b = np.zeros(k + 2, np.int32), np.full(k + 2, L, np.int32)
    a[0], b[0], a[-1], b[-1] = 5, 5, L, L  # the first and the last range empty
    for block, groups in ((1024, 1), (512, 1), (1024, 16)):
        with options(block=block, groups_per_cu=groups):
            if groups == 1:
                assert -(-k * pieces // TILE) >= 3 * n_cu() * groups  # tiles per workgroup of the capped grid
            dev = dev_packed(fm, a, b)
            assert dev[1].tolist() == [0] + [j * L for j in range(k + 1)] + [k * L] and (dev[2] == 0).all()
            got = dev[0][:k * L].reshape(k, L)
            bad = np.flatnonzero((got != whole[None, :]).any(axis=1))
            assert len(bad) == 0, "block %d groups %d: ranges %r differ" % (block, groups, bad[:5])
            assert (dev[0][k * L:] == SENT16).all() and dev[3] == 0
    with options(block=1024, groups_per_cu=1):
        chars, text_off, st = fm.extract_packed_batch(a[:3], b[:3])
        assert (chars.reshape(2, L) == whole[None, :]).all() and text_off.tolist() == [0, 0, L, 2 * L]


def test_cpp_mirror(tmp_path):
    """tests/cpp/test_extract_packed_mirror.cpp prints what extractPacked / lineTextBatch / lineText return"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_extract_packed_mirror")
    libdir = os.path.join(root, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_extract_packed_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(root, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    L = len(ia.as_chars(HD))
    o = orc.OracleFmIndex(HD, SR, True)
    starts = np.array([5, 0, 15, 1000, L - 40, -1, 10, 70000, 9], np.int32)
    stops = np.array([5, 1, 49, 1300, L, 4, L + 1, 69000, 10], np.int32)
    exp = expected_packed(("hd mirror", SR), o, SR, starts, stops)
    assert out["offsets"] == exp[1].tolist() and out["status"] == exp[2].tolist() and out["chars"] == exp[0].tolist()
    assert out["status"] == [0, 0, 0, 0, 0, 2, 3, 0, 0]
    lines = HD.split("\n")
    want = [lines[0], lines[1999], "", "", lines[7]]
    assert out["n_lines"] == [2000] and out["line_status"] == [0, 0, ST_POS_NEGATIVE, ST_POS_NEGATIVE, 0]
    assert out["line_offsets"] == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert out["line_chars"] == ia.as_chars("".join(want)).tolist()
    assert out["line3"] == ia.as_chars(lines[3]).tolist() and out["line4"] == ia.as_chars(lines[4]).tolist()

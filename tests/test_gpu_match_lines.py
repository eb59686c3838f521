"""The lines that match on the GPU: the line table (fmx_line_table_build / fmx_line_table_info / fmx_line_bounds_batch), packed hits ->
packed distinct lines (fmx_lines_of_hits_dev: the kernels of fmx_hit_lines.hip and rocPRIM's sort and scans) and the host form
fmx_match_lines_batch, with their Python and C++ mirrors.

The judge is the oracle plus numpy (tests/test_match_lines_cpu.py: judge_table, judge_lines — T = the oracle's locate() of the
boundary, sorted; a pattern's lines = np.unique(np.searchsorted(T, its hits, "left"))), computed once per batch.  Outputs are
prefilled with a sentinel.  The batches hold the corner cases — asserted on the judge's answer before the GPU runs.  Options are
set inside the tests and put back in `finally`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import _torch, options, run_block_text
from test_locate_all_cpu import ABSENT, SENT, assert_corner_cases, corner_batch, expected_packed
from test_match_lines_cpu import MAX_LINES, check_lines, judge_bounds, judge_lines, judge_n_lines, judge_table, with_boundary_patterns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
NL = ord("\n")
PAD = 64  # ints behind line_off[n] that must keep the sentinel
_JUDGE = {}


def judged(key, T, exp, max_lines):
    """judge_lines, once per (batch, limit), read-only"""
    if (key, max_lines) not in _JUDGE:
        res = judge_lines(T, exp[0], exp[1], max_lines)
        for a in res:
            a.setflags(write=False)
        _JUDGE[key, max_lines] = res
    return _JUDGE[key, max_lines]


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def host_lines(fm, ch, off, max_lines):
    lines, line_off, st, line_count, occ = fm.match_lines_batch(ch, off, max_lines, want_counts=True)
    return (np.concatenate([lines, np.full(PAD, SENT, np.int32)]), line_off, line_count), st, occ


def dev_lines(d, max_lines, extra_hits=0, ws_bytes=None):
    """fmx_lines_of_hits_dev over what a DevAll (stage 1 + a full stage 2) left; extra_hits: n_hits beyond hit_off[n]"""
    torch = d.torch
    n_hits = d.total + extra_hits
    assert extra_hits <= PAD  # (d.locs has that many slots behind the hits)
    need = ia.lib.fmx_lines_of_hits_scratch_bytes(d.n, n_hits)
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device="cuda")
    line_off = torch.full((d.n + 1,), SENT, dtype=torch.int64, device="cuda")
    lines = torch.full((n_hits + PAD,), SENT, dtype=torch.int32, device="cuda")
    line_count = torch.full((max(d.n, 1),), SENT, dtype=torch.int32, device="cuda")
    rc = ia.lib.fmx_lines_of_hits_dev(d.fm.handle, d.n, d.hit_off.data_ptr(), d.locs.data_ptr(), n_hits, max_lines, line_off.data_ptr(),
                                      lines.data_ptr(), line_count.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, d.stream)
    torch.cuda.synchronize()
    return rc, (lines.cpu().numpy(), line_off.cpu().numpy(), line_count.cpu().numpy()[: d.n])


def filled(fm, ch, off):
    d = DevAll(fm, ch, off, -1)
    d.fill(0, d.total)
    return d


@pytest.fixture(scope="module")
def hd():
    """the fixture at sampleRate 16 with its line table, its oracle, the judge's T and the corner-case batch (about 10^6 hits)"""
    t16 = ia.as_chars(HD)
    o = orc.OracleFmIndex(HD, 16, True)
    T = judge_table(o, NL)
    ch, off = corner_batch(t16, np.random.default_rng(16), 2900, min_len=2)
    ch, off = with_boundary_patterns(t16, ch, off, T, NL, more=("blk_",))
    exp = expected_packed("hd16 match lines", o, ch, off, -1)
    packed, hit_off, status, _, counts = exp
    # the corner cases, on the judge's answer
    assert_corner_cases(counts, status)
    assert counts[0] == 0 and counts[-1] == 0 and (status == 9).sum() == 1
    all_lines = judged("hd16", T, exp, 0)
    line_count = all_lines[2]
    pats = [ia.chars_to_str(ch[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    sp, blk = pats.index(" "), pats.index("blk_")
    assert counts[sp] == 30094 and line_count[sp] == 2000                # hits >= 10 x lines
    assert counts[blk] == 2468 and line_count[blk] == 1999               # a few hits more than lines
    assert (line_count == 1).any() and ((counts > 0) == (line_count > 0)).all()
    assert line_count[pats.index("\n")] == 2000 and counts[pats.index("\n")] == 2000
    assert int(hit_off[-1]) > 900_000
    fm = ia.FmIndex(HD, 16, True, device=0)
    assert fm.build_line_table("\n") == 2000
    yield t16, o, T, ch, off, exp, fm
    fm.close()


def test_line_table_build_replace_and_bounds(hd):
    t16, o, T, ch, off, exp, fm = hd
    assert len(T) == 2000 and judge_n_lines(T, len(t16)) == 2000
    info = fm.line_table_info()
    assert info[0] == NL and info[1] == 2000 and info[2] >= 8000
    ids = np.arange(2000, dtype=np.int32)
    start, stop = fm.line_bounds(ids)
    assert (stop == T).all() and (start == np.concatenate([[0], T[:-1] + 1])).all()  # the table, read back
    assert fm.build_line_table("\n") == 2000 and fm.line_table_info() == info          # a second build: nothing happens
    assert (fm.line_bounds(ids)[1] == T).all()
    odd = np.array([-1, 2000, 2001, 2**31 - 1, -2**31, 0, 1999], np.int32)
    s, e = fm.line_bounds(odd)
    es, ee = judge_bounds(T, 2000, len(t16), odd)
    assert (s == es).all() and (e == ee).all() and list(s[:5]) == [-1] * 5
    # another boundary replaces the table; the first one again restores it
    Ts = judge_table(o, " ")
    n_sp = judge_n_lines(Ts, len(t16))
    assert len(Ts) == 30094 and n_sp == 30095
    assert fm.build_line_table(" ") == n_sp
    assert fm.line_table_info()[:2] == (32, 30094)
    s, e = fm.line_bounds(np.arange(n_sp, dtype=np.int32))
    es, ee = judge_bounds(Ts, n_sp, len(t16), np.arange(n_sp))
    assert (s == es).all() and (e == ee).all()
    assert fm.build_line_table("\n") == 2000 and fm.line_table_info() == info
    assert (fm.line_bounds(ids)[1] == T).all()
    # the device form of the bounds
    torch = _torch()
    d_ids = torch.from_numpy(odd).cuda()
    d_s, d_e = torch.full((len(odd),), SENT, dtype=torch.int32, device="cuda"), torch.full((len(odd),), SENT, dtype=torch.int32, device="cuda")
    assert ia.lib.fmx_line_bounds_batch_dev(fm.handle, d_ids.data_ptr(), len(odd), d_s.data_ptr(), d_e.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    es, ee = judge_bounds(T, 2000, len(t16), odd)
    assert (d_s.cpu().numpy() == es).all() and (d_e.cpu().numpy() == ee).all()


@pytest.fixture(scope="module")
def hd_filled(hd):
    t16, o, T, ch, off, exp, fm = hd
    d = filled(fm, ch, off)
    assert d.total == int(exp[1][-1])
    return d


@pytest.mark.parametrize("max_lines", MAX_LINES)
def test_corner_batch_host_and_device_forms(hd, hd_filled, max_lines):
    t16, o, T, ch, off, exp, fm = hd
    want = judged("hd16", T, exp, max_lines)
    got, st, occ = host_lines(fm, ch, off, max_lines)
    check_lines(got, want, "host form, max_lines %d" % max_lines, tail=SENT)
    assert (st == exp[2]).all() and (occ == exp[4]).all()
    rc, dev = dev_lines(hd_filled, max_lines)
    assert rc == 0, last_error()
    check_lines(dev, want, "device form, max_lines %d" % max_lines, tail=SENT)  # (the sentinel intact behind d_line_off[n])
    total = int(want[1][-1])
    assert (dev[0][:total] == got[0][:total]).all() and (dev[1] == got[1]).all() and (dev[2] == got[2]).all()
    if max_lines in (0, 16):  # d_locs with slots behind hit_off[n]
        rc, dev = dev_lines(hd_filled, max_lines, extra_hits=37)
        assert rc == 0, last_error()
        check_lines(dev, want, "device form, n_hits beyond hit_off[n], max_lines %d" % max_lines, tail=SENT)


def test_skew_one_heavy_pattern_and_many_light_ones(hd):
    t16, o, T, ch, off, exp, fm = hd
    # ONE pattern that matches in every line
    ch1, off1 = ia.pack_patterns([" "])
    off1 = off1.astype(np.int32)
    exp1 = expected_packed("hd16 one heavy", o, ch1, off1, -1)
    assert int(exp1[1][-1]) == 30094
    for max_lines in (0, 7):
        want = judged("hd16 one heavy", T, exp1, max_lines)
        got, st, occ = host_lines(fm, ch1, off1, max_lines)
        check_lines(got, want, "one heavy pattern, host form", tail=SENT)
        assert list(occ) == [30094] and list(got[2]) == [2000]
        rc, dev = dev_lines(filled(fm, ch1, off1), max_lines)
        assert rc == 0, last_error()
        check_lines(dev, want, "one heavy pattern, device form", tail=SENT)
    # 3,000 patterns of at most one hit each
    rng = np.random.default_rng(77)
    cand = []
    for j, s in enumerate(rng.integers(0, len(t16) - 61, 9000)):
        p = t16[s:s + 60].copy()
        if j % 5 == 2:
            p[0] = ABSENT
        cand.append(p)
    cch, coff = ia.pack_patterns(cand)
    cc, _ = o.count_batch(cch, coff.astype(np.int32), threads=16)
    light = [cand[i] for i in np.flatnonzero(cc <= 1)[:3000]]
    assert len(light) == 3000
    chl, offl = ia.pack_patterns(light)
    offl = offl.astype(np.int32)
    expl = expected_packed("hd16 light", o, chl, offl, -1)
    assert expl[4].max() == 1 and 1500 < int(expl[1][-1]) < 3000
    want = judged("hd16 light", T, expl, 0)
    got, st, occ = host_lines(fm, chl, offl, 0)
    check_lines(got, want, "3,000 light patterns, host form", tail=SENT)
    assert (occ == expl[4]).all()
    rc, dev = dev_lines(filled(fm, chl, offl), 0)
    assert rc == 0, last_error()
    check_lines(dev, want, "3,000 light patterns, device form", tail=SENT)


_BETWEEN = {}


@pytest.mark.parametrize("cells,rows,compact", [(0, 0, 0), (1, 1, 0), (2, 0, 1)])
def test_residencies(hd, cells, rows, compact):
    t16, o, T, ch, off, exp = hd[:6]
    what = "window_cells %d locate_rows %d compact %d" % (cells, rows, compact)
    with options(window_cells=cells, locate_rows=rows, image_compact=compact):
        fm = ia.FmIndex(HD, 16, True, device=None)
        fm.blob()  # flattened under the option
        fm.to_device(0)
    try:
        assert (fm.locate_rows_info()[0] > 0) == bool(rows)
        assert fm.build_line_table("\n") == 2000
        assert (fm.line_bounds(np.arange(2000, dtype=np.int32))[1] == T).all()
        want = judged("hd16", T, exp, 0)
        got, st, occ = host_lines(fm, ch, off, 0)
        check_lines(got, want, what, tail=SENT)
        assert (st == exp[2]).all() and (occ == exp[4]).all()
        first = _BETWEEN.setdefault("first", got)
        assert all((a == b).all() for a, b in zip(got, first)), what + ": vs the first residency"
    finally:
        fm.close()


def test_quirk_text_table_is_what_the_reference_answers():
    """the run-block text with its most frequent symbol as the boundary: T is the sorted locate() of the oracle — derailed walks of
    quirk Q1 included — and every single-symbol pattern gets the judge's lines.  This pins "as the reference answers"."""
    text = run_block_text()
    t16 = ia.as_chars(text)
    syms, cnt = np.unique(t16, return_counts=True)
    boundary = int(syms[np.argmax(cnt)])
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, boundary)
    assert len(T) == cnt.max() == 70000
    n_lines = judge_n_lines(T, len(t16))
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in syms])
    off = off.astype(np.int32)
    exp = expected_packed("runblocks16", o, ch, off, -1)
    assert int(exp[1][-1]) == len(t16)
    fm = ia.FmIndex(text, 16, True, device=0)
    try:
        assert fm.build_line_table(boundary) == n_lines
        assert fm.line_table_info()[:2] == (boundary, 70000)
        s, e = fm.line_bounds(np.arange(n_lines, dtype=np.int32))
        es, ee = judge_bounds(T, n_lines, len(t16), np.arange(n_lines))
        assert (e[:70000] == T).all() and (s == es).all() and (e == ee).all()
        want = judged("runblocks16", T, exp, 0)
        got, st, occ = host_lines(fm, ch, off, 0)
        check_lines(got, want, "run blocks, host form", tail=SENT)
        assert (occ == exp[4]).all()
        rc, dev = dev_lines(filled(fm, ch, off), 0)
        assert rc == 0, last_error()
        check_lines(dev, want, "run blocks, device form", tail=SENT)
    finally:
        fm.close()


def test_size_every_grid_stride_loop_runs_several_times():
    text = ia.synth_log(1 << 21)
    t16 = ia.as_chars(text)
    fm = ia.FmIndex(text, 16, True, device=0, build_device=0)
    try:
        o = orc.OracleFmIndex.read(fm.write(False))
        ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in np.unique(t16)])
        off = off.astype(np.int32)
        exp = expected_packed("synth21", o, ch, off, -1)  # (the batch of test_gpu_locate_all's `synth` fixture: computed once)
        total = int(exp[1][-1])
        assert total == len(t16)  # 2 M packed hits
        T = judge_table(o, NL)
        assert fm.build_line_table("\n") == judge_n_lines(T, len(t16))
        key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
        assert ia.lib.fmx_hit_lines_geometry(fm.handle, total, C.byref(key_grid), C.byref(flat_grid)) == 0
        assert 3 * key_grid.value * 1024 <= total and 3 * flat_grid.value * 256 <= total  # every loop runs at least three times
        want = judged("synth21", T, exp, 0)
        assert (want[2] < np.diff(exp[1])).any()
        got, st, occ = host_lines(fm, ch, off, 0)
        check_lines(got, want, "2 M hits, host form", tail=SENT)
        rc, dev = dev_lines(filled(fm, ch, off), 0)
        assert rc == 0, last_error()
        check_lines(dev, want, "2 M hits, device form", tail=SENT)
    finally:
        fm.close()


def test_errors_and_edges(hd):
    t16, o, T, ch, off, exp = hd[:6]
    E_ARG = ia._lib.E_ARG
    torch = _torch()
    fm = ia.FmIndex(HD, 16, True, device=0)
    try:
        assert fm.line_table_info() == (-1, 0, 0)
        ch2, off2 = ia.pack_patterns(["INFO", "blk_"])
        off2 = off2.astype(np.int32)
        # no table: FMX_E_ARG, and the message names the call that makes one
        line_off = np.full(3, SENT, np.int64)
        buf = C.c_void_p(0x1234)
        rc = ia.lib.fmx_match_lines_batch(fm.handle, ch2.ctypes.data, off2.ctypes.data, 2, 0, line_off.ctypes.data, C.byref(buf), None, None, None)
        assert rc == E_ARG and "fmx_line_table_build" in last_error() and buf.value is None and (line_off == SENT).all()
        ids = np.zeros(2, np.int32)
        assert ia.lib.fmx_line_bounds_batch(fm.handle, ids.ctypes.data, 2, ids.ctypes.data, ids.ctypes.data) == E_ARG
        assert "fmx_line_table_build" in last_error()
        d = filled(fm, ch2, off2)
        rc, _ = dev_lines(d, 0)
        assert rc == E_ARG and "fmx_line_table_build" in last_error()
        assert fm.build_line_table("\n") == 2000
        # a workspace that is too small: an error, and nothing is launched
        rc, dev = dev_lines(d, 0, ws_bytes=ia.lib.fmx_lines_of_hits_scratch_bytes(2, d.total) - 256)
        assert rc == E_ARG and (dev[1] == SENT).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all()
        rc, dev = dev_lines(d, 0)
        assert rc == 0, last_error()
        exp2 = expected_packed("hd16 two", o, ch2, off2, -1)
        check_lines(dev, judged("hd16 two", T, exp2, 0), "two patterns", tail=SENT)
        # n == 0
        h = np.full(1, SENT, np.int64)
        assert ia.lib.fmx_match_lines_batch(fm.handle, None, None, 0, 0, h.ctypes.data, C.byref(buf), None, None, None) == 0
        assert h[0] == 0 and buf.value is None
        d_off = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
        assert ia.lib.fmx_lines_of_hits_dev(fm.handle, 0, None, None, 0, 0, d_off.data_ptr(), None, None, None, 0,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert int(d_off.cpu()[0]) == 0
        # a batch without hits (device form: n_hits == 0 — the offsets are zeroed, nothing else is written)
        ch0, off0 = ia.pack_patterns(["zzzzqq#", "", "qqqqzz#"])
        off0 = off0.astype(np.int32)
        lines, line_off, st, line_count, occ = fm.match_lines_batch(ch0, off0, 0, want_counts=True)
        assert len(lines) == 0 and (line_off == 0).all() and list(st) == [0, 9, 0] and (line_count == 0).all() and (occ == 0).all()
        d0 = filled(fm, ch0, off0)
        assert d0.total == 0
        rc, dev = dev_lines(d0, 0)
        assert rc == 0 and (dev[1] == 0).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all()
        # offsets that decrease: the host form's check
        bad = np.array([0, 3, 2, 4], np.int32)
        assert ia.lib.fmx_match_lines_batch(fm.handle, ch0.ctypes.data, bad.ctypes.data, 3, 0, np.zeros(4, np.int64).ctypes.data, C.byref(buf),
                                            None, None, None) == E_ARG
        # resident again: the table is gone with the rest of the resident state
        fm.to_device(0)
        assert fm.line_table_info() == (-1, 0, 0)
        rc = ia.lib.fmx_match_lines_batch(fm.handle, ch2.ctypes.data, off2.ctypes.data, 2, 0, line_off.ctypes.data, C.byref(buf), None, None, None)
        assert rc == E_ARG and "fmx_line_table_build" in last_error()
    finally:
        fm.close()


def test_round_trip_and_mirrors(hd, tmp_path):
    t16, o, T, ch, off, exp, fm = hd
    text_lines = HD.split("\n")[:2000]
    warn = [k for k, ln in enumerate(text_lines) if "WARN" in ln]
    assert len(warn) == 80
    got = fm.match_lines("WARN")
    assert got.dtype == np.int32 and list(got) == warn
    assert list(fm.match_lines("WARN", max_lines=5)) == warn[:5]
    start, stop = fm.line_bounds(got)
    width = int((stop - start).max())
    dst, out_len, st = fm.extract_batch(start, stop, width)
    assert (st == 0).all() and (out_len == stop - start).all()
    assert [ia.chars_to_str(dst[i, : out_len[i]]) for i in range(len(got))] == [text_lines[k] for k in warn]
    with pytest.raises(IndexError):
        fm.match_lines("")
    # the C++ mirror: tests/cpp/test_match_lines_mirror.cpp prints what buildLineTable / matchLinesBatch / matchLines return
    exe = str(tmp_path / "test_match_lines_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_match_lines_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    chm, offm = ia.pack_patterns(["WARN", "zzzzqq#", "blk_"])
    offm = offm.astype(np.int32)
    expm = expected_packed("hd16 mirror", o, chm, offm, -1)
    lines, line_off, line_count = judged("hd16 mirror", T, expm, 0)
    assert out["n_lines"] == [2000]
    assert out["batch_offsets"] == list(line_off) and out["batch_lines"] == list(lines)
    assert out["batch_line_count"] == list(line_count) == [80, 0, 1999] and out["batch_occurrences"] == list(expm[4])
    cut = judged("hd16 mirror", T, expm, 7)
    assert out["cut_offsets"] == [0, 7, 7, 14] == list(cut[1]) and out["cut_lines"] == list(cut[0]) and out["cut_line_count"] == [80, 0, 1999]
    assert out["one"] == warn

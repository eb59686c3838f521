""""All occurrences", packed (fmx_locate_all_batch / fmx_locate_all_ranges_dev / fmx_locate_all_fill_dev: k_locate_all of
fmx_kernels.hip, the hit counts and their scan of fmx_hit_offsets.hip) on the GPU.

The oracle is the judge (tests/orc.py): the expected packed result is its locate_batch with loc_cap = the largest count, each row's
first found[i] entries concatenated (test_locate_all_cpu.expected_packed; computed once, read-only).  Outputs are prefilled with
a sentinel.  The batches hold the corner cases of the layout — asserted on the oracle's answer before the GPU runs.  Options are
set inside the tests and put back in `finally`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_gpu_locate_rows import SHAPES, _torch, n_cu, options, run_block_text
from test_locate_all_cpu import SENT, assert_corner_cases, check, corner_batch, expected_packed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
# kLocateAllTile of index4j_amd/csrc/fmx_device.hpp: the hits of one tile of k_locate_all (a compile-time constant, not an option)
TILE = 1024
PAD = 64  # ints behind hit_off[n] that must keep the sentinel


def host_all(fm, ch, off, mm):
    locs, hit_off, st, lf = fm.locate_all_batch(ch, off, mm, want_steps=True)
    return np.concatenate([locs, np.full(PAD, SENT, np.int32)]), hit_off, st, lf


class DevAll:
    """the device form: stage 1 once, then any number of stage-2 windows into one sentinel-filled array"""

    def __init__(self, fm, ch, off, mm):
        torch = _torch()
        self.torch, self.fm, self.n = torch, fm, len(off) - 1
        n = self.n
        self.d_ch = torch.from_numpy(ch.view(np.int16)).cuda() if len(ch) else torch.zeros(1, dtype=torch.int16, device="cuda")
        self.d_off = torch.from_numpy(off).cuda()
        sent = lambda k: torch.full((max(k, 1),), SENT, dtype=torch.int32, device="cuda")
        self.lf, self.st, self.rng = sent(n), sent(n), sent(2 * n)
        self.hit_off = torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = ia.lib.fmx_locate_all_ranges_dev(fm.handle, self.d_ch.data_ptr(), self.d_off.data_ptr(), n, mm, self.hit_off.data_ptr(),
                                              self.lf.data_ptr(), self.st.data_ptr(), self.rng.data_ptr(), self.stream)
        assert rc == 0, (ia.lib.fmx_last_error() or b"").decode()
        torch.cuda.synchronize()
        self.total = int(self.hit_off[n].item())  # (the caller's allocate-between-stages)
        self.locs = sent(self.total + PAD)

    def fill(self, first, hits, at=None):
        rc = ia.lib.fmx_locate_all_fill_dev(self.fm.handle, self.n, self.hit_off.data_ptr(), self.rng.data_ptr(), first, hits,
                                            self.locs.data_ptr() + 4 * (first if at is None else at), self.lf.data_ptr(),
                                            self.st.data_ptr(), self.stream)
        assert rc == 0, (ia.lib.fmx_last_error() or b"").decode()

    def result(self):
        self.torch.cuda.synchronize()
        return self.locs.cpu().numpy(), self.hit_off.cpu().numpy(), self.st.cpu().numpy()[: self.n], self.lf.cpu().numpy()[: self.n]


def dev_all(fm, ch, off, mm):
    d = DevAll(fm, ch, off, mm)
    d.fill(0, d.total)
    return d.result()


def same(a, b, what):
    for x, y, name in zip(a, b, ("locs", "hit_off", "status", "lf_steps")):
        assert x.shape == y.shape and (x == y).all(), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def hd():
    """the fixture at sampleRate 16, its oracle and the corner-case batch of about 3,000 patterns"""
    t16 = ia.as_chars(HD)
    o = orc.OracleFmIndex(HD, 16, True)
    ch, off = corner_batch(t16, np.random.default_rng(16), 2900, min_len=2)  # 1.04 M hits
    oc, ost = o.count_batch(ch, off, threads=16)
    assert_corner_cases(oc, ost)
    for s, c in ((" ", 30094), ("1", 22337), ("0", 18814), ("INFO", 1920)):
        assert o.count(ia.as_chars(s)) == c
    return t16, o, ch, off


MMS = (-1, 0, 1, 16, 1000)
RESIDENCIES = [(0, 0, 0), (1, 0, 0), (3, 0, 0), (0, 1, 0), (1, 1, 0), (3, 1, 0), (2, 0, 1)]  # (window_cells, locate_rows, image_compact)
_BETWEEN = {}


@pytest.mark.parametrize("cells,rows,compact", RESIDENCIES)
def test_entry_points_and_residencies(hd, cells, rows, compact):
    t16, o, ch, off = hd
    what = "window_cells %d locate_rows %d compact %d" % (cells, rows, compact)
    with options(window_cells=cells, locate_rows=rows, image_compact=compact):
        fm = ia.FmIndex(HD, 16, True, device=None)
        fm.blob()  # flattened under the option
        fm.to_device(0)
    try:
        assert (fm.locate_rows_info()[0] > 0) == bool(rows)
        if cells != 2:
            assert (fm.window_cells_bytes() > 0) == (cells != 0)
        for mm in MMS:
            exp = expected_packed("hd16", o, ch, off, mm)
            host = host_all(fm, ch, off, mm)
            check(host, exp, "%s host mm %d" % (what, mm))
            dev = dev_all(fm, ch, off, mm)
            check(dev, exp, "%s device mm %d" % (what, mm))
            same(dev, host, "%s mm %d: device form vs host form" % (what, mm))
            first = _BETWEEN.setdefault(mm, host)
            same(host, first, "%s mm %d: vs the first residency" % (what, mm))
        # maxMatches 16: the first found[i] entries of fmx_locate_batch's rows on the same handle
        n = len(off) - 1
        rows16 = np.full((n, 16), SENT, np.int32)
        rows16, found, st, lf = fm.locate_batch(ch, off, 16, 16, want_steps=True, locs=rows16)
        host = host_all(fm, ch, off, 16)
        assert (np.diff(host[1]) == found).all()
        assert (host[0][: int(host[1][-1])] == rows16[np.arange(16)[None, :] < found[:, None]]).all()
        assert (host[2] == st).all() and (host[3] == lf).all()
    finally:
        fm.close()


@pytest.mark.parametrize("rows", [0, 1])
def test_quirk_rows(rows):
    """every single-symbol pattern of the run-block text without a limit: all rows but the sentinel's, derailed walks (quirk Q1) and
    replay rows included"""
    text = run_block_text()
    t16 = ia.as_chars(text)
    o = orc.OracleFmIndex(text, 16, True)
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in np.unique(t16)])
    off = off.astype(np.int32)
    exp = expected_packed("runblocks16", o, ch, off, -1)
    assert int(exp[1][-1]) == len(t16)
    with options(locate_rows=rows):
        fm = ia.FmIndex(text, 16, True, device=0)
    try:
        nbytes, replay = fm.locate_rows_info()
        assert (nbytes > 0) == bool(rows)
        if rows:
            assert replay > 0
        check(host_all(fm, ch, off, -1), exp, "run blocks, host form, locate_rows %d" % rows)
        check(dev_all(fm, ch, off, -1), exp, "run blocks, device form, locate_rows %d" % rows)
    finally:
        fm.close()


PAGING_HEAVY = ("INFO", "blk_", "dfs.", "Receiv")


@pytest.fixture(scope="module")
def paged(hd):
    """a batch with the same corner cases and fewer hits (no single characters): windows of ONE hit are a launch per hit"""
    t16, o = hd[:2]
    ch, off = corner_batch(t16, np.random.default_rng(3), 90, heavy=PAGING_HEAVY, min_len=10)  # 23,014 hits
    oc, ost = o.count_batch(ch, off, threads=16)
    assert_corner_cases(oc, ost)
    fm = ia.FmIndex(HD, 16, True, device=0)
    one_shot = dev_all(fm, ch, off, -1)
    check(one_shot, expected_packed("hd16 paging", o, ch, off, -1), "one-shot fill")
    yield fm, ch, off, one_shot
    fm.close()


@pytest.mark.parametrize("window", [1, 63, 64, 65, 4097])
def test_paging(paged, window):
    """stage 2 in windows that tile [0, hit_off[n]) once: positions, LF-steps and statuses of the one-shot fill; the sentinel intact
    behind hit_off[n]"""
    fm, ch, off, one_shot = paged
    d = DevAll(fm, ch, off, -1)
    assert d.total == int(one_shot[1][-1]) and d.total > 3 * 4097
    for at in range(0, d.total, window):
        d.fill(at, window)  # (the last window overhangs the end unless the size divides the total)
    res = d.result()
    same(res, one_shot, "windows of %d" % window)
    assert (res[0][d.total:] == SENT).all()


def test_paging_window_that_overhangs_the_end(paged):
    fm, ch, off, one_shot = paged
    d = DevAll(fm, ch, off, -1)
    d.fill(d.total - 1000, 1 << 40, at=0)   # far beyond the end: cut at hit_off[n]
    d.fill(d.total, 77, at=2000)            # starts at the end: nothing
    d.fill(d.total + 5, 1 << 62, at=2000)   # starts beyond it: nothing
    locs = d.result()[0]
    assert (locs[:1000] == one_shot[0][d.total - 1000:d.total]).all() and (locs[1000:] == SENT).all()


@pytest.fixture(scope="module")
def synth():
    text = ia.synth_log(1 << 21)
    t16 = ia.as_chars(text)
    fm = ia.FmIndex(text, 16, True, device=0, build_device=0)
    o = orc.OracleFmIndex.read(fm.write(False))
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in np.unique(t16)])
    off = off.astype(np.int32)
    exp = expected_packed("synth21", o, ch, off, -1)
    assert int(exp[1][-1]) == len(t16)  # 2 M packed hits
    yield fm, ch, off, exp
    fm.close()


_SHAPE_STEPS = {}


@pytest.mark.parametrize("block,groups", SHAPES)
def test_launch_shapes(synth, block, groups):
    fm, ch, off, exp = synth
    total = int(exp[1][-1])
    if groups == 1:  # one workgroup per CU: the grid-stride loop over the tiles runs at least three times
        assert (total + TILE - 1) // TILE >= 3 * n_cu()
    with options(block=block, groups_per_cu=groups):
        res = dev_all(fm, ch, off, -1)
        host = host_all(fm, ch, off, -1)
    check(res, exp, "block %d groups_per_cu %d, device form" % (block, groups))
    check(host, exp, "block %d groups_per_cu %d, host form" % (block, groups))
    first = _SHAPE_STEPS.setdefault("lf", res[3])
    assert (res[3] == first).all() and (host[3] == first).all()  # LF-steps per pattern, equal between shapes


def test_empty_batch_and_batch_without_hits(paged):
    fm = paged[0]
    torch = _torch()
    hit_off = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
    rc = ia.lib.fmx_locate_all_ranges_dev(fm.handle, None, None, 0, -1, hit_off.data_ptr(), None, None, None,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and int(hit_off.cpu()[0]) == 0
    h = np.full(1, SENT, np.int64)
    buf = C.c_void_p(0x1234)
    assert ia.lib.fmx_locate_all_batch(fm.handle, None, None, 0, -1, h.ctypes.data, C.byref(buf), None, None) == 0
    assert h[0] == 0 and buf.value is None
    ch, off = ia.pack_patterns(["zzzzqq#", "", "qqqqzz#"])
    locs, hit_off, st = fm.locate_all_batch(ch, off.astype(np.int32))
    assert len(locs) == 0 and (hit_off == 0).all() and list(st) == [0, 9, 0]
    bad = np.array([0, 3, 2, 4], np.int32)  # offsets that decrease: the host form's check
    assert ia.lib.fmx_locate_all_batch(fm.handle, ch.ctypes.data, bad.ctypes.data, 3, -1, np.zeros(4, np.int64).ctypes.data, C.byref(buf),
                                       None, None) == ia._lib.E_ARG


def test_mirrors(hd, paged, tmp_path):
    t16, o, ch, off = hd
    fm = paged[0]
    n, want = o.locate(ia.as_chars("INFO"), max_matches=-1, cap=4000)
    assert n == 1920
    got = fm.locate_all("INFO")
    assert got.dtype == np.int32 and (got == want).all()
    assert (fm.locate_all("xxINFOxx", offset=2, length=4) == want).all()
    assert (fm.locate_all("INFO", maxMatches=7) == want[:7]).all()
    with pytest.raises(IndexError):
        fm.locate_all("")
    # the C++ mirror: tests/cpp/test_locate_all_mirror.cpp prints what locateAllBatch / locateAll return
    exe = str(tmp_path / "test_locate_all_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_locate_all_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    nb, blk = o.locate(ia.as_chars("blk_"), max_matches=-1, cap=20000)
    assert out["batch_offsets"] == [0, 1920, 1920, 1920 + nb] and out["batch_locations"] == list(want) + list(blk)  # {"INFO", absent, "blk_"}
    assert out["cut_offsets"] == [0, 7, 7, 14] and out["cut_locations"] == list(want[:7]) + list(blk[:7])           # ... maxMatches 7
    assert out["all"] == list(want)                                                                                 # locateAll("INFO")

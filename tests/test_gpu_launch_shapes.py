"""Every query kernel at every launch shape, against the oracle.

Each kernel behind `grid_for` is compiled for 512- and 1024-lane workgroups (option "block") and grid-strides whatever its grid of
n_cu * "groups_per_cu" workgroups does not cover.  The rest of the suite runs the default 512 x 16, where its batches end in one
pass.  Here every query kind runs at (block, groups_per_cu) in (512, 1), (1024, 1), (512, 16), (1024, 16): with one workgroup per
CU the batches below are sized from the device's CU count so that every checked launch runs its grid-stride loop at least three
times (asserted: a change that made them too small fails instead of quietly leaving the loops untested), and that LDS reused
across iterations, `__syncthreads_or` rounds, per-wave ticket runs, scratch windows sized per grid lane and the halved grid of
uniform planned batches all see second and third passes.  The shapes run small grid -> large grid, 512 -> 1024, on indexes made
resident once: scratch the library cached for one shape must serve the next one too.

Every output is prefilled with a sentinel no kernel writes (device buffers, through the `_dev` entry points), whole arrays are
compared with the oracle (tests/orc.py, 16 threads; an answer does not depend on the launch shape, so the oracle runs once per
input), and the per-item LF-steps of a leg with those of its first run on the same inputs (the oracle batch does not return them).
The plan-stage knobs that change only the ORDER of work (coarse_bits, sort_bits, plan_fine, walk_fine, count_halve_uniform,
plan_fused) run at the default shape and at (512, 1).  Every option is put back in `finally`."""
import contextlib
import ctypes as C
import random

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text

pytestmark = pytest.mark.gpu

THREADS = 16
SHAPES = [(512, 1), (1024, 1), (512, 16), (1024, 16)]  # small grid -> large grid, 512 -> 1024
DEFAULT_SHAPE, FULL_SHAPE = (512, 16), (1024, 1)
SENT = -0x3C3C3C3D  # int32 outputs: no count, status, step count, position, length or aux the kernels write
SENT16 = 0xFFFE  # rows of characters: a noncharacter no test text holds
SR = 16  # sample rate of the synthetic indexes

# the value every option this module sets goes back to: FMX_OPTIONS' if it set one, else the library's default — except the four
# the suite's autouse fixture (conftest.py) holds at its own values for the length of every GPU test
LIB_DEFAULTS = {
    "block": 512, "groups_per_cu": 16, "sort_min": 16384, "count_lean": 0, "map_fast": 1, "window_cells": 2, "image_compact": 0,
    "walk_queue": 8, "walk_pack": 1, "walk_burst": 0, "boundary_group": 4, "boundary_narrow": 0, "boundary_narrow_min": 4096,
    "boundary_rounds": 1, "boundary_accel": 1, "coarse_bits": 12, "sort_bits": 28, "plan_fine": 1, "walk_fine": 1,
    "count_halve_uniform": 1, "plan_fused": 0, "host_pipeline_chunk": 262144,
    "plan_min_per_string": 0, "plan_sa_min": 0, "walk_order_min": 1, "boundary_order_min": 1,  # (conftest.py's values)
}


def _back(name):
    return ia._lib.ENV_OPTIONS.get(name, LIB_DEFAULTS[name])


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
        yield
    finally:
        for k in kw:
            ia.lib.fmx_set_option(k.encode(), _back(k))


def shape_opts(shape):
    return {"block": shape[0], "groups_per_cu": shape[1]}


# ---- device buffers -------------------------------------------------------------------------------------------------------------

def _torch():
    import torch

    return torch


def d_i32(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def d_i64(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def d_u16(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def d_sent(n, dtype="int32"):
    torch = _torch()
    if dtype == "u16":
        return torch.full((max(n, 1),), SENT16 - 0x10000, dtype=torch.int16, device="cuda")
    return torch.full((max(n, 1),), SENT, dtype=getattr(torch, dtype), device="cuda")


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def host(t, n=None, u16=False):
    _torch().cuda.synchronize()
    a = t.cpu().numpy()
    if n is not None:
        a = a[:n]
    return a.view(np.uint16) if u16 else a


def ok(rc, what):
    assert rc == 0, "%s: %s" % (what, (ia.lib.fmx_last_error() or b"").decode())


# ---- grid arithmetic (as grid_for in fmx_kernels.hip) ----------------------------------------------------------------------------

def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def grid_for(lanes, block, gpc):
    return max(1, min(-(-lanes // block), n_cu() * gpc))


def passes(items, lanes_per_item, shape, per_lane=1, halve=False):
    """passes of a grid-stride loop over items * lanes_per_item lanes' worth of work, a lane taking per_lane of them per pass"""
    block, gpc = shape
    work = items * lanes_per_item
    grid = grid_for(-(-work // per_lane), block, gpc)
    if halve and grid >= 2:
        grid = (grid + 1) // 2
    return -(-work // (grid * block * per_lane))


def assert_loops(what, shape, items, lanes_per_item, per_lane=1, halve=False, at_least=3):
    if shape[1] != 1:
        return
    p = passes(items, lanes_per_item, shape, per_lane, halve)
    assert p >= at_least, "%s at %r: %d items run %d pass(es) of the grid-stride loop, want >= %d" % (what, shape, items, p, at_least)


def full_lanes():
    return n_cu() * 1024  # lanes of the largest one-workgroup-per-CU grid


# ---- the indexes and inputs, made once -----------------------------------------------------------------------------------------

class World:
    pass


def _patterns(t16, rnd, n, lo, hi, absent_every=0):
    L = len(t16)
    starts = [rnd.randrange(L - hi - 1) for _ in range(n)]
    pats = [t16[s:s + rnd.randrange(lo, hi + 1)] for s in starts]
    if absent_every:
        for k in range(0, n, absent_every):
            pats[k] = pats[k].copy()
            pats[k][0] = 0x7A7B  # a character no text holds, met last
    return pats


def _pack(pats, empty=False):
    ch, off = ia.pack_patterns(pats)
    if empty:  # + an empty pattern: AIOOBE (FM:456-457)
        off = np.concatenate([off, [off[-1]]])
    return np.ascontiguousarray(ch), off.astype(np.int32)


@pytest.fixture(scope="module")
def world():
    w = World()
    rnd = random.Random(2026)
    L = full_lanes()
    w.text = ia.synth_log(1 << 21)  # ~2 MiB
    t16 = w.text
    n = len(t16)
    w.fms = {}
    try:
        for name, opts in (("flat", {}), ("cells", {"window_cells": 1}), ("none", {"window_cells": 0}),
                           ("compact", {"image_compact": 1}), ("slow", {"map_fast": 0})):
            with options(**opts):
                w.fms[name] = ia.FmIndex(w.text, SR, True, device=0)
        assert w.fms["none"].window_cells_bytes() == 0 < w.fms["cells"].window_cells_bytes() < 4 * n
        assert w.fms["flat"].window_cells_bytes() >= 4 * n  # the flat form: a word per position
        w.o = orc.OracleFmIndex(w.text, SR, True)
        # count: planned uniform length 8 (two pipeline chunks' worth for the host path), mixed lengths 1..30
        w.n_count = -(-3 * L // 2) + 1000
        w.uni = _pack(_patterns(t16, rnd, 2 * w.n_count, 8, 8, absent_every=97))
        w.mix = _pack(_patterns(t16, rnd, w.n_count, 1, 30, absent_every=89), empty=True)
        w.uni_exp = w.o.count_batch(*w.uni, threads=THREADS)
        w.mix_exp = w.o.count_batch(*w.mix, threads=THREADS)
        # locate: 8 lanes' worth of tickets per pattern at least
        w.n_loc = -(-3 * L // 8) + 3000
        w.loc = _pack(_patterns(t16, rnd, w.n_loc, 5, 12, absent_every=101), empty=True)  # (+ margin: patterns without a hit take one ticket)
        w.loc_exp = {mm: w.o.locate_batch(*w.loc, mm, mm, threads=THREADS, fill=SENT) for mm in (8, 64)}
        assert (w.loc_exp[64][1] > 8).mean() > 0.3  # many patterns with more hits than 8 slots
        # extract: rows that run into both ends of the text, stops before starts, out of range
        w.n_ext = 3 * L + 500
        r = np.random.default_rng(7)
        st = r.integers(0, n, w.n_ext).astype(np.int32)
        ln = r.integers(0, 40, w.n_ext).astype(np.int32)
        sp = np.minimum(st.astype(np.int64) + ln, n + 2).astype(np.int32)
        st[:64], sp[:64] = np.arange(64) // 3, np.arange(64) // 3 + 30  # the start of the text
        st[64:128], sp[64:128] = n - 64 + np.arange(64), n  # its end
        st[128:140], sp[128:140] = n - 10, n + 1 + np.arange(12)  # past it
        st[140:150], sp[140:150] = -1 - np.arange(10), 5
        st[150:160], sp[150:160] = 100, 90  # stop before start
        w.ext = (st, sp)
        w.ext_len, w.ext_off = 32, 3
        w.ext_exp = w.o.extract_batch(st, sp, w.ext_len, w.ext_off, threads=THREADS, fill=SENT16)
        # extractUntilBoundary: words (' ', a query per lane needs 3 x the grid), lines ('\n', the group of four needs a quarter)
        w.n_bnd = 3 * L + 500
        fr = r.integers(0, n, w.n_bnd).astype(np.int32)
        fr[:6] = [-1, 0, 1, n - 2, n - 1, n]
        w.bnd = fr
        w.bnd_len, w.bnd_off = 24, 2
        w.bnd_exp = {m: w.o.extract_until_boundary_batch(m, fr, " ", w.bnd_len, w.bnd_off, threads=THREADS, fill=SENT16)
                     for m in (0, 1, 2)}
        assert all(0.05 < (w.bnd_exp[m][2] == 8).mean() < 0.9 for m in (0, 1, 2))  # capped rows AND rows that fit
        w.n_lines = -(-3 * L // 4) + 500
        w.lines = fr[:w.n_lines].copy()
        w.lines_len = 160
        w.lines_exp = {m: w.o.extract_until_boundary_batch(m, w.lines, "\n", w.lines_len, 0, threads=THREADS, fill=SENT16)
                       for m in (0, 1, 2)}
        assert (w.lines_exp[0][2] == 0).mean() > 0.5
        # 12- and 16-bit plan codes; the reference's fixture at a sample rate that is no power of two
        w.wide = {}
        for bits, symbols in ((12, 700), (16, 5000)):
            t = ia.synth_log_multichar(1 << 18, symbols=symbols, seed=bits)
            fm = ia.FmIndex(t, SR, True, device=0)
            o = orc.OracleFmIndex(t, SR, True)
            batch = _pack(_patterns(t, rnd, w.n_count, 1, 30, absent_every=83), empty=True)
            w.wide[bits] = (fm, batch, o.count_batch(*batch, threads=THREADS))
        assert w.wide[12][0].getAlphabetLength() <= 4096 < w.wide[16][0].getAlphabetLength()
        hd = ia.as_chars(hdfs_text())
        w.hd = ia.FmIndex(hd, 12, True, device=0)
        w.hd_o = orc.OracleFmIndex(hd, 12, True)
        w.hd_loc = _pack(_patterns(hd, rnd, w.n_loc, 2, 10, absent_every=71), empty=True)
        w.hd_loc_exp = w.hd_o.locate_batch(*w.hd_loc, 8, 8, threads=THREADS, fill=SENT)
        w.hd_cnt_exp = w.hd_o.count_batch(*w.hd_loc, threads=THREADS)
        w.steps = {}  # leg -> per-item LF-steps of its first run
        yield w
    finally:
        for fm in list(w.fms.values()) + [x[0] for x in getattr(w, "wide", {}).values()] + [getattr(w, "hd", None)]:
            if fm is not None:
                fm.close()


def same_steps(w, leg, steps):
    assert (steps != SENT).all(), "%s: LF-steps not written for every item" % leg
    first = w.steps.setdefault(leg, steps)
    if first is not steps:
        bad = np.flatnonzero(first != steps)
        assert len(bad) == 0, "%s: LF-steps differ from the first run's at %d items (first %r)" % (leg, len(bad), bad[:5])


# ---- one call of each kind over device buffers prefilled with the sentinel -------------------------------------------------------

def run_count(fm, batch, n=None):
    ch, off = batch
    n = len(off) - 1 if n is None else n
    d_ch, d_off = d_u16(ch), d_i32(off[:n + 1])
    cnt, lf, st = d_sent(n), d_sent(n), d_sent(n)
    ok(ia.lib.fmx_count_batch_dev(fm.handle, d_ch.data_ptr(), d_off.data_ptr(), n, cnt.data_ptr(), lf.data_ptr(), st.data_ptr(),
                                  stream()), "fmx_count_batch_dev")
    return host(cnt, n), host(st, n), host(lf, n)


def check_count(w, leg, fm, batch, exp, n=None):
    """n: the batch's first n patterns only (their LF-steps then match those of the whole batch's first run)"""
    c, st, lf = run_count(fm, batch, n)
    k = len(c)
    bad = np.flatnonzero((c != exp[0][:k]) | (st != exp[1][:k]))
    assert len(bad) == 0, "%s: %d of %d patterns differ from the oracle, first %r" % (leg, len(bad), k, bad[:5])
    if n is None:
        same_steps(w, leg, lf)
    else:
        assert (lf == w.steps[leg][:n]).all(), "%s: LF-steps of the first %d patterns differ" % (leg, n)


def run_locate(fm, batch, mm):
    ch, off = batch
    n = len(off) - 1
    d_ch, d_off = d_u16(ch), d_i32(off)
    locs, found, lf, st, rng = d_sent(n * mm), d_sent(n), d_sent(n), d_sent(n), d_sent(2 * n)
    ok(ia.lib.fmx_locate_batch_dev(fm.handle, d_ch.data_ptr(), d_off.data_ptr(), n, mm, locs.data_ptr(), mm, found.data_ptr(),
                                   lf.data_ptr(), st.data_ptr(), rng.data_ptr(), stream()), "fmx_locate_batch_dev")
    return host(locs, n * mm).reshape(n, mm), host(found, n), host(st, n), host(lf, n)


def check_locate(w, leg, fm, batch, mm, exp):
    locs, found, st, lf = run_locate(fm, batch, mm)
    ol, of, ost = exp
    bad = np.flatnonzero((found != of) | (st != ost) | (locs != ol).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d patterns differ from the oracle (whole rows), first %r" % (leg, len(bad), len(found), bad[:5])
    same_steps(w, leg, lf)


def check_extract(w, leg, fm):
    st_, sp_ = w.ext
    n = len(st_)
    d_st, d_sp = d_i32(st_), d_i32(sp_)
    dst, ol, lf, st = d_sent(n * w.ext_len, "u16"), d_sent(n), d_sent(n), d_sent(n)
    ok(ia.lib.fmx_extract_batch_dev(fm.handle, d_st.data_ptr(), d_sp.data_ptr(), n, dst.data_ptr(), w.ext_len, w.ext_off,
                                    ol.data_ptr(), lf.data_ptr(), st.data_ptr(), stream()), "fmx_extract_batch_dev")
    dst, ol, st, lf = host(dst, n * w.ext_len, u16=True).reshape(n, w.ext_len), host(ol, n), host(st, n), host(lf, n)
    od, oo, ost = w.ext_exp
    bad = np.flatnonzero((ol != oo) | (st != ost) | (dst != od).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d rows differ from the oracle, first %r" % (leg, len(bad), n, bad[:5])
    same_steps(w, leg, lf)


def check_boundary(w, leg, fm, froms, boundary, mode, dst_len, offset, exp):
    n = len(froms)
    d_fr = d_i32(froms)
    dst, ol, lf, st, aux = d_sent(n * dst_len, "u16"), d_sent(n), d_sent(n), d_sent(n), d_sent(n)
    ok(ia.lib.fmx_extract_boundary_batch_dev(fm.handle, d_fr.data_ptr(), n, ord(boundary), mode, dst.data_ptr(), dst_len, offset,
                                             ol.data_ptr(), lf.data_ptr(), st.data_ptr(), aux.data_ptr(), stream()),
       "fmx_extract_boundary_batch_dev")
    dst, ol, st, aux, lf = (host(dst, n * dst_len, u16=True).reshape(n, dst_len), host(ol, n), host(st, n), host(aux, n),
                            host(lf, n))
    od, oo, ost, oaux = exp
    capped = ost == 8
    bad = np.flatnonzero((ol != oo) | (st != ost) | (dst != od).any(axis=1) | (capped & (aux != oaux)))
    assert len(bad) == 0, "%s mode %d: %d of %d rows differ from the oracle, first %r" % (leg, mode, len(bad), n, bad[:5])
    assert (aux != SENT).all(), "%s mode %d: aux not written for every query" % (leg, mode)
    same_steps(w, "%s/%d" % (leg, mode), lf)


# ---- count ----------------------------------------------------------------------------------------------------------------------

def _odd_batch(w, shape):
    """a planned uniform batch for which grid_for gives an ODD block count: the halved grid is (blocks + 1) / 2"""
    block, gpc = shape
    k = min(n_cu() * gpc, -(-2 * w.n_count // block))
    k -= 1 - k % 2
    n = block // 2 * k
    assert grid_for(2 * n, block, gpc) % 2 == 1 and 16384 <= n <= 2 * w.n_count
    return n


def count_legs(w, shape, full):
    fm = w.fms["flat"]
    n_uni = 2 * w.n_count
    assert ia.lib.fmx_count_batch_is_planned(fm.handle, n_uni) == 1
    assert_loops("count uniform", shape, n_uni, 2, halve=True)
    check_count(w, "count/uniform8", fm, w.uni, w.uni_exp)
    n_odd = _odd_batch(w, shape)
    assert_loops("count uniform, odd grid", shape, n_odd, 2, halve=True, at_least=2)  # (an odd grid halved runs two passes)
    check_count(w, "count/uniform8", fm, w.uni, w.uni_exp, n=n_odd)
    assert_loops("count mixed", shape, w.n_count, 2)
    check_count(w, "count/mixed", fm, w.mix, w.mix_exp)
    if not full:
        return
    with options(sort_min=w.n_count + 10):
        assert ia.lib.fmx_count_batch_is_planned(fm.handle, w.n_count + 1) == 0
        check_count(w, "count/unplanned", fm, w.mix, w.mix_exp)
    with options(count_lean=1):
        check_count(w, "count/lean", fm, w.mix, w.mix_exp)
        check_count(w, "count/lean-uniform", fm, w.uni, w.uni_exp)
        check_count(w, "count/lean-list", w.fms["slow"], w.mix, w.mix_exp)  # map_fast = 0: the whole batch on the redo list
    check_count(w, "count/slow", w.fms["slow"], w.mix, w.mix_exp)
    for form in ("cells", "none", "compact"):
        check_count(w, "count/mixed-" + form, w.fms[form], w.mix, w.mix_exp)
        check_count(w, "count/uniform8-" + form, w.fms[form], w.uni, w.uni_exp)
    for bits, (wfm, batch, exp) in w.wide.items():
        check_count(w, "count/bits%d" % bits, wfm, batch, exp)
        with options(sort_min=w.n_count + 10):
            check_count(w, "count/bits%d-unplanned" % bits, wfm, batch, exp)
        with options(count_lean=1):
            check_count(w, "count/bits%d" % bits, wfm, batch, exp)
    # the host-array path: two pipelined chunks of n_count patterns
    assert_loops("count host chunk", shape, w.n_count, 2, halve=True)
    with options(host_pipeline_chunk=n_uni // 2):
        c, st, lf = fm.count_batch(*w.uni, want_steps=True)
    assert (c == w.uni_exp[0]).all() and (st == w.uni_exp[1]).all(), "count/host"
    same_steps(w, "count/uniform8", lf)


def test_count_every_shape(world):
    """count: planned uniform (the halved grid, an odd grid among them), planned mixed lengths (regrouping), the caller's order,
    k_count_lean with a non-empty redo list (k_count's list mode), 12- and 16-bit plan codes, every directory form, the host path"""
    for shape in SHAPES:
        with options(**shape_opts(shape)):
            count_legs(world, shape, full=shape in (FULL_SHAPE, DEFAULT_SHAPE))


# ---- locate ---------------------------------------------------------------------------------------------------------------------

def locate_legs(w, shape, full):
    forms = ("flat", "cells", "none", "compact") if full else ("flat",)
    for form in forms:
        fm = w.fms[form]
        k8, k64 = "locate/8/" + form, "locate/64/" + form  # (a hit's walk is the same whichever kernel form walks it)
        assert_loops("locate cap 8", shape, w.n_loc, 8)
        check_locate(w, k8, fm, w.loc, 8, w.loc_exp[8])
        # (the ticket queue hands a lane 8 tickets per run: the bound of every form)
        assert_loops("locate cap 64 (ticket queue)", shape, w.n_loc, 64, per_lane=8)
        check_locate(w, k64, fm, w.loc, 64, w.loc_exp[64])
        if not full:
            continue
        for pack in (0, 2, 3):
            with options(walk_queue=0, walk_pack=pack):
                check_locate(w, k64, fm, w.loc, 64, w.loc_exp[64])
                check_locate(w, k8, fm, w.loc, 8, w.loc_exp[8])
        with options(walk_burst=1):
            check_locate(w, k64, fm, w.loc, 64, w.loc_exp[64])
        with options(walk_order_min=0):  # the caller's order
            check_locate(w, k8, fm, w.loc, 8, w.loc_exp[8])
            check_locate(w, k64, fm, w.loc, 64, w.loc_exp[64])
    # the reference's fixture (2,061 symbols) at sample rate 12
    check_locate(w, "locate/hdfs", w.hd, w.hd_loc, 8, w.hd_loc_exp)


def test_locate_every_shape(world):
    """locate: the packed walk (cap 8), the ticket queue (cap 64), walk_queue 0 with walk_pack 0 / 2 / 3, walk_burst 1, hits
    walked by SA row and in the caller's order — over the flat and cells directory, none, and the compact image"""
    for shape in SHAPES:
        with options(**shape_opts(shape)):
            locate_legs(world, shape, full=shape in (FULL_SHAPE, DEFAULT_SHAPE))


# ---- extract and extractUntilBoundary -------------------------------------------------------------------------------------------

def test_extract_every_shape(world):
    """extract over every directory form and the compact image: rows that run into both ends of the text, and out of it"""
    w = world
    for shape in SHAPES:
        assert_loops("extract", shape, w.n_ext, 1)
        with options(**shape_opts(shape)):
            for form in (("flat", "cells", "none", "compact") if shape in (FULL_SHAPE, DEFAULT_SHAPE) else ("flat", "none")):
                check_extract(w, "extract/" + form, w.fms[form])


def boundary_legs(w, shape, full):
    fm = w.fms["flat"]
    for mode in (0, 1, 2):
        assert_loops("extractUntilBoundary G=4", shape, w.n_bnd, 4)
        check_boundary(w, "bnd/g4", fm, w.bnd, " ", mode, w.bnd_len, w.bnd_off, w.bnd_exp[mode])
        assert_loops("extractUntilBoundary lines G=4", shape, w.n_lines, 4)
        check_boundary(w, "lines/g4", fm, w.lines, "\n", mode, w.lines_len, 0, w.lines_exp[mode])
    if not full:
        return
    for mode in (0, 1, 2):
        exp = w.bnd_exp[mode]
        for g in (0, 1, 2, 8, 16):
            with options(boundary_group=g):
                assert_loops("extractUntilBoundary G=%d" % g, shape, w.n_bnd, max(g, 1))
                check_boundary(w, "bnd/g%d" % g, fm, w.bnd, " ", mode, w.bnd_len, w.bnd_off, exp)
        with options(boundary_narrow=1, boundary_narrow_min=1):
            assert_loops("extractUntilBoundary narrow round", shape, w.n_bnd, 2)
            check_boundary(w, "bnd/narrow", fm, w.bnd, " ", mode, w.bnd_len, w.bnd_off, exp)
        with options(boundary_rounds=0):
            check_boundary(w, "bnd/g4-rounds0", fm, w.bnd, " ", mode, w.bnd_len, w.bnd_off, exp)
            check_boundary(w, "lines/g4-rounds0", fm, w.lines, "\n", mode, w.lines_len, 0, w.lines_exp[mode])
        with options(boundary_accel=0):  # the literal form: a lane per query, no scratch
            assert_loops("extractUntilBoundary literal", shape, w.n_bnd, 1)
            check_boundary(w, "bnd/literal", fm, w.bnd, " ", mode, w.bnd_len, w.bnd_off, exp)
        with options(boundary_order_min=0):  # the caller's order
            check_boundary(w, "bnd/g4", fm, w.bnd, " ", mode, w.bnd_len, w.bnd_off, exp)
        for form in ("cells", "none", "compact"):
            check_boundary(w, "bnd/g4/" + form, w.fms[form], w.bnd, " ", mode, w.bnd_len, w.bnd_off, exp)
            check_boundary(w, "lines/g4/" + form, w.fms[form], w.lines, "\n", mode, w.lines_len, 0, w.lines_exp[mode])


def test_extract_until_boundary_every_shape(world):
    """extractUntilBoundary modes 0 / 1 / 2: groups of 0 / 1 / 2 / 4 / 8 / 16 lanes, the narrow first round, the fill without
    rounds, the literal form, the caller's order, every directory form; words (many rows capped: status 8 and its aux) and lines"""
    for shape in SHAPES:
        with options(**shape_opts(shape)):
            boundary_legs(world, shape, full=shape in (FULL_SHAPE, DEFAULT_SHAPE))


# ---- the fused pipelines --------------------------------------------------------------------------------------------------------

def test_fused_pipelines_every_shape(world):
    """locate -> extract and locate -> extractUntilBoundary with the hits kept in HBM: every array against the oracle's locate
    followed by its extract / extractUntilBoundary of each hit"""
    w = world
    fm = w.fms["flat"]
    ch, off = w.loc
    n, mm, ext_len, line_len = len(off) - 1, 8, 20, 48
    ol, of, ost = w.loc_exp[mm]
    live = np.arange(mm)[None, :] < of[:, None]
    hits = ol[live]
    stops = np.minimum(hits.astype(np.int64) + ext_len, fm.getInputLength()).astype(np.int32)
    e_dst, e_len, e_st = w.o.extract_batch(hits, stops, ext_len, 0, threads=THREADS, fill=SENT16)
    b_exp = {m: w.o.extract_until_boundary_batch(m, hits, "\n", line_len, 0, threads=THREADS, fill=SENT16) for m in (0, 1, 2)}
    d_ch, d_off = d_u16(ch), d_i32(off)
    for shape in SHAPES:
        with options(**shape_opts(shape)):
            assert_loops("pipeline extract stage", shape, n, mm)
            for mode in (-1, 0, 1, 2):
                row = ext_len if mode < 0 else line_len
                locs, found, lf, st = d_sent(n * mm), d_sent(n), d_sent(n), d_sent(n)
                dst, out_len, hst, haux, rng = d_sent(n * mm * row, "u16"), d_sent(n * mm), d_sent(n * mm), d_sent(n * mm), d_sent(2 * n)
                if mode < 0:
                    ok(ia.lib.fmx_locate_extract_batch_dev(fm.handle, d_ch.data_ptr(), d_off.data_ptr(), n, mm, ext_len,
                                                           locs.data_ptr(), found.data_ptr(), dst.data_ptr(), out_len.data_ptr(),
                                                           lf.data_ptr(), st.data_ptr(), hst.data_ptr(), rng.data_ptr(), stream()),
                       "fmx_locate_extract_batch_dev")
                    xd, xl, xs, xa = e_dst, e_len, e_st, None
                else:
                    ok(ia.lib.fmx_locate_lines_batch_dev(fm.handle, d_ch.data_ptr(), d_off.data_ptr(), n, mm, ord("\n"), mode, line_len,
                                                         locs.data_ptr(), found.data_ptr(), dst.data_ptr(), out_len.data_ptr(),
                                                         lf.data_ptr(), st.data_ptr(), hst.data_ptr(), haux.data_ptr(), rng.data_ptr(),
                                                         stream()), "fmx_locate_lines_batch_dev")
                    xd, xl, xs, xa = b_exp[mode]
                leg = "pipeline/%d" % mode
                g_locs = host(locs, n * mm).reshape(n, mm)
                assert (host(found, n) == of).all() and (host(st, n) == ost).all() and (g_locs == ol).all(), leg
                g_dst = host(dst, n * mm * row, u16=True).reshape(n, mm, row)
                g_len, g_hst = host(out_len, n * mm).reshape(n, mm), host(hst, n * mm).reshape(n, mm)
                assert (g_dst[live] == xd).all() and (g_len[live] == xl).all() and (g_hst[live] == xs).all(), leg
                # slots past `found` keep what was there
                assert (g_dst[~live] == SENT16).all() and (g_len[~live] == SENT).all(), leg
                if xa is not None:
                    g_aux = host(haux, n * mm).reshape(n, mm)[live]
                    assert (g_aux[xs == 8] == xa[xs == 8]).all(), leg
                same_steps(w, leg, host(lf, n))


# ---- segment sets of mixed alphabet sizes ---------------------------------------------------------------------------------------

def test_segment_set_foreign_plans_every_shape(world):
    """count + locate over segments of 8-bit, 16-bit and 8-bit codes in ONE pass: the plan is made with segment 0, translated for
    segment 2 (k_count mode 2) and taken for its order only in segment 1 (mode 3) — at every shape, against one oracle per segment"""
    w = world
    rnd = random.Random(31)
    n_seg = 60_000
    ascii_a = np.array([rnd.randrange(97, 123) if rnd.random() < 0.93 else 10 for _ in range(n_seg)], dtype=np.uint16)
    wide = np.array([rnd.randrange(0x400, 0x400 + 600) if rnd.random() < 0.5 else rnd.randrange(97, 123) for _ in range(n_seg)],
                    dtype=np.uint16)
    wide[::50] = 10
    ascii_b = np.array([rnd.randrange(97, 110) if rnd.random() < 0.9 else 10 for _ in range(n_seg)], dtype=np.uint16)
    parts = [ascii_a, wide, ascii_b]
    segs = [ia.FmIndex(t, SR, True, device=0) for t in parts]
    try:
        assert segs[0].getAlphabetLength() <= 256 < segs[1].getAlphabetLength() and segs[2].getAlphabetLength() <= 256
        bases = np.cumsum([0] + [len(t) for t in parts[:-1]]).astype(np.int64)
        sf = ia.SegmentedFmIndex.from_segments(segs, bases)
        oracles = [orc.OracleFmIndex(t, SR, True) for t in parts]
        n, mm = w.n_count, 5
        pats = []
        for i in range(n):
            t = parts[i % 3]
            s0 = rnd.randrange(len(t) - 20)
            pats.append(t[s0:s0 + rnd.randrange(2, 20)])
        ch, off = _pack(pats)
        exp_cnt = np.zeros(n, np.int64)
        cols, valid = [], []
        for o, base in zip(oracles, bases):
            c, s = o.count_batch(ch, off, threads=THREADS)
            assert (s == 0).all()
            exp_cnt += c
            ol, of, _ = o.locate_batch(ch, off, mm, mm, threads=THREADS)
            cols.append(ol.astype(np.int64) + int(base))
            valid.append(np.arange(mm)[None, :] < of[:, None])
        allv, allc = np.concatenate(valid, axis=1), np.concatenate(cols, axis=1)
        order = np.argsort(~allv, axis=1, kind="stable")[:, :mm]  # the segments' hits in segment order, the first mm
        exp_found = np.minimum(allv.sum(axis=1), mm)
        exp_locs = np.where(np.arange(mm)[None, :] < exp_found[:, None], np.take_along_axis(allc, order, axis=1), SENT)
        d_ch, d_off = d_u16(ch), d_i32(off)
        d_base = bases.copy()
        for shape in SHAPES:
            assert_loops("segment count", shape, n, 2)
            with options(**shape_opts(shape)):
                cnt, lf, locs = d_sent(n, "int64"), d_sent(n, "int64"), d_sent(n * mm, "int64")
                found, st, tmp = d_sent(n), d_sent(n), d_sent(n * (4 + mm))
                ok(ia.lib.fmx_count_locate_segments_dev(sf.handles, len(segs), d_base.ctypes.data, d_ch.data_ptr(), d_off.data_ptr(),
                                                        n, mm, cnt.data_ptr(), lf.data_ptr(), locs.data_ptr(), found.data_ptr(),
                                                        st.data_ptr(), tmp.data_ptr(), stream()), "fmx_count_locate_segments_dev")
                assert (host(cnt, n) == exp_cnt).all() and (host(st, n) == 0).all(), shape
                assert (host(found, n) == exp_found).all() and (host(locs, n * mm).reshape(n, mm) == exp_locs).all(), shape
                same_steps(w, "segments", host(lf, n))
    finally:
        for s in segs:
            s.close()


# ---- the stand-alone wavelet tree and RRR vector -------------------------------------------------------------------------------

def test_standalone_wavelet_and_rrr_every_shape(world):
    """k_wt_rank, k_wt_inverse_select, k_rrr_rank_ones and k_rrr_access against the oracle (and, for the RRR vector, the bits and
    their prefix sum themselves)"""
    n_q = 3 * full_lanes() + 100
    rng = np.random.default_rng(11)
    seq = rng.integers(0, 2000, 300_000).astype(np.int16)
    wt = ia.WaveletFixedBlockBoosting(seq, 16)
    ow = orc.Wfbb(seq, 16)
    pos = rng.integers(0, len(seq) + 1, n_q).astype(np.int64)
    pos[:4] = [0, 1, len(seq), len(seq) + 7]
    sym = rng.integers(0, 2100, n_q).astype(np.int32)  # symbols past the alphabet too
    st = orc.C.c_int(0)
    exp_rank = np.zeros(n_q, np.int64)
    for i, (p, s) in enumerate(zip(pos.tolist(), sym.tolist())):
        exp_rank[i] = orc.lib().orc_wfbb_rank(ow.h, p, s, orc.C.byref(st))
        assert st.value == 0
    ipos = rng.integers(0, len(seq), n_q).astype(np.int64)
    exp_inv = np.array([ow.inverse_select(p) for p in ipos.tolist()], np.int64)
    bits = (rng.random(1_500_000) < 0.3).astype(np.uint8)
    rrr = ia.RrrVector(bits, 32)
    prefix = np.concatenate([[0], np.cumsum(bits)]).astype(np.int32)
    rpos = rng.integers(0, len(bits), n_q).astype(np.int32)
    rpos[:3] = [0, len(bits) - 1, len(bits)]
    orr = orc.Rrr(bits=bits, sample=32)
    exp_r1 = orr.rank_ones_batch(rpos, threads=THREADS)
    assert (exp_r1 == prefix[rpos]).all()
    d_rpos = d_i32(rpos)
    try:
        for shape in SHAPES:
            assert_loops("standalone kernels", shape, n_q, 1)
            with options(**shape_opts(shape)):
                out, stt = np.full(n_q, SENT, np.int64), np.full(n_q, SENT, np.int32)
                ok(ia.lib.fmx_wavelet_rank_batch(wt._h, pos.ctypes.data, sym.ctypes.data, n_q, out.ctypes.data, stt.ctypes.data),
                   "fmx_wavelet_rank_batch")
                assert (out == exp_rank).all() and (stt == 0).all(), shape
                out, stt = np.full(n_q, SENT, np.int64), np.full(n_q, SENT, np.int32)
                ok(ia.lib.fmx_wavelet_inverse_select_batch(wt._h, ipos.ctypes.data, n_q, out.ctypes.data, stt.ctypes.data),
                   "fmx_wavelet_inverse_select_batch")
                assert (out == exp_inv).all() and (stt == 0).all(), shape
                ranks = d_sent(n_q)
                ok(ia.lib.fmx_rrr_rank_ones_batch_dev(rrr._h, d_rpos.data_ptr(), n_q, ranks.data_ptr(), stream()),
                   "fmx_rrr_rank_ones_batch_dev")
                assert (host(ranks, n_q) == exp_r1).all(), shape
                torch = _torch()
                acc = torch.full((n_q,), 0xA5, dtype=torch.uint8, device="cuda")
                ast = d_sent(n_q)
                ok(ia.lib.fmx_rrr_access_batch_dev(rrr._h, d_rpos.data_ptr(), n_q, acc.data_ptr(), ast.data_ptr(), stream()),
                   "fmx_rrr_access_batch_dev")
                a, s = host(acc, n_q), host(ast, n_q)
                inside = rpos < len(bits)
                assert (a[inside] == bits[rpos[inside]]).all() and (s[inside] == 0).all() and (s[~inside] == 9).all(), shape
    finally:
        wt.close()
        rrr.close()


# ---- plan-stage knobs: the order of work changes, the answers do not ------------------------------------------------------------

KNOBS = [("coarse_bits", 4), ("coarse_bits", 13), ("sort_bits", 1), ("sort_bits", 9), ("sort_bits", 32), ("plan_fine", 0),
         ("plan_fine", 2), ("walk_fine", 0), ("count_halve_uniform", 0)]


def order_legs(w, tag):
    fm = w.fms["flat"]
    check_count(w, "count/uniform8", fm, w.uni, w.uni_exp)
    check_count(w, "count/mixed", fm, w.mix, w.mix_exp)
    check_locate(w, "locate/8/flat", fm, w.loc, 8, w.loc_exp[8])  # (walk_order_min = 1: walked by SA row)
    check_boundary(w, "bnd/g4", fm, w.bnd, " ", 0, w.bnd_len, w.bnd_off, w.bnd_exp[0])  # (boundary_order_min = 1: by position)


@pytest.mark.parametrize("knob,value", KNOBS, ids=["%s=%d" % kv for kv in KNOBS])
def test_plan_knobs_change_only_the_order(world, knob, value):
    """coarse_bits / sort_bits / plan_fine / walk_fine / count_halve_uniform: a planned count, an ordered locate and an ordered
    extractUntilBoundary at the default shape and at (512, 1), against the oracle and the LF-steps of the default settings"""
    for shape in (DEFAULT_SHAPE, (512, 1)):
        with options(**shape_opts(shape)):
            order_legs(world, shape)  # the default settings first: their LF-steps are what the knob's must match
            with options(**{knob: value}):
                order_legs(world, shape)


@pytest.mark.parametrize("shape", [(1024, 1), (1024, 16)], ids=["1024x1", "1024x16"])
def test_fused_plan_stage(world, shape):
    """plan_fused = 1: the plan stage as one launch with a grid barrier — at (1024, 1), where the whole grid is co-resident and the
    barrier completes, and at (1024, 16), where it may give up and leave the records in the caller's order"""
    tiles = -(-2 * world.n_count // 4096)
    assert tiles <= n_cu()  # (k_plan_fused runs only for batches of at most one tile per CU)
    with options(**shape_opts(shape)):
        order_legs(world, shape)
        with options(plan_fused=1):
            order_legs(world, shape)

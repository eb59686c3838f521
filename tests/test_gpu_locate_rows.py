"""The row table of a resident FmIndex (option "locate_rows": k_rows_fill / k_locate_rows of fmx_kernels.hip) on the GPU.

Every index is made resident twice — option 0 (locate walks, as always) and option 1 (a word per BWT row: locate gathers) — and
every entry point that locates runs on both over outputs prefilled with a sentinel: positions, found counts, statuses and LF-steps
must be equal element for element between the two AND equal to the oracle, which is the judge (tests/orc.py; its batch call
returns no per-pattern LF-steps, so those are compared as totals where no pattern overruns `locations`: there the reference
walks one hit more before it throws).  The option is set inside the tests and put back in `finally`."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import index4j_amd as ia
import orc
from index4j_amd import workload

pytestmark = pytest.mark.gpu

THREADS = 16
SENT = -0x3C3C3C3D
SHAPES = [(512, 1), (1024, 1), (512, 16), (1024, 16)]
DEFAULTS = {"locate_rows": 0, "rows_order": 0, "window_cells": 2, "window_cells_mb": 65536, "image_compact": 0, "block": 512,
            "groups_per_cu": 16}


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
        yield
    finally:
        for k in kw:
            ia.lib.fmx_set_option(k.encode(), ia._lib.ENV_OPTIONS.get(k, DEFAULTS[k]))


def _torch():
    import torch

    return torch


def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def patterns(t16, rng, n, lo, hi, absent_every=97):
    starts = rng.integers(0, len(t16) - hi - 1, n)
    lens = rng.integers(lo, hi + 1, n)
    pats = [t16[s:s + m] for s, m in zip(starts, lens)]
    for k in range(0, n, absent_every):
        pats[k] = pats[k].copy()
        pats[k][0] = 0x7A7B  # a character no text holds, met last
    ch, off = ia.pack_patterns(pats)
    off = np.concatenate([off, [off[-1]]]).astype(np.int32)  # + an empty pattern: AIOOBE (FM:456-457)
    return np.ascontiguousarray(ch), off


def run_block_text():
    """the text of tests/test_window_cells.py::test_large_alphabet_with_run_blocks_of_wide_symbols, from its seed (quirk Q1:
    derailed walks — tests/test_locate_rows_cpu.py pins that its table has replay rows AND serves derailed answers)"""
    rng = np.random.default_rng(9)
    parts = []
    for i in range(12):
        parts.append("".join(chr(0x4E00 + int(x) * 7) for x in rng.integers(0, 900, 1500)))
        parts.append(chr(0x30A1 + i) * 70_000)
        parts.append("log line %d\n" % i * 50)
    return "".join(parts)


def locate_host(fm, ch, off, mm, cap):
    n = len(off) - 1
    locs = np.full((n, cap), SENT, np.int32)
    locs, found, st, lf = fm.locate_batch(ch, off, mm, cap, want_steps=True, locs=locs)
    return locs, found, st, lf


def locate_dev(fm, ch, off, mm, cap):
    torch = _torch()
    n = len(off) - 1
    d_ch = torch.from_numpy(ch.view(np.int16)).cuda()
    d_off = torch.from_numpy(off).cuda()
    sent = lambda k: torch.full((max(k, 1),), SENT, dtype=torch.int32, device="cuda")
    locs, found, lf, st, rng = sent(n * cap), sent(n), sent(n), sent(n), sent(2 * n)
    rc = ia.lib.fmx_locate_batch_dev(fm.handle, d_ch.data_ptr(), d_off.data_ptr(), n, mm, locs.data_ptr(), cap, found.data_ptr(),
                                     lf.data_ptr(), st.data_ptr(), rng.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (ia.lib.fmx_last_error() or b"").decode()
    torch.cuda.synchronize()
    return locs.cpu().numpy()[: n * cap].reshape(n, cap), found.cpu().numpy()[:n], st.cpu().numpy()[:n], lf.cpu().numpy()[:n]


def same(a, b, what):
    for x, y, name in zip(a, b, ("locs", "found", "status", "lf_steps")):
        bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
        assert len(bad) == 0, "%s: %s differs at %d patterns, first %r" % (what, name, len(bad), bad[:5])


def against_oracle(res, o, ch, off, mm, cap, what):
    orc.counters_reset()
    exp = o.locate_batch(ch, off, mm, cap, threads=THREADS, fill=SENT)
    steps = orc.counters()["lf_steps"]
    same(res[:3], exp, what + " vs oracle")
    if not (exp[2] == 9)[:-1].any():  # (the last pattern is the empty one: no walk)
        assert int(res[3].astype(np.int64).sum()) == steps, what + ": LF-step total vs oracle"


LEGS = ((1, 1), (16, 16), (100, 100), (100, 60), (-1, 12))  # (max_matches, loc_cap): the last two overrun `locations` for some


def all_legs(fm, o, ch, off, what, pipelines=True):
    """every single-index entry point that locates; returns the results (for the comparison between the two residencies)"""
    out = {}
    for mm, cap in LEGS:
        out["host", mm, cap] = locate_host(fm, ch, off, mm, cap)
        against_oracle(out["host", mm, cap], o, ch, off, mm, cap, "%s locate_batch(%d, %d)" % (what, mm, cap))
        out["dev", mm, cap] = locate_dev(fm, ch, off, mm, cap)
        same(out["dev", mm, cap], out["host", mm, cap], "%s locate_batch_dev(%d, %d) vs the host call" % (what, mm, cap))
    if pipelines:
        k = min(len(off) - 1, 4000)
        pch, poff = ch[: off[k]], off[: k + 1]
        ex = fm.locate_extract_batch(pch, poff, 4, 24, fill=0xFFFE)
        ln = fm.locate_lines_batch(pch, poff, 4, "\n", 160, fill=0xFFFE)
        exp = o.locate_batch(pch, poff, 4, 4, threads=THREADS, fill=-1)
        for r, name in ((ex, "locate_extract_batch"), (ln, "locate_lines_batch")):
            assert (r["locs"] == exp[0]).all() and (r["found"] == exp[1]).all(), "%s %s vs oracle" % (what, name)
        out["extract"] = tuple(ex[f] for f in ("locs", "found", "dst", "out_len", "steps", "status", "hit_status"))
        out["lines"] = tuple(ln[f] for f in ("locs", "found", "dst", "out_len", "steps", "status", "hit_status", "hit_aux"))
    return out


def equal_runs(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert (x == y).all(), "%s: %r output %d differs between the walk and the table" % (what, key, i)


def twice(fm, what, body, expect_table=True):
    """body(fm, tag) under locate_rows 0 and 1 (the index made resident anew each time); returns both results"""
    res = []
    for rows in (0, 1):
        with options(locate_rows=rows):
            fm.to_device(0)
        nbytes, replay = fm.locate_rows_info()
        n = fm.getInputLength()
        if rows and expect_table:
            assert nbytes == (4 * n + 63) // 64 * 64 and 0 <= replay < n, (what, nbytes, replay)
        else:
            assert (nbytes, replay) == (0, 0), what
        res.append(body(fm))
    return res


@pytest.mark.parametrize("sr", [32, 64])
def test_log_index_every_entry_point(sr):
    """the log config at 16 MiB"""
    text = workload.log_text(24)
    fm = ia.FmIndex(text, sr, True, device=None, build_device=0)
    try:
        o = orc.OracleFmIndex.read(fm.write(False))
        ch, off = patterns(text, np.random.default_rng(sr), 20_000, 6, 12)
        walk, table = twice(fm, "log sr %d" % sr, lambda f: all_legs(f, o, ch, off, "log sr %d" % sr))
        equal_runs(walk, table, "log sr %d" % sr)
        assert fm.locate_rows_info()[1] == 0  # a clean text: every row served from the table
        # ... and with the walk-order stage in front (the suite holds walk_order_min at 1: k_locate_rows takes `order` records)
        with options(locate_rows=1, rows_order=1):
            ordered = all_legs(fm, o, ch, off, "log sr %d, rows_order 1" % sr, pipelines=False)
        for key in ordered:
            same(ordered[key], table[key], "rows_order 1 %r" % (key,))
    finally:
        fm.close()


@pytest.mark.parametrize("form", [0, 1, 3])
def test_run_block_text_quirk_rows(form):
    """derailed walks (Q1) and replay rows, the fill over no directory, the cells and the flat form"""
    text = run_block_text()
    t16 = ia.as_chars(text)
    with options(window_cells=form):
        fm = ia.FmIndex(text, 16, True, device=None)
        try:
            o = orc.OracleFmIndex(text, 16, True)
            rng = np.random.default_rng(5)
            ch, off = patterns(t16, rng, 6000, 1, 6, absent_every=101)
            walk, table = twice(fm, "run blocks", lambda f: all_legs(f, o, ch, off, "run blocks, window_cells %d" % form, pipelines=form == 3))
            equal_runs(walk, table, "run blocks")
            nbytes, replay = fm.locate_rows_info()
            assert 0 < replay < fm.getInputLength()
            REPLAY_ROWS.setdefault("n", replay)
            assert REPLAY_ROWS["n"] == replay  # the same table whatever the fill walked over
            # every single-symbol pattern, no limit: all rows but the sentinel's, replayed ones included
            syms = np.unique(t16)
            sch, soff = ia.pack_patterns([np.array([s], np.uint16) for s in syms])
            cap = int(np.bincount(t16).max())
            res = locate_host(fm, sch, soff.astype(np.int32), -1, cap)
            against_oracle(res, o, sch, soff.astype(np.int32), -1, cap, "every row of the run-block text")
        finally:
            fm.close()


REPLAY_ROWS = {}


def test_compact_image():
    text = workload.log_text(22)
    with options(image_compact=1):
        fm = ia.FmIndex(text, 32, True, device=None, build_device=0)
        fm.blob()  # flattened under the option
    try:
        o = orc.OracleFmIndex.read(fm.write(False))
        ch, off = patterns(text, np.random.default_rng(8), 8000, 5, 12)
        walk, table = twice(fm, "compact", lambda f: all_legs(f, o, ch, off, "compact"))
        equal_runs(walk, table, "compact")
    finally:
        fm.close()


def test_segment_set_and_replicas():
    """fmx_count_locate_segments (int64 positions, `taken` carried across segments) and two replicas on the one GPU, each with a
    table of its own"""
    text = workload.log_text(23)
    rng = np.random.default_rng(12)
    ch, off = patterns(text, rng, 12_000, 4, 9)
    n = len(off) - 1
    mm = 16
    results = []
    for rows in (0, 1):
        with options(locate_rows=rows):
            seg = ia.SegmentedFmIndex(text, 32, True, device=0, segment_chars=1 << 21)
            try:
                assert len(seg) >= 4
                for s in seg.segments:
                    assert (s.locate_rows_info()[0] > 0) == bool(rows)
                counts, lf = np.full(n, SENT, np.int64), np.full(n, SENT, np.int64)
                locs = np.full((n, mm), SENT, np.int64)
                found, st = np.full(n, SENT, np.int32), np.full(n, SENT, np.int32)
                rc = ia.lib.fmx_count_locate_segments(seg.handles, len(seg), seg.base_array.ctypes.data, ch.ctypes.data, off.ctypes.data, n,
                                                      mm, counts.ctypes.data, lf.ctypes.data, locs.ctypes.data, found.ctypes.data,
                                                      st.ctypes.data)
                assert rc == 0, (ia.lib.fmx_last_error() or b"").decode()
                if not rows:  # the oracle: every segment's own locate, appended in segment order until maxMatches
                    exp_locs = np.full((n, mm), SENT, np.int64)
                    exp_found, exp_counts, exp_st = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
                    for s, base in zip(seg.segments, seg.bases):
                        o = orc.OracleFmIndex.read(s.write(False))
                        ol, of, ost = o.locate_batch(ch, off, mm, mm, threads=THREADS)
                        oc, _ = o.count_batch(ch, off, threads=THREADS)
                        exp_counts += oc
                        exp_st |= ost
                        for i in np.flatnonzero(of):
                            take = min(int(of[i]), mm - int(exp_found[i]))
                            exp_locs[i, exp_found[i]:exp_found[i] + take] = base + ol[i, :take]
                            exp_found[i] += take
                    results.append(("oracle", (exp_locs, exp_found, exp_st, exp_counts)))
                    assert (exp_found == mm).any() and ((exp_found > 0) & (exp_found < mm)).any()
                results.append(("rows %d" % rows, (locs, found, st, counts)))
                if rows:
                    rs = ia.ReplicaSet(seg.segments[0], [0, 0])
                    try:
                        for h in rs.handles:
                            nbytes, replay = C.c_int64(0), C.c_int64(0)
                            assert ia.lib.fmx_locate_rows_info(h, C.byref(nbytes), C.byref(replay)) == 0
                            assert nbytes.value == seg.segments[0].locate_rows_info()[0] > 0
                        o0 = orc.OracleFmIndex.read(seg.segments[0].write(False))
                        for lmm, cap in ((16, 16), (-1, 12)):
                            rl = np.full((n, cap), SENT, np.int32)
                            r = rs.locate_batch(ch, off, lmm, cap, want_steps=True, locs=rl)
                            against_oracle(r, o0, ch, off, lmm, cap, "two replicas (%d, %d)" % (lmm, cap))
                            same(r, locate_host(seg.segments[0], ch, off, lmm, cap), "two replicas vs one index")
                    finally:
                        rs.close()
            finally:
                for s in seg.segments:
                    s.close()
    oracle = results[0][1]
    for name, got in results[1:]:
        for x, y, field in zip(got, oracle, ("locs", "found", "status", "counts")):
            assert (x == y).all(), "segment set, %s: %s differs from the oracle" % (name, field)


def test_launch_shapes_loop_three_times():
    """(512, 1), (1024, 1), (512, 16), (1024, 16): with one workgroup per CU the batch is sized from the CU count so that
    k_locate_rows runs its grid-stride loop at least three times (asserted), with 16-lane groups (cap 16) and whole waves (cap 100)"""
    text = ia.synth_log(1 << 21)
    L = n_cu() * 1024
    n_pat = -(-3 * L // 16) + 1000
    ch, off = patterns(text, np.random.default_rng(21), n_pat, 5, 12, absent_every=101)
    n = len(off) - 1
    o = orc.OracleFmIndex(text, 16, True)
    exp = {(mm, cap): o.locate_batch(ch, off, mm, cap, threads=THREADS, fill=SENT) for mm, cap in ((16, 16), (100, 100), (-1, 40))}
    assert (exp[100, 100][1] > 16).any() and (exp[-1, 40][2] == 9).any()  # more hits than a 16-lane group, `locations` overrun
    with options(locate_rows=1):
        fm = ia.FmIndex(text, 16, True, device=0)
    try:
        assert fm.locate_rows_info()[0] > 0
        first = {}
        for block, gpc in SHAPES:
            with options(block=block, groups_per_cu=gpc):
                for (mm, cap), e in exp.items():
                    lanes = 16 if cap == 16 else 64
                    if gpc == 1:
                        grid = max(1, min(-(-n * lanes // block), n_cu() * gpc))
                        assert -(-n * lanes // (grid * block)) >= 3, "the batch is too small to loop three times at %r" % ((block, gpc),)
                    for call, ordered in ((locate_dev, 0), (locate_host, 0), (locate_dev, 1)):
                        with options(rows_order=ordered):
                            r = call(fm, ch, off, mm, cap)
                        same(r[:3], e, "shape %r (%d, %d) vs oracle" % ((block, gpc), mm, cap))
                        f = first.setdefault((mm, cap), r[3])
                        assert (f == r[3]).all(), "LF-steps differ between shapes"
    finally:
        fm.close()


def test_info_bytes_budget_and_resident_bytes():
    text = ia.synth_log(1 << 22)
    fm = ia.FmIndex(text, 32, True, device=None)
    try:
        o = orc.OracleFmIndex(text, 32, True)
        ch, off = patterns(text, np.random.default_rng(2), 3000, 5, 10)
        n = fm.getInputLength()

        def resident():
            out = [C.c_int64(-1) for _ in range(3)]
            assert ia.lib.fmx_resident_bytes(fm.handle, *[C.byref(x) for x in out]) == 0
            return tuple(x.value for x in out)

        assert fm.locate_rows_info() == (0, 0)  # not resident
        with options(locate_rows=0):
            fm.to_device(0)
        assert fm.locate_rows_info() == (0, 0)
        off_bytes = resident()
        with options(locate_rows=1):
            fm.to_device(0)
        assert fm.locate_rows_info() == ((4 * n + 63) // 64 * 64, 0)
        assert resident() == off_bytes  # fmx_resident_bytes reports image, suffix table and directory: unchanged by the option
        # a budget below the table's size (16 MiB + 64): resident without a table, and still right
        with options(locate_rows=1, window_cells_mb=(4 * n >> 20) - 1):
            fm.to_device(0)
        assert fm.locate_rows_info() == (0, 0)
        r = locate_host(fm, ch, off, 16, 16)
        against_oracle(r, o, ch, off, 16, 16, "without a table (budget)")
        with options(locate_rows=1, window_cells_mb=(4 * n >> 20) + 1):
            fm.to_device(0)
        assert fm.locate_rows_info()[0] > 0
        same(locate_host(fm, ch, off, 16, 16), r, "with a table again")
        # kinds that never get one
        with options(locate_rows=1):
            rrr = ia.RrrVector([1, 0, 0, 1] * 1000, device=0)
            wt = ia.WaveletFixedBlockBoosting("abracadabra" * 50, device=0)
            for h in (rrr._h, wt._h):
                nbytes = C.c_int64(-1)
                assert ia.lib.fmx_locate_rows_info(h, C.byref(nbytes), None) == 0 and nbytes.value == 0
    finally:
        fm.close()


@pytest.mark.plan_policy
def test_config2_full_size_with_the_table():
    """configs[2] at its stated size — 100,000 patterns, <= 16 hits, the 256 MiB log, sampleRate 32 — through the table, under the
    library's own plan policy: every position against the oracle, as tests/test_gpu_configs_fullsize.py does for the walk"""
    M, K = 8, 100_000
    text = workload.log_text(28)
    pat, off, _ = workload.count_batch_patterns(text, K, M)
    fm = ia.FmIndex(text, 32, True, device=None, build_device=0)
    try:
        with options(locate_rows=1):
            fm.to_device(0)
        nbytes, replay = fm.locate_rows_info()
        assert nbytes == (4 * ((1 << 28) + 1) + 63) // 64 * 64 and replay == 0
        oracle = orc.OracleFmIndex.read(fm.write(False))
        locs, found, st, lf = fm.locate_batch(pat, off, 16, want_steps=True)
        orc.counters_reset()
        olocs, ofound, ost = oracle.locate_batch(pat, off, 16, threads=os.cpu_count() or 1)
        c = orc.counters()
        assert (st == ost).all() and (st == 0).all() and (found == ofound).all()
        live = np.arange(16)[None, :] < found[:, None]
        assert (locs[live] == olocs[live]).all()
        assert (locs[~live] == 0).all()  # slots beyond `found` keep the caller's values
        assert int(lf.astype(np.int64).sum()) == c["lf_steps"]
        P = pat.reshape(K, M)
        for k in range(16):
            sel = found > k
            assert (text[locs[sel, k][:, None] + np.arange(M)[None, :]] == P[sel]).all()
    finally:
        fm.close()

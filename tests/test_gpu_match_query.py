"""The lines that match a QUERY of several terms on the GPU: packed hits of a batch of terms -> the packed distinct lines of each
query (fmx_query_lines_of_hits_dev: the kernels of fmx_query_lines.hip and rocPRIM's sort, reduction by key and scans) and the host
form fmx_match_query_batch, with their Python and C++ mirrors.

The judge is the oracle plus numpy (tests/test_match_query_cpu.py: Universe, TermBatch.judge — the lines of a term are
judge_lines' of tests/test_match_lines_cpu.py, the lines of a query the set formula over them by np.intersect1d / union1d /
setdiff1d), computed once per batch.  Outputs are prefilled with a sentinel.  The batches hold the corner cases — asserted on the
judge's answer before the GPU runs.  Options are set inside the tests and put back in `finally`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import _torch, options
from test_locate_all_cpu import ABSENT, SENT, assert_corner_cases, corner_batch, expected_packed
from test_match_lines_cpu import MAX_LINES, check_lines, judge_n_lines, judge_table, with_boundary_patterns
from test_match_query_cpu import ALL, ANY, NONE, TermBatch, Universe, cut_into_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
NL = ord("\n")
PAD = 64  # ints behind line_off[q] that must keep the sentinel

# the named queries, as (all, any, none), and their lines on the fixture
NAMED = [
    ((["WARN"], [], []), 80),
    ((["INFO"], [], []), 1920),
    ((["WARN", "INFO"], [], []), 0),
    ((["WARN", "blk_"], [], []), 80),
    ((["INFO", "PacketResponder", "terminating"], [], []), 310),
    ((["INFO"], [], ["PacketResponder"]), 1318),
    (([" "], [], ["INFO"]), 80),
    ((["blk_"], ["WARN", "NameSystem"], ["exception"]), 653),
]


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def as_query(U, spec):
    return [(pid, kind) for kind, group in zip((ALL, ANY, NONE), spec) for pid in U.ids(*group)]


def host_query(fm, b, max_lines):
    lines, line_off, st, line_count, occ = fm.match_query_batch(b.ch, b.off, b.query_off, b.kinds, max_lines, want_counts=True)
    return (np.concatenate([lines, np.full(PAD, SENT, np.int32)]), line_off, line_count), st, occ


def filled(fm, b):
    d = DevAll(fm, b.ch, b.off, -1)
    d.fill(0, d.total)
    assert d.total == b.total
    return d


def dev_query(d, b, max_lines, extra_hits=0, ws_bytes=None, query_off=None, kinds=None):
    """fmx_query_lines_of_hits_dev over what a DevAll (stage 1 + a full stage 2) left; extra_hits: n_hits beyond hit_off[n]"""
    torch = d.torch
    n_hits = d.total + extra_hits
    assert extra_hits <= PAD  # (d.locs has that many slots behind the hits)
    need = ia.lib.fmx_query_lines_scratch_bytes(b.n, b.q, n_hits)
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device="cuda")
    line_off = torch.full((b.q + 1,), SENT, dtype=torch.int64, device="cuda")
    lines = torch.full((n_hits + PAD,), SENT, dtype=torch.int32, device="cuda")
    line_count = torch.full((max(b.q, 1),), SENT, dtype=torch.int32, device="cuda")
    qo = np.array(b.query_off if query_off is None else query_off, np.int32)   # the call's own copies: scribbled over once it is back
    kd = np.array(b.kinds if kinds is None else kinds, np.uint8)
    rc = ia.lib.fmx_query_lines_of_hits_dev(d.fm.handle, b.n, b.q, qo.ctypes.data, kd.ctypes.data, d.hit_off.data_ptr(), d.locs.data_ptr(), n_hits,
                                            max_lines, line_off.data_ptr(), lines.data_ptr(), line_count.data_ptr(), ws.data_ptr(),
                                            need if ws_bytes is None else ws_bytes, d.stream)
    qo[:] = -7  # (the call has copied what it needs before it returns)
    kd[:] = 9
    torch.cuda.synchronize()
    return rc, (lines.cpu().numpy(), line_off.cpu().numpy(), line_count.cpu().numpy()[: b.q])


@pytest.fixture(scope="module")
def hd():
    """the fixture at sampleRate 16 with its line table, its oracle, the judge's T, and the corner-case batch of
    tests/test_gpu_match_lines.py (about 10^6 hits) cut into queries, with the named queries, a NONE-only one and empty ones"""
    t16 = ia.as_chars(HD)
    o = orc.OracleFmIndex(HD, 16, True)
    T = judge_table(o, NL)
    ch, off = corner_batch(t16, np.random.default_rng(16), 2900, min_len=2)
    ch, off = with_boundary_patterns(t16, ch, off, T, NL, more=("blk_",))
    exp = expected_packed("hd16 match lines", o, ch, off, -1)  # (the batch of test_gpu_match_lines' fixture: computed once)
    assert_corner_cases(exp[4], exp[2])
    chn, offn = ia.pack_patterns(["WARN", "PacketResponder", "terminating", "NameSystem", "exception"])
    offn = offn.astype(np.int32)
    U = Universe((ch, off, exp), (chn, offn, expected_packed("hd16 query names", o, chn, offn, -1)))
    n_base = len(off) - 1
    named = [as_query(U, spec) for spec, _ in NAMED]
    queries = [[]] + cut_into_queries(list(range(n_base)), np.random.default_rng(23)) + named
    queries += [[(U.ids("INFO")[0], NONE), (U.ids(" ")[0], NONE)], []]
    b = TermBatch(U, queries)
    # the corner cases, on the judge's answer
    per = b.per_query(T)
    assert [len(u) for u in per[-2 - len(NAMED):-2]] == [k for _, k in NAMED]
    assert len(per[0]) == 0 and len(per[-1]) == 0 and len(per[-2]) == 0 and b.query_off[1] == 0 and b.query_off[-2] == b.n
    sp = U.ids(" ")[0]
    assert U.counts[sp] == 30094 and len(np.unique(np.searchsorted(T, U.hits[sp]))) == 2000
    sizes = np.diff(b.query_off)
    assert sizes.max() == 6 and (sizes == 0).sum() > 10 and b.total > 900_000 and (b.status == 9).sum() == 1
    n_out = np.array([len(u) for u in per])
    assert (n_out > 16).sum() > 20 and (n_out == 1).any() and ((n_out == 0) & (sizes > 0)).sum() > 20
    fm = ia.FmIndex(HD, 16, True, device=0)
    assert fm.build_line_table("\n") == 2000
    yield t16, o, T, U, b, fm
    fm.close()


@pytest.fixture(scope="module")
def hd_filled(hd):
    return filled(hd[5], hd[4])


@pytest.mark.parametrize("max_lines", MAX_LINES)
def test_corner_batch_host_and_device_forms(hd, hd_filled, max_lines):
    t16, o, T, U, b, fm = hd
    want = b.judge(T, max_lines)
    got, st, occ = host_query(fm, b, max_lines)
    check_lines(got, want, "host form, max_lines %d" % max_lines, tail=SENT)
    assert (st == b.status).all() and (occ == b.counts).all()
    rc, dev = dev_query(hd_filled, b, max_lines)
    assert rc == 0, last_error()
    check_lines(dev, want, "device form, max_lines %d" % max_lines, tail=SENT)  # (the sentinel intact behind d_line_off[q])
    total = int(want[1][-1])
    assert (dev[0][:total] == got[0][:total]).all() and (dev[1] == got[1]).all() and (dev[2] == got[2]).all()
    if max_lines in (0, 16):  # d_locs with slots behind hit_off[n]
        rc, dev = dev_query(hd_filled, b, max_lines, extra_hits=37)
        assert rc == 0, last_error()
        check_lines(dev, want, "device form, n_hits beyond hit_off[n], max_lines %d" % max_lines, tail=SENT)


def test_one_term_per_query_is_match_lines_batch(hd):
    t16, o, T, U, b0, fm = hd
    empty = [i for i, p in enumerate(U.pats) if len(p) == 0]
    ids = sorted(set(range(0, len(U.pats), 3)) | set(empty))
    b = TermBatch(U, [[(pid, ALL)] for pid in ids])
    assert b.total > 200_000 and (b.status == 9).sum() == 1
    for max_lines in (0, 16):
        ref = fm.match_lines_batch(b.ch, b.off, max_lines, want_counts=True)
        got = fm.match_query_batch(b.ch, b.off, b.query_off, b.kinds, max_lines, want_counts=True)
        for a, r, what in zip(got, ref, ("lines", "line_off", "status", "line_count", "occurrences")):
            assert a.dtype == r.dtype and a.shape == r.shape and (a == r).all(), what
        check_lines((np.concatenate([got[0], [SENT]]).astype(np.int32), got[1], got[3]), b.judge(T, max_lines), "one term per query", tail=SENT)


def test_skew_one_heavy_query_and_many_light_terms(hd):
    t16, o, T, U, b0, fm = hd
    # ONE query whose ALL term matches in every line: about 30,000 hits, an answer of 80 lines
    b = TermBatch(U, [as_query(U, ([" "], [], ["INFO"]))])
    assert b.q == 1 and b.total == 30094 + U.counts[U.ids("INFO")[0]]
    for max_lines in (0, 7):
        want = b.judge(T, max_lines)
        assert list(want[2]) == [80]
        got, st, occ = host_query(fm, b, max_lines)
        check_lines(got, want, "one heavy query, host form", tail=SENT)
        assert occ[0] == 30094
        rc, dev = dev_query(filled(fm, b), b, max_lines)
        assert rc == 0, last_error()
        check_lines(dev, want, "one heavy query, device form", tail=SENT)
    # 3,000 terms of at most one hit each (the batch of test_gpu_match_lines' skew test), in pairs as ANY
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
    bl = TermBatch(Universe((chl, offl, expl)), [[(2 * i, ANY), (2 * i + 1, ANY)] for i in range(1500)])
    want = bl.judge(T, 0)
    assert {1, 2} <= set(want[2]) <= {0, 1, 2}  # (a pair on one line, a pair on two)
    got, st, occ = host_query(fm, bl, 0)
    check_lines(got, want, "1,500 light queries, host form", tail=SENT)
    assert (occ == expl[4]).all()
    rc, dev = dev_query(filled(fm, bl), bl, 0)
    assert rc == 0, last_error()
    check_lines(dev, want, "1,500 light queries, device form", tail=SENT)


_BETWEEN = {}


@pytest.mark.parametrize("cells,rows,compact", [(0, 0, 0), (1, 1, 0), (2, 0, 1)])
def test_residencies(hd, cells, rows, compact):
    t16, o, T, U, b = hd[:5]
    what = "window_cells %d locate_rows %d compact %d" % (cells, rows, compact)
    with options(window_cells=cells, locate_rows=rows, image_compact=compact):
        fm = ia.FmIndex(HD, 16, True, device=None)
        fm.blob()  # flattened under the option
        fm.to_device(0)
    try:
        assert (fm.locate_rows_info()[0] > 0) == bool(rows)
        assert fm.build_line_table("\n") == 2000
        want = b.judge(T, 0)
        got, st, occ = host_query(fm, b, 0)
        check_lines(got, want, what, tail=SENT)
        assert (st == b.status).all() and (occ == b.counts).all()
        first = _BETWEEN.setdefault("first", got)
        assert all((a == r).all() for a, r in zip(got, first)), what + ": vs the first residency"
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
        U = Universe((ch, off, exp))
        kinds = [(ALL, ALL, NONE), (ALL, ANY, ANY), (ANY, NONE, ALL), (ALL, ALL, ALL), (ANY, ANY, NONE), (NONE, ALL, ANY)]
        n = len(U.pats)
        queries = [[(pid, kinds[(i // 3) % len(kinds)][pid - i]) for pid in range(i, min(i + 3, n))] for i in range(0, n, 3)]
        b = TermBatch(U, queries)
        assert b.total == len(t16)  # 2 M packed hits
        T = judge_table(o, NL)
        assert fm.build_line_table("\n") == judge_n_lines(T, len(t16))
        key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
        assert ia.lib.fmx_hit_lines_geometry(fm.handle, b.total, C.byref(key_grid), C.byref(flat_grid)) == 0
        assert 3 * key_grid.value * 1024 <= b.total and 3 * flat_grid.value * 256 <= b.total  # every loop over hits runs at least three times
        per_term, per = b.term_lines(T), b.per_query(T)
        loses = proper = False
        for Q, qu in enumerate(queries):
            terms = list(range(b.query_off[Q], b.query_off[Q + 1]))
            alls = [per_term[t] for t in terms if b.kinds[t] == ALL]
            nones = [per_term[t] for t in terms if b.kinds[t] == NONE]
            if len(alls) == 2 and len(terms) == 3 and nones:
                both = np.intersect1d(alls[0], alls[1])
                proper |= 0 < len(both) < min(len(alls[0]), len(alls[1]))
                loses |= 0 < len(per[Q]) < len(both)
        assert loses and proper  # a query loses lines to a NONE term; an ALL pair intersects to a proper, non-empty subset
        want = b.judge(T, 0)
        assert int(want[1][-1]) > 3 * len(T)
        got, st, occ = host_query(fm, b, 0)
        check_lines(got, want, "2 M hits, host form", tail=SENT)
        rc, dev = dev_query(filled(fm, b), b, 0)
        assert rc == 0, last_error()
        check_lines(dev, want, "2 M hits, device form", tail=SENT)
    finally:
        fm.close()


def test_errors_and_edges(hd):
    t16, o, T, U = hd[:4]
    E_ARG = ia._lib.E_ARG
    torch = _torch()
    fm = ia.FmIndex(HD, 16, True, device=0)
    try:
        assert fm.line_table_info() == (-1, 0, 0)
        b = TermBatch(U, [as_query(U, (["INFO"], [], ["PacketResponder"])), as_query(U, (["blk_"], ["WARN"], []))])
        host = ia.lib.fmx_match_query_batch

        def call(bb=b, query_off=None, kinds=None, lo=None, out=None):
            qo = bb.query_off if query_off is None else np.array(query_off, np.int32)
            kd = bb.kinds if kinds is None else np.array(kinds, np.uint8)
            return host(fm.handle, bb.ch.ctypes.data, bb.off.ctypes.data, bb.n, qo.ctypes.data, kd.ctypes.data, len(qo) - 1, 0, lo.ctypes.data,
                        C.byref(out), None, None, None)

        # no table: FMX_E_ARG, and the message names the call that makes one
        line_off = np.full(3, SENT, np.int64)
        buf = C.c_void_p(0x1234)
        assert call(lo=line_off, out=buf) == E_ARG and "fmx_line_table_build" in last_error() and buf.value is None and (line_off == SENT).all()
        d = filled(fm, b)
        rc, _ = dev_query(d, b, 0)
        assert rc == E_ARG and "fmx_line_table_build" in last_error()
        assert fm.build_line_table("\n") == 2000
        # a workspace that is too small: an error, nothing is launched, nothing is written
        rc, dev = dev_query(d, b, 0, ws_bytes=ia.lib.fmx_query_lines_scratch_bytes(b.n, b.q, d.total) - 256)
        assert rc == E_ARG and (dev[1] == SENT).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all()
        # a bad query_off, a kind above 2: likewise
        for bad in (dict(query_off=[1, 2, 4]), dict(query_off=[0, 3, 2]), dict(query_off=[0, 5, 4]), dict(query_off=[0, 2, 3]),
                    dict(kinds=[0, 2, 0, 3])):
            rc, dev = dev_query(d, b, 0, **bad)
            assert rc == E_ARG and (dev[1] == SENT).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all(), bad
            buf.value = 0x1234
            assert call(lo=line_off, out=buf, **bad) == E_ARG and buf.value is None and (line_off == SENT).all(), bad
        rc, dev = dev_query(d, b, 0)
        assert rc == 0, last_error()
        want = b.judge(T, 0)
        assert list(want[2]) == [1318, 80]
        check_lines(dev, want, "two queries", tail=SENT)
        # q == 0 (then n == 0): the one offset is zeroed, nothing else is written
        none = TermBatch(U, [])
        h = np.full(1, SENT, np.int64)
        assert call(bb=none, lo=h, out=buf) == 0 and h[0] == 0 and buf.value is None
        d_off = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
        zero = np.zeros(1, np.int32)
        assert ia.lib.fmx_query_lines_of_hits_dev(fm.handle, 0, 0, zero.ctypes.data, None, None, None, 0, 0, d_off.data_ptr(), None, None, None, 0,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert int(d_off.cpu()[0]) == 0
        # queries without terms
        lines, line_off3, st, line_count, occ = fm.match_query_batch(np.zeros(0, np.uint16), [0], [0, 0, 0], [], 0, want_counts=True)
        assert len(lines) == 0 and list(line_off3) == [0, 0, 0] and list(line_count) == [0, 0]
        # a batch without hits (device form: n_hits == 0 — the offsets are zeroed, nothing else is written)
        ch0, off0 = ia.pack_patterns(["zzzzqq#", "", "qqqqzz#"])
        off0 = off0.astype(np.int32)
        b0 = TermBatch(Universe((ch0, off0, expected_packed("hd16 query no hits", o, ch0, off0, -1))), [[(0, ALL), (1, ANY)], [(2, ANY)], []])
        got, st, occ = host_query(fm, b0, 0)
        assert (got[0] == SENT).all() and (got[1] == 0).all() and list(st) == [0, 9, 0] and (got[2] == 0).all() and (occ == 0).all()
        d0 = filled(fm, b0)
        assert d0.total == 0
        rc, dev = dev_query(d0, b0, 0)
        assert rc == 0 and (dev[1] == 0).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all()
        # the wrong handle kinds
        sa = ia.SuffixArray("banana", device=None, build_device=-1)
        sa.construct()
        rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
        wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
        for other in (sa._h, rrr._h, wt._h):
            buf.value = 0x1234
            assert host(other, b.ch.ctypes.data, b.off.ctypes.data, b.n, b.query_off.ctypes.data, b.kinds.ctypes.data, b.q, 0, line_off.ctypes.data,
                        C.byref(buf), None, None, None) == E_ARG and buf.value is None
        # resident again: the table is gone with the rest of the resident state
        fm.to_device(0)
        assert fm.line_table_info() == (-1, 0, 0)
        assert call(lo=line_off, out=buf) == E_ARG and "fmx_line_table_build" in last_error()
    finally:
        fm.close()


def test_round_trip_and_mirrors(hd, tmp_path):
    t16, o, T, U, b0, fm = hd
    text_lines = HD.split("\n")[:2000]
    words = ["INFO", "PacketResponder", "terminating"]
    mine = [k for k, ln in enumerate(text_lines) if all(w in ln for w in words)]
    assert len(mine) == 310
    got = fm.match_query(all=words)
    assert got.dtype == np.int32 and list(got) == mine
    assert list(fm.match_query(all=words, max_lines=5)) == mine[:5]
    start, stop = fm.line_bounds(got)
    width = int((stop - start).max())
    dst, out_len, st = fm.extract_batch(start, stop, width)
    assert (st == 0).all() and (out_len == stop - start).all()
    extracted = [ia.chars_to_str(dst[i, : out_len[i]]) for i in range(len(got))]
    assert extracted == [text_lines[k] for k in mine] and all(w in ln for ln in extracted for w in words)
    plain = [k for k, ln in enumerate(text_lines) if "blk_" in ln and ("WARN" in ln or "NameSystem" in ln) and "exception" not in ln]
    assert len(plain) == 653 and list(fm.match_query(all="blk_", any=["WARN", "NameSystem"], none=["exception"])) == plain
    assert list(fm.match_query(all=" ", none="INFO")) == [k for k, ln in enumerate(text_lines) if "INFO" not in ln]
    assert len(fm.match_query(none="INFO")) == 0 and len(fm.match_query()) == 0
    with pytest.raises(IndexError):
        fm.match_query(all=["INFO", ""])
    # the C++ mirror: tests/cpp/test_match_query_mirror.cpp prints what matchQueryBatch / matchQuery return
    exe = str(tmp_path / "test_match_query_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_match_query_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    specs = [(words, [], []), (["blk_"], ["WARN", "NameSystem"], ["exception"]), ([], [], ["INFO"]), ([], [], []), ([" "], [], ["INFO"])]
    bm = TermBatch(U, [as_query(U, s) for s in specs])
    lines, line_off, line_count = bm.judge(T, 0)
    assert out["n_lines"] == [2000]
    assert out["batch_offsets"] == list(line_off) and out["batch_lines"] == list(lines)
    assert out["batch_line_count"] == list(line_count) == [310, 653, 0, 0, 80] and out["batch_occurrences"] == list(bm.counts)
    cut = bm.judge(T, 7)
    assert out["cut_offsets"] == [0, 7, 14, 14, 14, 21] == list(cut[1]) and out["cut_lines"] == list(cut[0])
    assert out["cut_line_count"] == [310, 653, 0, 0, 80]
    assert out["one"] == mine and out["one_cut"] == mine[:3]

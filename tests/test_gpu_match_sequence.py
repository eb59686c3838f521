"""The lines that hold a SEQUENCE of terms in order on the GPU (grep 'A.*B'): packed hits of a batch of terms -> the packed lines of
each sequence (fmx_sequence_lines_of_hits_dev: the kernels of fmx_sequence_lines.hip and rocPRIM's sort and scans) and the host forms
fmx_match_sequence_batch / fmx_match_sequence_class_batch, with their Python and C++ mirrors.

The judge is the oracle plus numpy (tests/test_match_sequence_cpu.py: SeqBatch.judge — the oracle's hits per term, judge_table's T,
a BACKWARD pass per sequence over the lines, the opposite direction to the kernel's rule; spans by judge_spans, and by Python's re
for the named sequences), computed once per batch.  Outputs are prefilled with a sentinel.  The batches hold the corner cases —
asserted on the judge's answer before the GPU runs.  Options are set inside the tests and put back in `finally`."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import _torch, options, run_block_text
from test_locate_all_cpu import ABSENT, SENT, assert_corner_cases, corner_batch, expected_packed
from test_match_lines_cpu import MAX_LINES, judge_n_lines, judge_table, with_boundary_patterns
from test_match_query_cpu import Universe
from test_match_sequence_cpu import COLON5, NAMED, SP12, SeqBatch, check_sequence, cut_into_sequences, occurrences_in_text, re_judge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
NL = ord("\n")
PAD = 64  # ints behind line_off[q] that must keep the sentinel


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def host_sequence(fm, b, max_lines, want_spans=True):
    out = fm.match_sequence_batch(b.ch, b.off, b.query_off, max_lines, want_counts=True, want_spans=want_spans)
    lines, line_off, st, line_count, occ = out[:5]
    spans = np.concatenate([out[5].reshape(-1), np.full(PAD, SENT, np.int32)]) if want_spans else None
    return (np.concatenate([lines, np.full(PAD, SENT, np.int32)]), line_off, line_count), spans, st, occ


def filled(fm, b):
    d = DevAll(fm, b.ch, b.off, -1)
    d.fill(0, d.total)
    assert d.total == b.total
    return d


def dev_sequence(d, b, max_lines, extra_hits=0, ws_bytes=None, query_off=None, term_len=None, want_spans=True):
    """fmx_sequence_lines_of_hits_dev over what a DevAll (stage 1 + a full stage 2) left; extra_hits: n_hits beyond hit_off[n]"""
    torch = d.torch
    n_hits = d.total + extra_hits
    assert extra_hits <= PAD  # (d.locs has that many slots behind the hits)
    need = ia.lib.fmx_sequence_lines_scratch_bytes(b.n, b.q, n_hits)
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device="cuda")
    line_off = torch.full((b.q + 1,), SENT, dtype=torch.int64, device="cuda")
    lines = torch.full((n_hits + PAD,), SENT, dtype=torch.int32, device="cuda")
    spans = torch.full((2 * (n_hits + PAD),), SENT, dtype=torch.int32, device="cuda")
    line_count = torch.full((max(b.q, 1),), SENT, dtype=torch.int32, device="cuda")
    qo = np.array(b.query_off if query_off is None else query_off, np.int32)  # the call's own copies: scribbled over once it is back
    tl = np.array(b.term_len if term_len is None else term_len, np.int32)
    rc = ia.lib.fmx_sequence_lines_of_hits_dev(d.fm.handle, b.n, b.q, qo.ctypes.data, tl.ctypes.data, d.hit_off.data_ptr(), d.locs.data_ptr(),
                                               n_hits, max_lines, line_off.data_ptr(), lines.data_ptr(), line_count.data_ptr(),
                                               spans.data_ptr() if want_spans else None, ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                               d.stream)
    qo[:] = -7  # (the call has copied what it needs before it returns)
    tl[:] = -9
    torch.cuda.synchronize()
    return rc, (lines.cpu().numpy(), line_off.cpu().numpy(), line_count.cpu().numpy()[: b.q]), spans.cpu().numpy()


@pytest.fixture(scope="module")
def hd():
    """the fixture at sampleRate 16 with its line table, its oracle, the judge's T, and the corner-case batch of
    tests/test_gpu_match_lines.py (about 10^6 hits) cut into sequences, with the named sequences and empty ones"""
    t16 = ia.as_chars(HD)
    o = orc.OracleFmIndex(HD, 16, True)
    T = judge_table(o, NL)
    ch, off = corner_batch(t16, np.random.default_rng(16), 2900, min_len=2)
    ch, off = with_boundary_patterns(t16, ch, off, T, NL, more=("blk_",))
    exp = expected_packed("hd16 match lines", o, ch, off, -1)  # (the batch of test_gpu_match_lines' fixture: computed once)
    assert_corner_cases(exp[4], exp[2])
    names = sorted({t for terms, _, _ in NAMED for t in terms} - {"blk_", " "})
    chn, offn = ia.pack_patterns(names)
    offn = offn.astype(np.int32)
    U = Universe((ch, off, exp), (chn, offn, expected_packed("hd16 sequence names", o, chn, offn, -1)))
    n_base = len(off) - 1
    named = [U.ids(*terms) for terms, _, _ in NAMED]
    b = SeqBatch.of(U, [[]] + cut_into_sequences(list(range(n_base)), np.random.default_rng(23)) + named + [[]])
    # the corner cases, on the judge's answer
    per = b.per_sequence(T, len(t16))
    assert [len(u) for u in per[-1 - len(NAMED):-1]] == [k for _, k, _ in NAMED]
    assert len(per[0]) == 0 and len(per[-1]) == 0 and b.query_off[1] == 0 and b.query_off[-2] == b.n
    sizes = np.diff(b.query_off)
    assert sizes.max() == 12 and (sizes == 0).sum() > 10 and b.total > 900_000 and (b.status == 9).sum() == 1
    n_out = np.array([len(u) for u in per])
    assert (n_out > 16).sum() > 5 and (n_out == 1).any() and ((n_out == 0) & (sizes > 0)).sum() > 20
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
    want = b.judge(T, len(t16), max_lines)
    got, spans, st, occ = host_sequence(fm, b, max_lines)
    check_sequence(got, spans, want, "host form, max_lines %d" % max_lines)
    assert (st == b.status).all() and (occ == b.counts).all()
    rc, dev, dspans = dev_sequence(hd_filled, b, max_lines)
    assert rc == 0, last_error()
    check_sequence(dev, dspans, want, "device form, max_lines %d" % max_lines)  # (the sentinel intact behind d_line_off[q])
    # spans off: the same lines, nothing stored where the spans would go
    got2, none, _, _ = host_sequence(fm, b, max_lines, want_spans=False)
    check_sequence(got2, None, want, "host form without spans, max_lines %d" % max_lines)
    rc, dev2, untouched = dev_sequence(hd_filled, b, max_lines, want_spans=False)
    assert rc == 0, last_error()
    check_sequence(dev2, None, want, "device form without spans, max_lines %d" % max_lines)
    assert (untouched == SENT).all()
    if max_lines in (0, 16):  # d_locs with slots behind hit_off[n]
        rc, dev, dspans = dev_sequence(hd_filled, b, max_lines, extra_hits=37)
        assert rc == 0, last_error()
        check_sequence(dev, dspans, want, "device form, n_hits beyond hit_off[n], max_lines %d" % max_lines)


def test_named_sequences_against_re(hd):
    t16, o, T, U, b0, fm = hd
    for terms in sorted({t for terms, _, _ in NAMED for t in terms}):  # the oracle's hits of these terms are the text's occurrences
        assert (np.sort(U.hits[U.ids(terms)[0]]) == occurrences_in_text(HD, terms)).all(), terms
    text_lines = HD.split("\n")[:2000]
    for terms, in_order, _ in NAMED:
        rl, rs = re_judge(HD, "\n", terms, 2000)
        assert len(rl) == in_order
        lines, spans = fm.match_sequence(terms, want_spans=True)
        assert lines.dtype == np.int32 and (lines == rl).all() and (spans == rs).all(), terms
        assert (fm.match_sequence(terms) == rl).all() and list(fm.match_sequence(terms, max_lines=5)) == list(rl[:5])
        assert fm.grep(sequence=terms, max_lines=3) == [(int(k), text_lines[k]) for k in rl[:3]]
    got = fm.grep(sequence=["PacketResponder", "terminating"])
    assert len(got) == 310 and all(ln.index("PacketResponder") < ln.index("terminating") for _, ln in got)
    assert len(fm.match_sequence([])) == 0 and (fm.match_sequence("blk_") == fm.match_lines("blk_")).all()
    assert len(fm.match_sequence("\n")) == 0 and len(fm.match_lines("\n")) == 2000  # the boundary itself runs over its line's end
    with pytest.raises(IndexError):
        fm.match_sequence(["INFO", ""])
    with pytest.raises(ValueError):
        fm.grep("INFO", sequence=["INFO"])
    # ignore_case: class patterns as terms
    low = [ln.lower() for ln in text_lines]
    fwd = [k for k, ln in enumerate(low) if "block" in ln and "namesystem" in ln[ln.index("block") + 5:]]
    rev = [k for k, ln in enumerate(low) if "namesystem" in ln and "block" in ln[ln.index("namesystem") + 10:]]
    assert len(fwd) == 653 and len(rev) == 659
    assert list(fm.match_sequence(["block", "namesystem"], ignore_case=True)) == fwd
    lines, spans = fm.match_sequence(["namesystem", "block"], ignore_case=True, want_spans=True)
    assert list(lines) == rev and len(fm.match_sequence(["block", "namesystem"])) == 0
    start, _ = fm.line_bounds(lines)
    assert all(low[k][a - s:e - s].startswith("namesystem") and low[k][a - s:e - s].endswith("block") for k, s, (a, e) in zip(lines, start, spans))
    assert [k for k, _ in fm.grep(sequence=["block", "namesystem"], ignore_case=True, max_lines=4)] == fwd[:4]


def test_skew_one_heavy_sequence_and_many_light_terms(hd):
    t16, o, T, U, b0, fm = hd
    # ONE sequence of twelve " ": 12 x 30,094 hits, an answer of 1,757 lines
    b = SeqBatch.of(U, [U.ids(*SP12)])
    assert b.q == 1 and b.total == 12 * 30094
    for max_lines in (0, 7):
        want = b.judge(T, len(t16), max_lines)
        assert list(want[0][2]) == [1757]
        got, spans, st, occ = host_sequence(fm, b, max_lines)
        check_sequence(got, spans, want, "one heavy sequence, host form")
        assert (occ == 30094).all()
        rc, dev, dspans = dev_sequence(filled(fm, b), b, max_lines)
        assert rc == 0, last_error()
        check_sequence(dev, dspans, want, "one heavy sequence, device form")
    # 3,000 terms of at most one hit each (the batch of test_gpu_match_lines' skew test), in pairs
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
    # ... paired as they follow each other in the text, every other pair the wrong way round
    where = np.array([expl[0][expl[1][i]] if expl[4][i] else 2**31 - 1 for i in range(3000)])
    by_pos = [int(i) for i in np.argsort(where, kind="stable")]
    bl = SeqBatch.of(Universe((chl, offl, expl)), [by_pos[2 * i:2 * i + 2][::-1 if i % 2 else 1] for i in range(1500)])
    want = bl.judge(T, len(t16), 0)
    assert set(want[0][2]) == {0, 1}  # (a pair in order on one line; a pair that is not)
    got, spans, st, occ = host_sequence(fm, bl, 0)
    check_sequence(got, spans, want, "1,500 light sequences, host form")
    assert (occ == bl.counts).all()
    rc, dev, dspans = dev_sequence(filled(fm, bl), bl, 0)
    assert rc == 0, last_error()
    check_sequence(dev, dspans, want, "1,500 light sequences, device form")


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
        want = b.judge(T, len(t16), 0)
        got, spans, st, occ = host_sequence(fm, b, 0)
        check_sequence(got, spans, want, what)
        assert (st == b.status).all() and (occ == b.counts).all()
        first = _BETWEEN.setdefault("first", got + (spans,))
        assert all((a == r).all() for a, r in zip(got + (spans,), first)), what + ": vs the first residency"
    finally:
        fm.close()


def test_quirk_text_follows_the_reference_hits_and_table():
    """the run-block text (it derails walks: quirk Q1) with its most frequent symbol as the boundary: the answer follows the
    oracle's hits and the oracle's table, whatever positions they report"""
    text = run_block_text()
    t16 = ia.as_chars(text)
    syms, cnt = np.unique(t16, return_counts=True)
    boundary = int(syms[np.argmax(cnt)])
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, boundary)
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in syms])
    off = off.astype(np.int32)
    exp = expected_packed("runblocks16", o, ch, off, -1)  # (the batch of test_gpu_match_lines: computed once)
    truth = np.sort(np.concatenate([np.flatnonzero(t16 == s) for s in syms]))
    assert not np.array_equal(np.sort(exp[0]), truth) or not np.array_equal(T, np.flatnonzero(t16 == boundary))  # the oracle's answer is not the text's
    U = Universe((ch, off, exp))
    k = len(syms)
    order = np.random.default_rng(5).permutation(k)
    sequences = [[int(order[i]), int(order[(i + 1) % k])] for i in range(k)]
    sequences += [[int(order[i]), int(order[i + 2]), int(order[i])] for i in range(0, k - 2, 8)] + [[i] for i in range(0, k, 8)]
    b = SeqBatch.of(U, sequences)
    want = b.judge(T, len(t16), 0)
    assert (want[0][2] > 0).sum() > k
    fm = ia.FmIndex(text, 16, True, device=0)
    try:
        assert fm.build_line_table(boundary) == judge_n_lines(T, len(t16))
        got, spans, st, occ = host_sequence(fm, b, 0)
        check_sequence(got, spans, want, "run blocks, host form")
        assert (occ == b.counts).all()
        rc, dev, dspans = dev_sequence(filled(fm, b), b, 0)
        assert rc == 0, last_error()
        check_sequence(dev, dspans, want, "run blocks, device form")
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
        n = len(U.pats)
        b = SeqBatch.of(U, [list(range(i, min(i + 3, n))) for i in range(0, n, 3)])
        assert b.total == len(t16)  # 2 M packed hits
        T = judge_table(o, NL)
        assert fm.build_line_table("\n") == judge_n_lines(T, len(t16))
        key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
        assert ia.lib.fmx_hit_lines_geometry(fm.handle, b.total, C.byref(key_grid), C.byref(flat_grid)) == 0
        assert 3 * key_grid.value * 1024 <= b.total and 3 * flat_grid.value * 256 <= b.total  # every loop over hits runs at least three times
        per = b.per_sequence(T, len(t16))
        proper = False
        for Q, sq in enumerate(b.sequences):  # a sequence on a proper, non-empty subset of the lines that hold all its terms
            holds = None
            for t in sq:
                lines_t = np.unique(np.searchsorted(T, U.hits[t], side="left"))
                holds = lines_t if holds is None else np.intersect1d(holds, lines_t)
            proper |= 0 < len(per[Q]) < len(holds)
        assert proper
        want = b.judge(T, len(t16), 0)
        assert int(want[0][1][-1]) > len(T) // 2
        got, spans, st, occ = host_sequence(fm, b, 0)
        check_sequence(got, spans, want, "2 M hits, host form")
        rc, dev, dspans = dev_sequence(filled(fm, b), b, 0)
        assert rc == 0, last_error()
        check_sequence(dev, dspans, want, "2 M hits, device form")
    finally:
        fm.close()


def test_errors_and_edges(hd):
    t16, o, T, U = hd[:4]
    E_ARG = ia._lib.E_ARG
    torch = _torch()
    fm = ia.FmIndex(HD, 16, True, device=0)
    try:
        assert fm.line_table_info() == (-1, 0, 0)
        b = SeqBatch.of(U, [U.ids("blk_", "/"), U.ids("PacketResponder", "terminating")])
        host = ia.lib.fmx_match_sequence_batch

        def call(bb=b, query_off=None, lo=None, out=None, sp=None):
            qo = bb.query_off if query_off is None else np.array(query_off, np.int32)
            return host(fm.handle, bb.ch.ctypes.data, bb.off.ctypes.data, bb.n, qo.ctypes.data, len(qo) - 1, 0, lo.ctypes.data, C.byref(out),
                        None if sp is None else C.byref(sp), None, None, None)

        # no table: FMX_E_ARG, and the message names the call that makes one
        line_off = np.full(3, SENT, np.int64)
        buf, sp = C.c_void_p(0x1234), C.c_void_p(0x1234)
        assert call(lo=line_off, out=buf, sp=sp) == E_ARG and "fmx_line_table_build" in last_error()
        assert buf.value is None and sp.value is None and (line_off == SENT).all()
        d = filled(fm, b)
        rc, _, _ = dev_sequence(d, b, 0)
        assert rc == E_ARG and "fmx_line_table_build" in last_error()
        assert fm.build_line_table("\n") == 2000
        untouched = lambda dev, spans: (dev[1] == SENT).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all() and (spans == SENT).all()
        # a workspace that is too small: an error, nothing is launched, nothing is written
        rc, dev, spans = dev_sequence(d, b, 0, ws_bytes=ia.lib.fmx_sequence_lines_scratch_bytes(b.n, b.q, d.total) - 256)
        assert rc == E_ARG and untouched(dev, spans)
        # a bad query_off, a negative length: likewise
        for bad in (dict(query_off=[1, 2, 4]), dict(query_off=[0, 3, 2]), dict(query_off=[0, 5, 4]), dict(query_off=[0, 2, 3]),
                    dict(term_len=[4, 1, -1, 11])):
            rc, dev, spans = dev_sequence(d, b, 0, **bad)
            assert rc == E_ARG and untouched(dev, spans), bad
            if "query_off" in bad:
                buf.value = 0x1234
                assert call(lo=line_off, out=buf, **bad) == E_ARG and buf.value is None and (line_off == SENT).all(), bad
        want = b.judge(T, len(t16), 0)
        assert list(want[0][2]) == [1013, 310]
        rc, dev, spans = dev_sequence(d, b, 0)
        assert rc == 0, last_error()
        check_sequence(dev, spans, want, "two sequences")
        # the lengths are the caller's: a "/" of 40 characters, and the lines where it stands nearer to the end are gone
        longer = SeqBatch(b.term_hits, [4, 40, 15, 11], [[0, 1], [2, 3]])
        wl = longer.judge(T, len(t16), 0)
        assert 0 < wl[0][2][0] < 1013
        rc, dev, spans = dev_sequence(d, longer, 0)
        assert rc == 0, last_error()
        check_sequence(dev, spans, wl, "the caller's lengths")
        # q == 0 (then n == 0): the one offset is zeroed, nothing else is written
        none = SeqBatch.of(U, [])
        h = np.full(1, SENT, np.int64)
        assert call(bb=none, lo=h, out=buf) == 0 and h[0] == 0 and buf.value is None
        d_off = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
        zero = np.zeros(1, np.int32)
        assert ia.lib.fmx_sequence_lines_of_hits_dev(fm.handle, 0, 0, zero.ctypes.data, None, None, None, 0, 0, d_off.data_ptr(), None, None, None,
                                                     None, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert int(d_off.cpu()[0]) == 0
        # sequences without terms
        out = fm.match_sequence_batch(np.zeros(0, np.uint16), [0], [0, 0, 0], 0, want_counts=True, want_spans=True)
        assert len(out[0]) == 0 and list(out[1]) == [0, 0, 0] and list(out[3]) == [0, 0] and out[5].shape == (0, 2)
        # a batch without hits (device form: n_hits == 0 — the offsets are zeroed, nothing else is written)
        ch0, off0 = ia.pack_patterns(["zzzzqq#", "", "qqqqzz#"])
        off0 = off0.astype(np.int32)
        b0 = SeqBatch.of(Universe((ch0, off0, expected_packed("hd16 query no hits", o, ch0, off0, -1))), [[0, 1], [2], []])
        got, spans, st, occ = host_sequence(fm, b0, 0)
        assert (got[0] == SENT).all() and (got[1] == 0).all() and list(st) == [0, 9, 0] and (got[2] == 0).all() and (occ == 0).all()
        d0 = filled(fm, b0)
        assert d0.total == 0
        rc, dev, spans = dev_sequence(d0, b0, 0)
        assert rc == 0 and (dev[1] == 0).all() and (dev[0] == SENT).all() and (dev[2] == SENT).all() and (spans == SENT).all()
        # the wrong handle kinds
        sa = ia.SuffixArray("banana", device=None, build_device=-1)
        sa.construct()
        rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
        wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
        for other in (sa._h, rrr._h, wt._h):
            buf.value = 0x1234
            assert host(other, b.ch.ctypes.data, b.off.ctypes.data, b.n, b.query_off.ctypes.data, b.q, 0, line_off.ctypes.data, C.byref(buf), None,
                        None, None, None) == E_ARG and buf.value is None
        # resident again: the table is gone with the rest of the resident state
        fm.to_device(0)
        assert fm.line_table_info() == (-1, 0, 0)
        assert call(lo=line_off, out=buf) == E_ARG and "fmx_line_table_build" in last_error()
    finally:
        fm.close()


def test_two_host_threads_on_one_index(hd):
    t16, o, T, U, b, fm = hd
    small = SeqBatch.of(U, [U.ids(*terms) for terms, _, _ in NAMED])
    batches = [b, small]
    serial = [fm.match_sequence_batch(x.ch, x.off, x.query_off, 0, want_counts=True, want_spans=True) for x in batches]
    for x, res in zip(batches, serial):
        want = x.judge(T, len(t16), 0)
        assert (res[0] == want[0][0]).all() and (res[1] == want[0][1]).all() and (res[5] == want[1]).all()
    results, errors = [None, None], []

    def run(k):
        try:
            x = batches[k]
            results[k] = [fm.match_sequence_batch(x.ch, x.off, x.query_off, 0, want_counts=True, want_spans=True) for _ in range(2)]
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(2):
        for res in results[k]:
            assert all(a.shape == r.shape and (a == r).all() for a, r in zip(res, serial[k]))


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_match_sequence_mirror.cpp prints what matchSequenceBatch / matchSequence return"""
    t16, o, T, U, b0, fm = hd
    exe = str(tmp_path / "test_match_sequence_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_match_sequence_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    seqs = [["PacketResponder", "terminating"], ["terminating", "PacketResponder"], ["blk_", "blk_", "blk_"], [], ["blk_", "/"], COLON5]
    bm = SeqBatch.of(U, [U.ids(*s) for s in seqs])
    (lines, line_off, line_count), spans = bm.judge(T, len(t16), 0)
    assert out["n_lines"] == [2000]
    assert out["batch_offsets"] == list(line_off) and out["batch_lines"] == list(lines) and out["batch_spans"] == list(spans.reshape(-1))
    assert out["batch_line_count"] == list(line_count) == [310, 0, 3, 0, 1013, 305] and out["batch_occurrences"] == list(bm.counts)
    (clines, coff, ccount), _ = bm.judge(T, len(t16), 7)
    assert out["cut_offsets"] == [0, 7, 7, 10, 10, 17, 24] == list(coff) and out["cut_lines"] == list(clines) and out["cut_spans"] == []
    assert out["cut_line_count"] == [310, 0, 3, 0, 1013, 305]
    mine = list(bm.per_sequence(T, len(t16))[0])
    assert out["one"] == mine and out["one_cut"] == mine[:3]

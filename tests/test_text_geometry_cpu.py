"""The texts of tests/geometry_cases.py on the CPU: the text-only judge against the oracle, the host mirrors of the line stack
(tests/match_lines_hostsim.cpp, match_query_hostsim.cpp, sequence_hostsim.cpp, values_hostsim.cpp, extract_packed_hostsim.cpp) at
every case's real `count` with 4096 fences against that judge, and the geometry each case is named for — so that an edit to the
generator cannot quietly move a case off its edge, and so that the judge is proven here before a GPU sees it
(tests/test_gpu_text_geometry.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import geometry_cases as gc
import index4j_amd as ia
import orc
from common import hdfs_text
from test_extract_packed_cpu import PAD as PAD16, PackedSim, SENT16
from test_field_values_cpu import check_values, judge_values, run_hostsim
from test_locate_all_cpu import SENT, corner_batch, expected_packed
from test_match_lines_cpu import check_lines, judge_table, probe_positions, ptr, sim_lib as lines_sim_lib, sim_lines
from test_match_query_cpu import sim_lib as query_sim_lib, sim_query
from test_match_sequence_cpu import SeqBatch, check_sequence, sim_lib as sequence_sim_lib, sim_sequence

SR = 4
FENCES = 4096  # kLineFences
MAX_LINES = (0, 1, 3)
MAX_LENS = (1, 4, 64)
# Texts on which the reference does not answer the text (quirk rows) would be judged by the oracle's hits instead of by the text,
# and are to be listed here by name; at most 3 may be.  None of the texts trips one: every case is judged from the text alone.
ORACLE_JUDGED = ()
# the fence shift and fm_bits(count) each count_K is named for: 4096 -> 4097, 8192 -> 8193 and 16384 -> 16385 step the shift,
# 2^k - 1 -> 2^k steps the bits
SHIFT_OF = {1: 0, 2: 0, 3: 0, 4095: 0, 4096: 0, 4097: 1, 8191: 1, 8192: 1, 8193: 2, 16385: 3, 32767: 3, 32768: 3, 32769: 4}
BITS_OF = {1: 1, 2: 2, 3: 2, 4095: 12, 4096: 13, 4097: 13, 8191: 13, 8192: 14, 8193: 14, 16385: 15, 32767: 15, 32768: 16, 32769: 16}
# `count` of the two texts every GPU test of the line stack used before these: the HDFS fixture and synth_log(1 << 21)
OLD_COUNTS = {"hdfs": 2000, "synth_log(1 << 21)": 16777}


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    d = tmp_path_factory.mktemp("text_geometry_hostsim")
    return types.SimpleNamespace(dir=d, lines=lines_sim_lib(d), query=query_sim_lib(d), sequence=sequence_sim_lib(d))


_ORACLE = {}


def oracle_answer(c):
    """(oracle, T, expected_packed of the case's batch), once per case"""
    if c.name not in _ORACLE:
        o = orc.OracleFmIndex(c.units(), SR, True)
        _ORACLE[c.name] = (o, judge_table(o, gc.NL), expected_packed(("text geometry", c.name), o, c.ch, c.off, -1))
    return _ORACLE[c.name]


def agrees_with_the_text(c):
    o, T, (packed, hit_off, status, _, counts) = oracle_answer(c)
    hits = c.hits()
    return (np.array_equal(T, np.array(c.T, np.int32)) and np.array_equal(status, c.status) and
            all(np.array_equal(np.sort(packed[hit_off[i]:hit_off[i + 1]]), hits[i]) for i in range(c.n)))


@pytest.mark.parametrize("name", gc.names())
def test_judge_against_the_oracle(name):
    """the oracle's hits equal the text's occurrences, pattern by pattern; its table is the text's boundaries; its extract of the
    lines and of the windows behind the hits is the text's"""
    c = gc.case(name)
    assert agrees_with_the_text(c) == (name not in ORACLE_JUDGED)
    if name in ORACLE_JUDGED:
        return
    o, T, (packed, hit_off, status, _, counts) = oracle_answer(c)
    assert (counts == [len(h) for h in c.hits()]).all()
    for stop, max_len in ((gc.NL, 4), (c.stops[-1], 64)):
        want = c.values(stop, max_len)
        by_oracle = judge_values(o, packed, hit_off, c.lens, stop, max_len)
        check_values((want.chars, want.text_off, want.counts, want.val_off), by_oracle, "%s: values, stop %r max_len %d" % (name, stop, max_len))
    ids = c.line_ids()
    start, stop = c.bounds(ids)
    if len(ids) and int((stop - start).max()) > 0:
        dst, out_len, st = o.extract_batch(start, stop, int((stop - start).max()), 0, threads=8, fill=SENT16)
        assert (st == 0).all() and [ia.chars_to_str(dst[i, :out_len[i]]) for i in range(len(ids))] == \
            [ia.chars_to_str(gc.units(s)) for s in c.line_texts(ids)]


def test_how_many_texts_fall_back_to_the_oracles_hits():
    assert len(ORACLE_JUDGED) == 0 and set(ORACLE_JUDGED) <= set(gc.names())
    assert sum(not agrees_with_the_text(gc.case(name)) for name in gc.names()) == 0


def ordered_hits(c, any_case=False):
    """the batch's packed hits (ascending per pattern: the mirrors sort, as the kernels do)"""
    hits = c.hits(any_case)
    return np.concatenate(hits + [np.zeros(0, np.int32)]).astype(np.int32), np.concatenate([[0], np.cumsum([len(h) for h in hits])]).astype(np.int64)


class Windows:
    """what run_hostsim of tests/test_field_values_cpu.py reads of a judged answer: the windows behind the hits, cut from the text"""

    def __init__(self, c, locs, hit_off, max_len, want):
        u = c.units()
        which = np.repeat(np.arange(c.n), np.diff(hit_off))
        s = np.clip(locs.astype(np.int64) + c.lens[which], 0, c.text_len)
        e = np.minimum(s + max_len, c.text_len)
        at = np.minimum(s[:, None] + np.arange(max_len)[None, :], max(c.text_len - 1, 0))
        self.rows = u[at] if len(u) else np.zeros((len(s), max_len), np.uint16)
        self.starts, self.stops, self.lengths = s.astype(np.int32), e.astype(np.int32), e - s
        self.val_off, self.counts, self.text_off, self.chars = want.val_off, want.counts, want.text_off, want.chars


@pytest.mark.parametrize("name", [n for n in gc.names() if n not in ORACLE_JUDGED])
def test_host_mirrors_against_the_judge(sims, name):
    c = gc.case(name)
    T = np.array(c.T, np.int32)
    T_ = np.ascontiguousarray(T if len(T) else np.zeros(1, np.int32))
    n = c.text_len
    # fm_line_of over the fences the kernels stage, fm_line_total, fm_line_bounds
    ps = probe_positions(T, n)
    got = np.full(len(ps), SENT, np.int32)
    nf = C.c_int32(-1)
    shift = sims.lines.sim_line_of(ptr(T_), c.count, FENCES, ptr(ps), len(ps), ptr(got), C.byref(nf))
    assert (got == np.searchsorted(T, ps, side="left")).all(), name
    assert nf.value == -(-c.count >> shift) <= FENCES and (shift == 0 or -(-c.count >> (shift - 1)) > FENCES)
    assert sims.lines.sim_line_total(ptr(T_), c.count, n) == c.n_lines
    ids = np.arange(-1, c.n_lines + 1, dtype=np.int32)
    start, stop = np.full(len(ids), SENT, np.int32), np.full(len(ids), SENT, np.int32)
    sims.lines.sim_line_bounds(ptr(T_), c.count, c.n_lines, n, ptr(ids), len(ids), ptr(start), ptr(stop))
    es, ee = c.bounds(ids)
    assert (start == es).all() and (stop == ee).all() and start[0] == -1 == start[-1]
    # the stages: lines, queries, sequences
    locs, hit_off = ordered_hits(c)
    total = int(hit_off[-1])
    qb = types.SimpleNamespace(packed=locs, hit_off=hit_off, n=c.n, q=len(c.query_off) - 1, kinds=c.kinds, query_off=c.query_off)
    seq_hits = c.seq_hits()
    sb = SeqBatch(seq_hits, [len(t) for t in c.seq_terms], [list(range(a, b)) for a, b in zip(c.seq_off[:-1], c.seq_off[1:])])
    assert (sb.query_off == c.seq_off).all()
    if total == 0:  # the early return of every stage: the offsets are zeroed and nothing else is written
        assert sb.total == 0
        for res in (sim_lines(sims.lines, T, FENCES, hit_off, locs, 0, 0)[0], sim_query(sims.query, T, FENCES, qb, 0, 0)[0],
                    sim_sequence(sims.sequence, T, n, FENCES, sb, 0, 0)[0]):
            assert (res[1] == 0).all() and (res[0] == SENT).all() and (res[2] == SENT).all()
        assert all(len(x) == 0 for x in c.lines(0)[0:1] + c.queries(0)[0:1] + c.sequence_packed(0)[0][0:1])
        return
    for max_lines in MAX_LINES:
        for n_hits in (total, total + 37):
            what = "%s max_lines %d n_hits %d" % (name, max_lines, n_hits)
            res, bits = sim_lines(sims.lines, T, FENCES, hit_off, locs, n_hits, max_lines)
            check_lines(res, c.lines(max_lines), what + ", lines", tail=SENT)
            assert bits == sims.lines.sim_bits(c.n) + sims.lines.sim_bits(c.count)
            res, width = sim_query(sims.query, T, FENCES, qb, n_hits, max_lines)
            check_lines(res, c.queries(max_lines), what + ", queries", tail=SENT)
        want = c.sequence_packed(max_lines)
        for n_hits, want_spans in ((sb.total, True), (sb.total + 37, max_lines == 0)):
            res, spans, width = sim_sequence(sims.sequence, T, n, FENCES, sb, n_hits, max_lines, want_spans)
            check_sequence(res, spans, want, "%s max_lines %d, sequences" % (name, max_lines))
        by_hits = sb.judge(T, n, max_lines)  # (the backward pass of tests/test_match_sequence_cpu.py and re agree)
        assert all((a == b).all() for a, b in zip(by_hits[0] + (by_hits[1],), want[0] + (want[1],)))
    # the values: fm_val_window and the grouping passes over the text's windows
    for k, (stop_set, max_len) in enumerate((s, m) for s in c.stops for m in MAX_LENS):
        want = c.values(stop_set, max_len)
        win = Windows(c, locs, hit_off, max_len, want)
        res, runs = run_hostsim(sims.dir, win, locs, hit_off, c.lens, stop_set, max_len, n, extra_hits=37 * (k % 2), form=("bitmap", "list")[k % 2])
        check_values(res, want, "%s: values, stop %r max_len %d" % (name, stop_set, max_len))
    # the packed extract over the lines
    ids = c.line_ids()
    a, b = c.bounds(ids)
    chars, text_off, st, info = PackedSim(sims.dir, c.units(), SR).packed(a, b)
    texts = c.line_texts(ids)
    assert (st == 0).all() and (np.diff(text_off) == [len(s) for s in texts]).all()
    assert (chars[:int(text_off[-1])] == gc.units("".join(texts))).all() and (chars[int(text_off[-1]):] == SENT16).all() and len(chars) == text_off[-1] + PAD16


def test_the_table_has_the_geometry_its_names_promise(sims):
    names = gc.names()
    assert len(names) == len(set(names)) and max(gc.case(n).text_len for n in names) <= 130_000
    for K in gc.COUNT_KS:
        for closed in (True, False):
            c = gc.case("count_%d%s" % (K, "" if closed else "_open"))
            assert c.count == K == len(c.T) and c.text.endswith(gc.NL) == closed and c.n_lines == K + (0 if closed else 1)
            assert set(c.text) <= set(gc.ALPHA6 + gc.NL) and all(1 <= len(s) <= 3 for s in c.text.split(gc.NL)[:c.n_lines])
            nf = C.c_int32(-1)
            T = np.array(c.T, np.int32)
            p = np.zeros(1, np.int32)
            assert sims.lines.sim_line_of(ptr(T), K, FENCES, ptr(p), 1, ptr(p.copy()), C.byref(nf)) == SHIFT_OF[K]
            assert sims.lines.sim_bits(K) == BITS_OF[K] == K.bit_length()
            assert (c.n_lines - 1).bit_length() <= BITS_OF[K] and (closed or sims.lines.sim_bits(c.n_lines - 1) == BITS_OF[K])  # the last line's id
    c = gc.case("no_boundary")
    assert c.count == 0 and c.n_lines == 1 and c.text_len == 5000
    assert [gc.case(n).text for n in ("only_boundary", "single_a", "a_boundary", "boundary_a")] == ["\n", "a", "a\n", "\na"]
    c = gc.case("empty_lines")
    assert c.count == c.text_len == c.n_lines == 5000
    c = gc.case("leading_and_double")
    assert c.text.startswith("\n\n") and "\n\n" in c.text[2:] and not c.text.endswith(gc.NL) and c.T[:2] == [0, 1]
    c = gc.case("giant_line")
    assert c.text_len == 65536 and c.T == [32768] and set(c.text) == set("ab\n")
    for name, lone, every in (("period1", "a", 997), ("period2", "ab", 1001)):
        c = gc.case(name)
        assert c.text.replace(gc.NL, "") == lone * 4000 and c.T == list(range(every, c.text_len, every + 1)) and not c.text.endswith(gc.NL)
        for p in ("a", "aa", "aaa", "ab", "ba", "aba"):
            assert p in c.patterns
        h = c.hits()[c.patterns.index("aa" if name == "period1" else "aba")]
        assert (np.diff(h) <= len(lone)).sum() > 3900  # every hit overlaps its neighbour
        assert sum(len(v) < 64 for v, _ in c.values("", 64).per[c.patterns.index("a")]) >= 63 // len(lone)  # the last windows are all cut at textLength
    c = gc.case("high_units")
    assert set(map(ord, c.text)) == set(gc.HIGH) | {10} and 0xFFFE not in set(map(ord, c.text))
    got = [v for v, _ in c.values(gc.NL, 64).per[c.patterns.index(gc.HIGH_PREFIX)]]
    variants = gc.high_variants()
    assert got == sorted(variants) and len(set(variants)) == 1 + 4 * 6
    assert sorted(variants) == sorted(variants, key=lambda v: [ord(x) for x in v])  # (the order of str is the code units')
    for k in gc.CHUNK_EDGES:
        rest = gc.HIGH_BASE[:k] + gc.HIGH_BASE[k + 1:]
        assert {v[k] for v in variants if v[:k] + v[k + 1:] == rest} == {chr(u) for u in gc.HIGH}  # every unit at every chunk edge
    assert all(sum(a != b for a, b in zip(v, gc.HIGH_BASE)) <= 1 and len(v) == 10 for v in variants)  # ... and no other difference
    # batch sizes on both sides of the powers of two; the padding inside one tile's slice of hit_off, on both sides of the slice
    sizes = {gc.case(n).n for n in names}
    assert sizes == {1, 3, 2047, 2048, 2049, 4097}
    for name in names:
        c = gc.case(name)
        if c.n >= 2047:
            hit_off = np.concatenate([[0], np.cumsum([len(h) for h in c.hits()])]).tolist()
            assert (c.widest_slice(hit_off) > gc.SLICE) == (c.n == 4097), name
    for name in gc.RESIDENT:
        assert name in names
    assert sum(len(h) for h in gc.case("only_boundary_no_hits").hits()) == 0 and sum(len(h) for h in gc.case("only_boundary_no_hits").seq_hits()) == 0


def test_the_old_suite_never_left_the_slice_and_its_two_counts():
    """the corner batch of the GPU suites (tests/test_gpu_locate_all.py: corner_batch over the fixture, 2,900 random patterns) never
    needs more than kLocateAllSlice entries of hit_off for a tile, so the route that searches hit_off where it lies ran on no GPU
    before the batches of 4,097 patterns; and the two values `count` took there"""
    HD = hdfs_text()
    t16 = ia.as_chars(HD)
    ch, off = corner_batch(t16, np.random.default_rng(16), 2900, min_len=2)
    counts, _ = orc.OracleFmIndex(HD, 16, True).count_batch(ch, off, threads=8)
    probe = types.SimpleNamespace(n=len(counts))
    assert gc.Case.widest_slice(probe, np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).tolist()) <= gc.SLICE
    assert HD.count("\n") == OLD_COUNTS["hdfs"] and int((ia.as_chars(ia.synth_log(1 << 21)) == 10).sum()) == OLD_COUNTS["synth_log(1 << 21)"]
    for count in OLD_COUNTS.values():
        assert count not in gc.COUNT_KS and (count <= 4096 or 16384 < count <= 32768)  # shift 0 and shift 3, 11 and 15 bits: nothing between

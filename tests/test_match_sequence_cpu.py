"""The lines that hold a SEQUENCE of terms in order (fmx_sequence_lines_of_hits_dev, fmx_match_sequence_batch; grep 'A.*B') on the
CPU: the functions the kernels of fmx_sequence_lines.hip run — the key term | position and its unpacking, fm_seq_key_width,
fm_seq_lower_bound, fm_seq_head, fm_seq_chain, fm_seq_flag — compiled for the host and driven by a mirror of the stages
(tests/sequence_hostsim.cpp; the device-wide sort = std::sort, the scans = running sums).

The judge is the oracle plus numpy, never the code under test.  The hits of a term are the oracle's (expected_packed, Universe of
tests/test_match_query_cpu.py), T is judge_table's, the bounds of a line are judge_bounds'.  Whether line L belongs to a sequence
t_0 .. t_{k-1} is decided by a BACKWARD pass — the opposite direction to the kernel's earliest-fit rule:

    need_{k-1} = the largest hit h of t_{k-1} with h + len_{k-1} <= stop(L)
    need_j     = the largest hit h of t_j with h + len_j <= need_{j+1}
    L matches iff need_0 exists and need_0 >= start(L)

(if need_0 >= start then every need_j is: they only grow with j).  The spans of the named sequences, and their lines once more,
come from Python's `re` on the fixture's lines — ".*?".join(map(re.escape, terms)), m.start() / m.end() plus the line's start —
after the test has asserted that the oracle's hits of those terms are exactly the text's occurrences.  The spans of the large
batches are judged by judge_spans (numpy: the smallest hit of t_0 in the line, then term by term the smallest hit at or behind the
bound), which the named sequences check against `re` too.  The GPU suite (tests/test_gpu_match_sequence.py) shares the helpers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_locate_all_cpu import SENT, expected_packed
from test_match_lines_cpu import MAX_LINES, batch_for, check_lines, judge_bounds, judge_n_lines, judge_table, ptr, texts
from test_match_query_cpu import Universe, cut_into_queries

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
_SIM = {}
NOWHERE = -(1 << 40)

# the named sequences and their lines on the fixture: in order, then in any order (match_query(all=...))
SP12, COLON5 = [" "] * 12, [":"] * 5
NAMED = [
    (["PacketResponder", "terminating"], 310, 310),
    (["terminating", "PacketResponder"], 0, 310),
    (["blk_", "blk_"], 266, 1999),
    (["blk_", "blk_", "blk_"], 3, 1999),
    (["/", "blk_"], 400, 1140),
    (["blk_", "/"], 1013, 1140),
    (["from", "of size"], 0, 242),
    (["terminat", "ting"], 0, 310),  # (the two overlap inside "terminating")
    (SP12, 1757, 2000),
    (COLON5, 305, 2000),
]


# ---- the judge -------------------------------------------------------------------------------------------------------------
def line_bounds(T, text_len):
    """(start, stop) of every line of the text, as int64 arrays"""
    n_lines = judge_n_lines(T, text_len)
    start, stop = judge_bounds(T, n_lines, text_len, np.arange(n_lines))
    return start.astype(np.int64), stop.astype(np.int64)


def judge_sequence(hits, lens, start, stop):
    """the lines of ONE sequence by the backward pass; hits[j]: the hits of term j (any order, any int32), lens[j] its length"""
    if not hits or min(len(h) for h in hits) == 0:
        return np.zeros(0, np.int32)
    need = stop.copy()
    for h, m in zip(hits[::-1], lens[::-1]):
        H = np.sort(np.asarray(h, np.int64))
        at = np.searchsorted(H, need - int(m), side="right") - 1  # the largest hit with h + len <= need
        need = np.where((at >= 0) & (need > NOWHERE), H[np.maximum(at, 0)], NOWHERE)
    return np.flatnonzero(need >= start).astype(np.int32)


def judge_spans(hits, lens, start, stop, lines):
    """[span_start, span_stop) of the matching `lines` of one sequence: forwards, the earliest hit that fits, term by term"""
    H = [np.sort(np.asarray(h, np.int64)) for h in hits]
    first = H[0][np.searchsorted(H[0], start[lines], side="left")]
    at = first + int(lens[0])
    for h, m in zip(H[1:], lens[1:]):
        at = h[np.searchsorted(h, at, side="left")] + int(m)
    assert (at <= stop[lines]).all()  # (the backward pass said these lines match: the forward chain must fit them)
    return np.stack([first, at], axis=1).astype(np.int32)


class SeqBatch:
    """sequences = a list of lists of term ids into (hits, lens): the batch of TERMS as the calls take it, and its judged answer"""

    def __init__(self, hits, lens, sequences, pats=None, status=None, counts=None):
        self.sequences = sequences
        ids = [t for sq in sequences for t in sq]
        self.query_off = np.concatenate([[0], np.cumsum([len(sq) for sq in sequences])]).astype(np.int32)
        self.term_hits = [np.asarray(hits[i], np.int32) for i in ids]
        self.term_len = np.array([lens[i] for i in ids], np.int32)
        self.packed = np.concatenate(self.term_hits + [np.zeros(0, np.int32)]).astype(np.int32)
        self.hit_off = np.concatenate([[0], np.cumsum([len(h) for h in self.term_hits])]).astype(np.int64)
        self.n, self.q, self.total = len(ids), len(sequences), int(self.hit_off[-1])
        if pats is not None:
            ch, off = ia.pack_patterns([pats[i] for i in ids])
            self.ch, self.off = np.ascontiguousarray(ch), off.astype(np.int32)
            assert (np.diff(self.off) == self.term_len).all()
            self.status = np.array([status[i] for i in ids], np.int32)
            self.counts = np.array([counts[i] for i in ids], np.int32)
        for a in (self.query_off, self.term_len, self.packed, self.hit_off):
            a.setflags(write=False)
        self._judged = {}

    @classmethod
    def of(cls, U, sequences):
        return cls(U.hits, [len(p) for p in U.pats], sequences, U.pats, U.status, U.counts)

    def terms_of(self, Q):
        t = range(self.query_off[Q], self.query_off[Q + 1])
        return [self.term_hits[i] for i in t], [int(self.term_len[i]) for i in t]

    def per_sequence(self, T, text_len):
        if "per" not in self._judged:
            start, stop = line_bounds(T, text_len)
            per, spans = [], []
            for Q in range(self.q):
                hits, lens = self.terms_of(Q)
                lines = judge_sequence(hits, lens, start, stop)
                per.append(lines)
                spans.append(judge_spans(hits, lens, start, stop, lines) if len(lines) else np.zeros((0, 2), np.int32))
            self._judged["per"], self._judged["spans"] = per, spans
        return self._judged["per"]

    def judge(self, T, text_len, max_lines):
        """((lines, line_off, line_count), spans) of the sequences; once per limit, read-only"""
        per = self.per_sequence(T, text_len)
        if max_lines not in self._judged:
            cut = (lambda u: u[:max_lines]) if max_lines > 0 else (lambda u: u)
            kept = [cut(u) for u in per]
            line_off = np.concatenate([[0], np.cumsum([len(u) for u in kept])]).astype(np.int64)
            lines = np.concatenate(kept + [np.zeros(0, np.int32)]).astype(np.int32)
            spans = np.concatenate([cut(s) for s in self._judged["spans"]] + [np.zeros((0, 2), np.int32)]).astype(np.int32)
            res = ((lines, line_off, np.array([len(u) for u in per], np.int32)), spans)
            for a in res[0] + (spans,):
                a.setflags(write=False)
            self._judged[max_lines] = res
        return self._judged[max_lines]


def check_sequence(got, spans, want, what):
    """lines, offsets and counts as check_lines has them, then the spans of the stored lines; the sentinel behind both"""
    (elines, eoff, ecount), espans = want
    check_lines(got, (elines, eoff, ecount), what, tail=SENT)
    if spans is not None:
        total = int(eoff[-1])
        sp = np.asarray(spans).reshape(-1)
        bad = np.flatnonzero(sp[:2 * total].reshape(total, 2) != espans)
        assert len(bad) == 0, "%s: %d span entries differ, first at %r" % (what, len(bad), bad[:5])
        assert (sp[2 * total:] == SENT).all(), what + ": spans stored beyond line_off[q]"


def occurrences_in_text(text, term):
    out, at = [], text.find(term)
    while at >= 0:
        out.append(at)
        at = text.find(term, at + 1)
    return np.array(out, np.int32)


def re_judge(text, boundary, terms, n_lines):
    """(lines, spans) of one sequence of literal terms by Python's re, line by line"""
    rx = re.compile(".*?".join(map(re.escape, terms)), re.S)
    lines, spans, at = [], [], 0
    for k, ln in enumerate(text.split(boundary)[:n_lines]):
        m = rx.search(ln)
        if m:
            lines.append(k)
            spans.append((at + m.start(), at + m.end()))
        at += len(ln) + 1
    return np.array(lines, np.int32), np.array(spans, np.int32).reshape(len(lines), 2)


def cut_into_sequences(ids, rng, most=6):
    """consecutive pattern ids cut into sequences of 0 .. most terms (the cut of test_match_query_cpu, the kinds dropped)"""
    return [[pid for pid, _ in qu] for qu in cut_into_queries(ids, rng, most)]


# ---- the host build --------------------------------------------------------------------------------------------------------
def sim_lib(tmpdir):
    if "lib" not in _SIM:
        so = os.path.join(str(tmpdir), "libsequencehostsim.so")
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "sequence_hostsim.cpp")])
        L = C.CDLL(so)
        vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
        L.sim_seq_key_width.argtypes = [i32]
        L.sim_seq_key.restype = u64
        L.sim_seq_key.argtypes = [i32, i32, vp]
        L.sim_seq_lower_bound.restype = i64
        L.sim_seq_lower_bound.argtypes = [vp, i64, i64, i64]
        L.sim_sequence_lines.argtypes = [vp, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp]
        _SIM["lib"] = L
    return _SIM["lib"]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return sim_lib(tmp_path_factory.mktemp("sequence_hostsim"))


def bits(v):
    return max(int(v).bit_length(), 1)


def sim_sequence(L, T, text_len, fences, b, n_hits, max_lines, want_spans=True, pad=8):
    T_ = np.ascontiguousarray(T if len(T) else np.zeros(1, np.int32))
    locs = np.concatenate([b.packed, np.full(max(n_hits - len(b.packed), 0) + 1, SENT, np.int32)]).astype(np.int32)
    line_off = np.full(b.q + 1, SENT, np.int64)
    lines = np.full(n_hits + pad, SENT, np.int32)
    spans = np.full(2 * (n_hits + pad), SENT, np.int32)
    line_count = np.full(max(b.q, 1), SENT, np.int32)
    lens = np.ascontiguousarray(b.term_len if b.n else np.zeros(1, np.int32))
    width = L.sim_sequence_lines(ptr(T_), len(T), judge_n_lines(T, text_len), text_len, fences, b.n, b.q, ptr(b.query_off), ptr(lens), ptr(b.hit_off),
                                 ptr(locs), n_hits, max_lines, ptr(line_off), ptr(lines), ptr(line_count), ptr(spans) if want_spans else None)
    return (lines, line_off, line_count[:b.q]), spans if want_spans else None, width


def cpu_batch(name):
    text, boundary = texts()[name]
    t16 = ia.as_chars(text)
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, boundary)
    ch, off = batch_for(name, text, t16, T, boundary)
    exp = expected_packed(("match lines cpu", name), o, ch, off, -1)  # (the batch of test_match_lines_cpu: computed once)
    return T, Universe((ch, off, exp)), text, boundary


@pytest.mark.parametrize("name", list(texts()))
def test_stages_against_the_judge(L, name):
    T, U, text, boundary = cpu_batch(name)
    n = len(text)
    ids = list(range(len(U.pats)))
    inside = np.array([not (p == ord(boundary)).any() for p in U.pats])  # (a pattern that holds the boundary matches nowhere)
    heavy = int(np.argmin(np.where(inside, np.abs(np.array(U.counts) - 2000), 1 << 30)))  # (on the fixture a pattern of some 2,000 hits)
    # the corner batch in its own order, cut into sequences of 0 to 6 terms; then every pattern behind that one and in front of
    # it, and that one twice
    sequences = [[]] + cut_into_sequences(ids, np.random.default_rng(11)) + [[heavy, i] for i in ids] + [[i, heavy] for i in ids]
    sequences += [[heavy, heavy], [heavy], []]
    b = SeqBatch.of(U, sequences)
    per = b.per_sequence(T, n)
    sizes = np.diff(b.query_off)
    assert sizes.max() == 6 and sizes.min() == 0 and (b.status == 9).sum() >= 1
    assert len(per[0]) == 0 and len(per[-1]) == 0
    if name.startswith("hdfs"):
        pairs = per[-3 - 2 * len(ids):-3]
        behind, before = pairs[:len(ids)], pairs[len(ids):]
        assert sum(len(a) > 0 and len(a) != len(c) for a, c in zip(behind, before)) > 20  # the order matters for many pairs
        assert len(per[-3]) <= len(per[-2]) and len(per[-2]) > 0
        assert sum(len(u) > 0 for u in per) > 50
    for max_lines in MAX_LINES:
        want = b.judge(T, n, max_lines)
        for fences, n_hits, want_spans in ((4096, b.total, True), (0, b.total, False), (3, b.total + 37, True)):
            got, spans, w = sim_sequence(L, T, n, fences, b, n_hits, max_lines, want_spans)
            assert w == bits(b.n) + 32 == L.sim_seq_key_width(b.n)
            check_sequence(got, spans, want, "%s max_lines %d fences %d n_hits %d" % (name, max_lines, fences, n_hits))


def test_named_sequences(L):
    text, boundary = texts()["hdfs"]
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, boundary)
    names = sorted({t for terms, _, _ in NAMED for t in terms})
    ch, off = ia.pack_patterns(names)
    U = Universe((np.ascontiguousarray(ch), off.astype(np.int32), expected_packed("sequence names", o, ch, off.astype(np.int32), -1)))
    for i, s in enumerate(names):  # the oracle's hits of these terms are exactly the text's occurrences
        assert (np.sort(U.hits[i]) == occurrences_in_text(text, s)).all(), s
    b = SeqBatch.of(U, [U.ids(*terms) for terms, _, _ in NAMED])
    per = b.per_sequence(T, len(text))
    per_term = [np.unique(np.searchsorted(T, h, side="left")) for h in U.hits]
    for (terms, in_order, any_order), lines in zip(NAMED, per):  # the counts, on the judge first
        assert len(lines) == in_order, terms
        both = per_term[U.ids(terms[0])[0]]
        for t in U.ids(*terms):
            both = np.intersect1d(both, per_term[t])
        assert len(both) == any_order, terms
    want = b.judge(T, len(text), 0)
    got, spans, _ = sim_sequence(L, T, len(text), 4096, b, b.total, 0)
    check_sequence(got, spans, want, "named sequences")
    for Q, (terms, in_order, _) in enumerate(NAMED):  # ... and against re, spans included
        rl, rs = re_judge(text, boundary, terms, judge_n_lines(T, len(text)))
        a, e = got[1][Q], got[1][Q + 1]
        assert (got[0][a:e] == rl).all() and (spans.reshape(-1, 2)[a:e] == rs).all(), terms


def hand(L, text, sequences, max_lines=0, hits=None, lens=None, boundary="\n"):
    """a hand-made text: the terms' hits are the text's occurrences (or `hits`); returns (per-sequence lines, per-sequence spans)
    of the stages after they have been checked against the judge"""
    terms = sorted({t for sq in sequences for t in sq})
    T = occurrences_in_text(text, boundary)
    if hits is None:
        hits, lens = [occurrences_in_text(text, t) for t in terms], [len(t) for t in terms]
    b = SeqBatch(hits, lens, [[terms.index(t) for t in sq] for sq in sequences])
    want = b.judge(T, len(text), max_lines)
    for fences in (4096, 0, 1):
        got, spans, _ = sim_sequence(L, T, len(text), fences, b, b.total, max_lines)
        check_sequence(got, spans, want, "%r %r" % (text, sequences))
    lo = got[1]
    sp = spans.reshape(-1, 2)
    return [list(got[0][lo[Q]:lo[Q + 1]]) for Q in range(b.q)], [[tuple(r) for r in sp[lo[Q]:lo[Q + 1]]] for Q in range(b.q)]


def test_the_rule_by_hand(L):
    # in order and not; adjacent terms touch (h + len == the next hit); a term may not overlap its predecessor
    lines, spans = hand(L, "abcd\ncdab\nabab\naba\n", [["ab", "cd"], ["cd", "ab"], ["ab", "ab"], ["aba", "ba"], ["ab", "b"]])
    assert lines == [[0], [1], [2], [], [2]]
    assert spans[0] == [(0, 4)] and spans[1] == [(5, 9)] and spans[2] == [(10, 14)] and spans[4] == [(10, 14)]
    # the leftmost start and the earliest end — not the tightest window ("a..ab": the window "ab" at 3 is tighter)
    lines, spans = hand(L, "a..ab\n", [["a", "b"]])
    assert lines == [[0]] and spans == [[(0, 5)]]
    # a term that is a whole line; len reaching exactly stop; the same one character longer runs over the boundary
    lines, spans = hand(L, "xy\nabc\nxy", [["abc"], ["x", "y"], ["bc"], ["bc\n"], ["y\na"], ["xy"]])
    assert lines == [[1], [0, 2], [1], [], [], [0, 2]]
    assert spans[0] == [(3, 6)] and spans[1] == [(0, 2), (7, 9)] and spans[5] == [(0, 2), (7, 9)]  # (the last line has no boundary)
    # a first-term hit ON the boundary character: the boundary belongs to the line it ends, and nothing fits behind it there
    lines, _ = hand(L, "a\nb\n\nc", [["\n"], ["\n", "b"], ["\nb"], ["a", "\n"], ["b"], ["c"]])
    assert lines == [[], [], [], [], [1], [3]]
    # two hits of the first term on one line: the line once; the second term is also the first
    lines, spans = hand(L, "blk_1 blk_2\nblk_3\nx blk_4 y blk_5 blk_6\n", [["blk_", "blk_"], ["blk_", "blk_", "blk_"], ["blk_"]], max_lines=0)
    assert lines == [[0, 2], [2], [0, 1, 2]] and spans[0] == [(0, 10), (20, 32)] and spans[1] == [(20, 38)]
    assert hand(L, "blk_1 blk_2\nblk_3\nx blk_4 y blk_5 blk_6\n", [["blk_", "blk_"], ["blk_"]], max_lines=1)[0] == [[0], [0]]
    # a sequence without terms, and one with a term without hits, have no lines
    assert hand(L, "ab\nab\n", [[], ["ab", "zz"], ["zz", "ab"], ["ab"]])[0] == [[], [], [], [0, 1]]


def test_equal_positions_and_the_signed_order(L):
    """hits as a quirk row may report them: any int32, the same position twice, in any order"""
    text = "ab ab\nab\n"  # T = [5, 8]; lines [0, 5), [6, 8); the text is 9 characters long
    I = 2**31 - 1
    # term 0: "ab" with its hits doubled, two negative positions and positions behind the text; term 1: a 2-character term at 3, 3, -4
    hits = [np.array([6, 0, 3, 0, 6, -1, -I - 1, I, 9, 40], np.int32), np.array([3, -4, 3], np.int32), np.array([I - 1], np.int32)]
    lines, spans = hand(L, text, [["t0"], ["t0", "t1"], ["t1", "t0"], ["t0", "t2"], ["t2"]], hits=hits, lens=[2, 2, 2])
    #        equal positions open a line once; -1 and -2^31 lie before line 0; 9, 40 and 2^31 - 1 lie behind the text
    assert lines == [[0, 1], [0], [], [], []] and spans[0] == [(0, 2), (6, 8)] and spans[1] == [(0, 5)]
    # h + len beyond 2^31 - 1 does not wrap: a term of 2^31 - 1 characters at 2^31 - 2
    assert hand(L, text, [["t0", "t1"], ["t1"]], hits=[np.array([0], np.int32), np.array([I - 1], np.int32)], lens=[2, I])[0] == [[], []]
    out = np.zeros(2, np.int32)
    vals = [-I - 1, -I, -2, -1, 0, 1, 2, 2000, I - 1, I]
    keys = [L.sim_seq_key(t, v, ptr(out)) for t in (0, 1, 5, I) for v in vals]
    for k, (t, v) in zip(keys, [(t, v) for t in (0, 1, 5, I) for v in vals]):
        assert k == (t << 32) | ((v + 2**31) & 0xffffffff) and k < 2**63
        L.sim_seq_key(t, v, ptr(out))
        assert list(out) == [t, v]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)  # the order of the keys is the order of (term, signed position)
    for n, w in ((0, 33), (1, 33), (2, 34), (2000, 43), (I, 63)):
        assert L.sim_seq_key_width(n) == w
    pos = np.array([-5, -5, 0, 3, 3, 3, 9, I], np.int32)
    for lo, hi in ((0, 8), (2, 6), (3, 3), (5, 8)):
        for at in (-2**33, -6, -5, -4, 0, 1, 3, 4, 9, 10, I, I + 1, 2**33):
            assert L.sim_seq_lower_bound(ptr(pos), lo, hi, at) == lo + int(np.searchsorted(pos[lo:hi].astype(np.int64), at, side="left"))


def test_one_term_is_match_lines_less_the_hits_over_the_end():
    T, U, text, boundary = cpu_batch("hdfs")
    b = SeqBatch.of(U, [[i] for i in range(len(U.pats))])
    per = b.per_sequence(T, len(text))
    nl = ord(boundary)
    holds = 0
    for i, lines in enumerate(per):
        plain = np.unique(np.searchsorted(T, U.hits[i], side="left"))
        if (U.pats[i] == nl).any():  # a pattern that holds the boundary runs over its line's end everywhere
            holds += 1
            assert len(lines) == 0 and len(plain) > 0
        else:
            assert (lines == plain).all()
    assert holds >= 3  # (with_boundary_patterns' three, the boundary itself among them)


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_sequence_lines_scratch_bytes", "fmx_sequence_lines_of_hits_dev", "fmx_match_sequence_batch", "fmx_match_sequence_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("This is a long string\n", 4, True, device=None)
    ch, off = ia.pack_patterns(["is", "long", "string"])
    off = off.astype(np.int32)
    qoff = np.array([0, 2, 3], np.int32)
    line_off = np.full(3, SENT, np.int64)
    buf, sp = C.c_void_p(0x1234), C.c_void_p(0x1234)
    host = ia.lib.fmx_match_sequence_batch

    def call(h=fm._h, off_=off, n=3, qoff_=qoff, q=2, lo=line_off, out=buf):
        return host(h, ch.ctypes.data, None if off_ is None else off_.ctypes.data, n, None if qoff_ is None else qoff_.ctypes.data, q, 0,
                    None if lo is None else lo.ctypes.data, None if out is None else C.byref(out), C.byref(sp), None, None, None)

    assert call() == E_NO_DEVICE
    assert buf.value is None and sp.value is None and (line_off == SENT).all()  # *lines = *spans = NULL on every failure, nothing written
    for bad in (dict(h=None), dict(n=-1), dict(q=-1), dict(off_=None), dict(qoff_=None), dict(lo=None), dict(out=None),
                dict(qoff_=np.array([1, 2, 3], np.int32)),      # does not start at 0
                dict(qoff_=np.array([0, 3, 2], np.int32)),      # decreases (and does not end at n)
                dict(qoff_=np.array([0, 4, 3], np.int32)),      # decreases, ends at n
                dict(qoff_=np.array([0, 1, 2], np.int32))):     # does not end at n
        buf.value = sp.value = 0x1234
        assert call(**bad) == E_ARG, bad
        assert (buf.value is None or "out" in bad) and sp.value is None and (line_off == SENT).all()
    alt, pos_off, pat_off = ia.pack_class_patterns([ia.ignore_case("is"), ia.ignore_case("long")])
    klass = ia.lib.fmx_match_sequence_class_batch
    two = np.array([0, 2], np.int32)

    def ccall(h=fm._h, qoff_=two, max_ranges=16):
        return klass(h, alt.ctypes.data, pos_off.ctypes.data, len(pos_off) - 1, pat_off.ctypes.data, 2, max_ranges, qoff_.ctypes.data, 1, 0,
                     line_off.ctypes.data, C.byref(buf), None, None, None, None)

    assert ccall() == E_NO_DEVICE and buf.value is None
    assert ccall(qoff_=np.array([0, 1], np.int32)) == E_ARG and ccall(max_ranges=0) == E_ARG and ccall(h=None) == E_ARG
    ids = np.zeros(4, np.int32)
    hit_off = np.zeros(4, np.int64)
    lens = np.array([2, 4, 6], np.int32)
    dev = ia.lib.fmx_sequence_lines_of_hits_dev

    def dcall(h=fm._h, n=3, q=2, qoff_=qoff, lens_=lens, n_hits=2, lo=line_off):
        return dev(h, n, q, None if qoff_ is None else qoff_.ctypes.data, None if lens_ is None else lens_.ctypes.data, hit_off.ctypes.data,
                   ids.ctypes.data, n_hits, 0, None if lo is None else lo.ctypes.data, ids.ctypes.data, None, None, None, 0, None)

    assert dcall() == E_NO_DEVICE
    for bad in (dict(h=None), dict(n=-1), dict(q=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(qoff_=None), dict(lens_=None), dict(lo=None),
                dict(qoff_=np.array([1, 2, 3], np.int32)), dict(qoff_=np.array([0, 3, 2], np.int32)), dict(qoff_=np.array([0, 1, 2], np.int32)),
                dict(lens_=np.array([2, -1, 6], np.int32))):
        assert dcall(**bad) == E_ARG, bad
    assert (line_off == SENT).all()
    sb = ia.lib.fmx_sequence_lines_scratch_bytes
    assert sb(0, 2, 5) == 0 and sb(5, 0, 5) == 0 and sb(5, 2, 0) == 0 and sb(5, 2, 1 << 31) == 0 and sb(-1, 2, 5) == 0
    assert sb(3, 2, 1000) >= 36 * 1000 and sb(3, 2, 1000) % 256 == 0
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert call(h=h) == E_ARG and dcall(h=h) == E_ARG and ccall(h=h) == E_ARG
    # the Python mirror: an empty term raises as match_lines("") does, before anything runs; without a device the call says so
    for terms in ([""], ["is", ""], ""):
        with pytest.raises(IndexError, match="ArrayIndexOutOfBoundsException"):
            fm.match_sequence(terms)
    with pytest.raises(ia.FmxError) as e:
        fm.match_sequence(["is", "long"])
    assert e.value.code == E_NO_DEVICE
    for kw in (dict(pattern="is"), dict(all=["is"]), dict(any="is"), dict(none=["is"])):
        with pytest.raises(ValueError):
            fm.grep(sequence=["is", "long"], **kw)

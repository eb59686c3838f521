"""The lines that match a QUERY of several terms (fmx_query_lines_of_hits_dev, fmx_match_query_batch) on the CPU: the functions the
kernels of fmx_query_lines.hip run — the key query | line | term and its unpacking, fm_query_key_width, the per-group word
(fm_query_word, fm_query_word_join, fm_query_contribution), fm_query_matches, fm_query_first_group — compiled for the host and driven
by a mirror of the stages (tests/match_query_hostsim.cpp; the device-wide sort = std::stable_sort, the reduction by key = one pass).

The judge is the oracle plus numpy, never the code under test: the lines of a TERM are judge_lines' of tests/test_match_lines_cpu.py
(T = the oracle's locate() of the boundary, sorted; np.unique(np.searchsorted(T, the oracle's hits))), the lines of a QUERY are

    the intersection over its ALL terms, intersected with the union over its ANY terms if it has any, less the union over its NONE terms

by np.intersect1d / np.union1d / np.setdiff1d, and nothing for a query without an ALL and without an ANY term; the limit and the
offsets follow.  The GPU suite (tests/test_gpu_match_query.py) shares the helpers below."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from test_locate_all_cpu import SENT, expected_packed
from test_match_lines_cpu import MAX_LINES, batch_for, check_lines, judge_lines, judge_table, ptr, sim_lib as lines_sim_lib, sim_lines, texts

HERE = os.path.dirname(os.path.abspath(__file__))
ALL, ANY, NONE = 0, 1, 2
_SIM = {}


# ---- the judge -------------------------------------------------------------------------------------------------------------
class Universe:
    """patterns with the oracle's answers: parts = (chars, offsets, expected_packed(...)) batches; pattern ids run through them"""

    def __init__(self, *parts):
        self.pats, self.hits, self.status, self.counts = [], [], [], []
        for ch, off, exp in parts:
            packed, hit_off, status, _, counts = exp
            for i in range(len(off) - 1):
                self.pats.append(np.asarray(ch[off[i]:off[i + 1]]))
                self.hits.append(np.asarray(packed[hit_off[i]:hit_off[i + 1]]))
                self.status.append(int(status[i]))
                self.counts.append(int(counts[i]))

    def ids(self, *strings):
        names = [ia.chars_to_str(p) for p in self.pats]
        return [names.index(s) for s in strings]


class TermBatch:
    """queries = a list of lists of (pattern id, kind): the batch of TERMS as the calls take it, and the oracle's packed hits of it"""

    def __init__(self, U, queries):
        self.queries = queries
        ids = [pid for qu in queries for pid, _ in qu]
        self.kinds = np.array([k for qu in queries for _, k in qu], np.uint8)
        self.query_off = np.concatenate([[0], np.cumsum([len(qu) for qu in queries])]).astype(np.int32)
        ch, off = ia.pack_patterns([U.pats[i] for i in ids])
        self.ch, self.off = np.ascontiguousarray(ch), off.astype(np.int32)
        self.packed = np.concatenate([U.hits[i] for i in ids] + [np.zeros(0, np.int32)]).astype(np.int32)
        self.hit_off = np.concatenate([[0], np.cumsum([len(U.hits[i]) for i in ids])]).astype(np.int64)
        self.status = np.array([U.status[i] for i in ids], np.int32)
        self.counts = np.array([U.counts[i] for i in ids], np.int32)
        self.n, self.q, self.total = len(ids), len(queries), int(self.hit_off[-1])
        for a in (self.kinds, self.query_off, self.ch, self.off, self.packed, self.hit_off, self.status, self.counts):
            a.setflags(write=False)
        self._judged = {}

    def term_lines(self, T):
        lines, line_off, _ = judge_lines(T, self.packed, self.hit_off, 0)
        return [lines[line_off[t]:line_off[t + 1]] for t in range(self.n)]

    def judge(self, T, max_lines):
        """(lines, line_off, line_count) of the queries: the set formula over judge_lines' per-term lines; once per limit, read-only"""
        if "per" not in self._judged:
            per_term, per = self.term_lines(T), []
            for Q in range(self.q):
                terms = range(self.query_off[Q], self.query_off[Q + 1])
                alls = [per_term[t] for t in terms if self.kinds[t] == ALL]
                anys = [per_term[t] for t in terms if self.kinds[t] == ANY]
                nones = [per_term[t] for t in terms if self.kinds[t] == NONE]
                if not alls and not anys:
                    per.append(np.zeros(0, np.int32))
                    continue
                res = None
                for a in alls:
                    res = a if res is None else np.intersect1d(res, a)
                if anys:
                    u = anys[0]
                    for a in anys[1:]:
                        u = np.union1d(u, a)
                    res = u if res is None else np.intersect1d(res, u)
                for a in nones:
                    res = np.setdiff1d(res, a)
                per.append(np.asarray(res, np.int32))
            self._judged["per"] = per
        if max_lines not in self._judged:
            per = self._judged["per"]
            kept = [u[:max_lines] if max_lines > 0 else u for u in per]
            line_off = np.concatenate([[0], np.cumsum([len(u) for u in kept])]).astype(np.int64)
            lines = np.concatenate(kept + [np.zeros(0, np.int32)]).astype(np.int32)
            res = (lines, line_off, np.array([len(u) for u in per], np.int32))
            for a in res:
                a.setflags(write=False)
            self._judged[max_lines] = res
        return self._judged[max_lines]

    def per_query(self, T):
        self.judge(T, 0)
        return self._judged["per"]


def truth_table(h, light, zero, empty):
    """queries over the pattern ids h[0..3] (many lines), light[0..1] (few), zero (no hits), empty (the empty pattern): every row
    of the truth table — ALL only, ANY only, ALL + ANY, each with and without NONE, NONE only, no terms — the same term twice, the
    empty pattern and a pattern without hits as each kind; returns (queries, their names)"""
    rows = {
        "ALL": [(h[0], ALL)],
        "ALL ALL": [(h[1], ALL), (h[2], ALL)],
        "ALL ALL ALL": [(h[0], ALL), (h[1], ALL), (h[2], ALL)],
        "ANY": [(light[0], ANY)],
        "ANY ANY": [(h[1], ANY), (light[0], ANY)],
        "ALL + ANY": [(h[0], ALL), (h[1], ANY), (light[0], ANY)],
        "ALL - NONE": [(h[0], ALL), (h[1], NONE)],
        "ALL - NONE NONE": [(h[0], ALL), (light[0], NONE), (light[1], NONE)],
        "ANY - NONE": [(h[0], ANY), (h[2], ANY), (h[1], NONE)],
        "ALL + ANY - NONE": [(h[0], ALL), (h[2], ANY), (h[3], ANY), (h[1], NONE)],
        "kinds interleaved": [(h[1], NONE), (h[2], ANY), (h[0], ALL), (light[0], NONE), (h[3], ANY)],
        "NONE only": [(h[0], NONE)],
        "NONE NONE only": [(light[0], NONE), (h[1], NONE)],
        "no terms": [],
        "twice ALL": [(h[0], ALL), (h[0], ALL)],
        "twice ANY - itself": [(h[1], ANY), (h[1], ANY), (h[1], NONE)],
        "ALL and NONE of one term": [(h[0], ALL), (h[0], NONE)],
        "empty as ALL": [(h[0], ALL), (empty, ALL)],
        "empty as NONE": [(h[0], ALL), (empty, NONE)],
        "empty as ANY": [(empty, ANY), (h[0], ANY)],
        "empty as the only ANY": [(h[0], ALL), (empty, ANY)],
        "no hits as ALL": [(h[0], ALL), (zero, ALL)],
        "no hits as NONE": [(h[0], ALL), (zero, NONE)],
        "no hits as the only ANY": [(zero, ANY)],
    }
    return list(rows.values()), list(rows)


def cut_into_queries(ids, rng, most=6):
    """consecutive pattern ids cut into queries of 0 .. most terms, kinds from the generator"""
    out, at = [], 0
    while at < len(ids):
        k = (most, 0, 3)[len(out)] if len(out) < 3 else int(rng.integers(0, most + 1))
        out.append([(pid, int(rng.integers(0, 3))) for pid in ids[at:at + k]])
        at += k
    return out


def pick(U, T):
    """pattern ids for truth_table from the judge's data: h[0] has the most lines; h[1], h[2] are, where the batch has such a pair,
    two patterns on fewer lines whose lines overlap without one holding the other's; h[3] one more; two with the fewest lines (but
    some), one without hits, the empty one"""
    per = [np.unique(np.searchsorted(T, hits, side="left")) for hits in U.hits]
    n_lines = np.array([len(u) for u in per])
    lens = np.array([len(p) for p in U.pats])
    order = [int(i) for i in np.argsort(-n_lines, kind="stable") if n_lines[i] > 0]
    assert len(order) >= 4
    partial = [i for i in order if n_lines[i] < n_lines[order[0]]][:16]
    pair = [(i, j) for i in partial for j in partial if i < j and 0 < len(np.intersect1d(per[i], per[j])) < min(n_lines[i], n_lines[j])][:1]
    h = [order[0]] + (list(pair[0]) if pair else order[1:3])
    h += [i for i in partial + order if i not in h][:1]
    some = order[::-1][:2]  # (on a tiny text they may be among the four)
    zero = int(np.flatnonzero((n_lines == 0) & (lens > 0))[0])
    empty = int(np.flatnonzero(lens == 0)[0])
    assert len(h) == 4 and U.status[empty] == 9 and U.counts[zero] == 0
    return h, some, zero, empty


# ---- the host build --------------------------------------------------------------------------------------------------------
def sim_lib(tmpdir):
    if "lib" not in _SIM:
        so = os.path.join(str(tmpdir), "libmatchqueryhostsim.so")
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "match_query_hostsim.cpp")])
        L = C.CDLL(so)
        vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
        L.sim_query_key_width.argtypes = [i32, i32, i32]
        L.sim_query_key.restype = u64
        L.sim_query_key.argtypes = [i32, i32, i32, i32, i32, vp, vp]
        L.sim_query_word.restype = u64
        L.sim_query_word.argtypes = [i32]
        L.sim_query_word_join.restype = u64
        L.sim_query_word_join.argtypes = [u64, u64]
        L.sim_query_matches.argtypes = [u64, i32, i32]
        L.sim_query_lines.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, i32, vp, vp, vp]
        _SIM["lib"] = L
    return _SIM["lib"]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return sim_lib(tmp_path_factory.mktemp("match_query_hostsim"))


def bits(v):
    return max(int(v).bit_length(), 1)


def sim_query(L, T, fences, b, n_hits, max_lines, pad=8):
    T_ = np.ascontiguousarray(T if len(T) else np.zeros(1, np.int32))
    locs = np.concatenate([b.packed, np.full(max(n_hits - len(b.packed), 0) + 1, SENT, np.int32)]).astype(np.int32)
    line_off = np.full(b.q + 1, SENT, np.int64)
    lines = np.full(n_hits + pad, SENT, np.int32)
    line_count = np.full(max(b.q, 1), SENT, np.int32)
    kinds = np.ascontiguousarray(b.kinds if b.n else np.zeros(1, np.uint8))
    width = L.sim_query_lines(ptr(T_), len(T), fences, b.n, b.q, ptr(b.query_off), ptr(kinds), ptr(b.hit_off), ptr(locs), n_hits, max_lines,
                              ptr(line_off), ptr(lines), ptr(line_count))
    return (lines, line_off, line_count[:b.q]), width


def cpu_batch(name):
    text, boundary = texts()[name]
    t16 = ia.as_chars(text)
    o = orc.OracleFmIndex(text, 16, True)
    T = judge_table(o, boundary)
    ch, off = batch_for(name, text, t16, T, boundary)
    exp = expected_packed(("match lines cpu", name), o, ch, off, -1)  # (the batch of test_match_lines_cpu: computed once)
    U = Universe((ch, off, exp))
    return T, U


@pytest.mark.parametrize("name", list(texts()))
def test_stages_against_the_judge(L, name):
    T, U = cpu_batch(name)
    h, light, zero, empty = pick(U, T)
    table, names = truth_table(h, light, zero, empty)
    rng = np.random.default_rng(11)
    #          the first and the last query have no lines: one without terms, one of NONE terms only
    queries = [[]] + table + cut_into_queries(list(range(len(U.pats))), rng) + [[(h[0], NONE), (h[1], NONE)]]
    b = TermBatch(U, queries)
    per_term, per = b.term_lines(T), b.per_query(T)
    # what the batch holds, on the judge's data
    if name.startswith("hdfs") or name == "no boundary":  # (the two hand-made texts have no such term)
        assert (np.array([len(u) for u in per_term]) < np.diff(b.hit_off)).any()  # a term with several hits on one line
    assert max(np.diff(b.query_off)) == 6 and min(np.diff(b.query_off)) == 0
    assert len(per[0]) == 0 and len(per[-1]) == 0 and b.query_off[1] == 0 and b.query_off[-2] < b.n
    row = {nm: per[1 + i] for i, nm in enumerate(names)}
    lines_of = lambda pid: np.unique(np.searchsorted(T, U.hits[pid], side="left"))
    assert len(row["ALL"]) > 0 and (row["ALL"] == lines_of(h[0])).all() and (row["twice ALL"] == row["ALL"]).all()
    assert (row["empty as NONE"] == row["ALL"]).all() and (row["no hits as NONE"] == row["ALL"]).all()
    for nm in ("NONE only", "NONE NONE only", "no terms", "twice ANY - itself", "ALL and NONE of one term", "empty as ALL", "empty as the only ANY",
               "no hits as ALL", "no hits as the only ANY"):
        assert len(row[nm]) == 0, nm
    assert (row["empty as ANY"] == row["ALL"]).all() and len(row["ANY"]) > 0
    assert set(row["ALL ALL"]) <= set(lines_of(h[1])) and set(row["ALL - NONE"]) == set(row["ALL"]) - set(lines_of(h[1]))
    if name.startswith("hdfs"):
        assert 0 < len(row["ALL ALL"]) < min(len(lines_of(h[1])), len(lines_of(h[2])))  # a proper, non-empty intersection
        assert 0 < len(row["ALL - NONE"]) < len(row["ALL"])                              # NONE takes some lines, not all
        assert len(row["ALL + ANY"]) > 0 and len(row["ALL + ANY - NONE"]) > 0 and len(row["kinds interleaved"]) > 0
        assert len(row["ANY ANY"]) > max(len(lines_of(h[1])), len(lines_of(light[0]))) or set(lines_of(light[0])) <= set(lines_of(h[1]))
    assert sum(len(u) > 0 for u in per) > 5
    width = bits(b.q) + bits(len(T)) + bits(6)
    for max_lines in MAX_LINES:
        want = b.judge(T, max_lines)
        if max_lines == 1 and name.startswith("hdfs"):
            assert (want[2] > 1).any() and (np.diff(want[1]) <= 1).all()
        for fences, n_hits in ((4096, b.total), (0, b.total), (3, b.total + 37)):
            got, w = sim_query(L, T, fences, b, n_hits, max_lines)
            assert w == width == L.sim_query_key_width(b.q, len(T), 6)
            check_lines(got, want, "%s max_lines %d fences %d n_hits %d" % (name, max_lines, fences, n_hits), tail=SENT)


@pytest.mark.parametrize("name", ["hdfs", "empty lines", "no boundary"])
def test_one_all_term_per_query_is_match_lines(L, name, tmp_path_factory):
    """q queries of ONE ALL term each: array for array what the stages of fmx_lines_of_hits_dev give for those patterns"""
    T, U = cpu_batch(name)
    b = TermBatch(U, [[(pid, ALL)] for pid in range(len(U.pats))])
    LL = lines_sim_lib(tmp_path_factory.mktemp("match_lines_hostsim_for_queries"))
    for max_lines in MAX_LINES:
        for n_hits in (b.total, b.total + 37):
            got, _ = sim_query(L, T, 4096, b, n_hits, max_lines)
            ref, _ = sim_lines(LL, T, 4096, b.hit_off, b.packed, n_hits, max_lines)
            assert all((a == r).all() for a, r in zip(got, ref)), "%s max_lines %d" % (name, max_lines)
            check_lines(got, judge_lines(T, b.packed, b.hit_off, max_lines), name, tail=SENT)


def test_edges_of_the_stages(L):
    T, U = cpu_batch("empty lines")
    h, light, zero, empty = pick(U, T)
    # no queries; queries but no terms; terms but no hits: the offsets are zeroed and nothing else is written
    for queries in ([], [[], [], []], [[(zero, ALL), (empty, ANY)], [(zero, NONE)]]):
        b = TermBatch(U, queries)
        assert b.total == 0
        got, w = sim_query(L, T, 4096, b, 0, 0)
        assert (got[1] == 0).all() and (got[0] == SENT).all() and (got[2] == SENT).all()
    # one query of every pattern as ANY: the union of everything
    b = TermBatch(U, [[(pid, ANY) for pid in range(len(U.pats))]])
    got, w = sim_query(L, T, 4096, b, b.total, 0)
    check_lines(got, b.judge(T, 0), "one wide query", tail=SENT)
    assert w == 1 + bits(len(T)) + bits(len(U.pats))


def test_keys_words_and_the_width_check(L):
    out, group = np.zeros(3, np.int32), C.c_uint64(0)
    widest = [(31, 31, 2), (31, 2, 31), (2, 31, 31), (31, 1, 31), (1, 31, 31), (11, 11, 3)]
    for qb, lb, tb in widest:
        assert qb + lb + tb <= 64
        for query, line, term in ((2**qb - 1, min(2**lb - 1, 2**31 - 1), 2**tb - 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
                                  (2**(qb - 1), min(2**(lb - 1), 2**31 - 1), 2**(tb - 1))):
            key = L.sim_query_key(query, line, term, lb, tb, ptr(out), C.byref(group))
            assert key == (((query << lb) | line) << tb) | term and key < 2**64
            assert list(out) == [query, line, term] and group.value == key >> tb
    # the order of the keys is the order of (query, line, term)
    rng = np.random.default_rng(3)
    triples = sorted({(int(a), int(b), int(c)) for a, b, c in rng.integers(0, 2**11, (400, 3))})
    keys = [L.sim_query_key(a, b_, c, 11, 11, ptr(out), C.byref(group)) for a, b_, c in triples]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # the width: bits(q) + bits(|T|) + bits(the most terms of a query); 64 is legal, 65 is not
    I = 2**31 - 1
    assert L.sim_query_key_width(0, 0, 0) == 3 and L.sim_query_key_width(2000, 2000, 6) == 11 + 11 + 3
    assert L.sim_query_key_width(I, I, 3) == 64 and L.sim_query_key_width(I, I, 4) == 65 and L.sim_query_key_width(I, I, I) == 93
    # the word of a group: the ALL terms are counted, ANY and NONE are flags; joining is associative and commutative
    A, Y, N = (L.sim_query_word(k) for k in (ALL, ANY, NONE))
    assert (A, Y, N) == (1, 1 << 32, 1 << 33)
    join = L.sim_query_word_join
    words = [0, A, Y, N, join(A, A), join(Y, N), join(join(A, Y), N), 2**31 - 1, (2**31 - 1) | Y | N]
    for a in words:
        assert join(a, 0) == a and join(Y, Y) == Y and join(N, N) == N
        for b_ in words:
            assert join(a, b_) == join(b_, a)
            for c in words:
                assert join(join(a, b_), c) == join(a, join(b_, c))
    w = 0
    for _ in range(5):
        w = join(w, A)
    assert w == 5 and join(w, join(Y, Y)) == 5 | Y
    # the predicate, every row
    m = L.sim_query_matches
    assert m(2, 2, 0) and not m(1, 2, 0) and not m(2 | N, 2, 0) and m(2 | Y, 2, 0)       # ALL only (an ANY flag cannot be there, but does no harm)
    assert m(Y, 0, 3) and not m(0, 0, 3) and not m(Y | N, 0, 3)                           # ANY only
    assert m(1 | Y, 1, 2) and not m(1, 1, 2) and not m(Y, 1, 2) and not m(1 | Y | N, 1, 2)  # ALL + ANY
    assert not m(0, 0, 0) and not m(N, 0, 0)                                              # NONE only, no terms
    assert m(2**31 - 1, 2**31 - 1, 0)


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_query_lines_scratch_bytes", "fmx_query_lines_of_hits_dev", "fmx_match_query_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("This is a long string\n", 4, True, device=None)
    ch, off = ia.pack_patterns(["is", "long", "string"])
    off = off.astype(np.int32)
    qoff, kinds = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.uint8)
    line_off = np.full(3, SENT, np.int64)
    buf = C.c_void_p(0x1234)
    host = ia.lib.fmx_match_query_batch

    def call(h=fm._h, off_=off, n=3, qoff_=qoff, kinds_=kinds, q=2, lo=line_off, out=buf):
        return host(h, ch.ctypes.data, None if off_ is None else off_.ctypes.data, n, None if qoff_ is None else qoff_.ctypes.data,
                    None if kinds_ is None else kinds_.ctypes.data, q, 0, None if lo is None else lo.ctypes.data,
                    None if out is None else C.byref(out), None, None, None)

    assert call() == E_NO_DEVICE
    assert buf.value is None and (line_off == SENT).all()  # *lines = NULL on every failure, nothing written
    for bad in (dict(h=None), dict(n=-1), dict(q=-1), dict(off_=None), dict(qoff_=None), dict(kinds_=None), dict(lo=None), dict(out=None),
                dict(qoff_=np.array([1, 2, 3], np.int32)),      # does not start at 0
                dict(qoff_=np.array([0, 3, 2], np.int32)),      # decreases (and does not end at n)
                dict(qoff_=np.array([0, 4, 3], np.int32)),      # decreases, ends at n
                dict(qoff_=np.array([0, 1, 2], np.int32)),      # does not end at n
                dict(kinds_=np.array([0, 3, 1], np.uint8))):    # a kind above 2
        buf.value = 0x1234
        assert call(**bad) == E_ARG, bad
        assert (buf.value is None or "out" in bad) and (line_off == SENT).all()
    ids = np.zeros(4, np.int32)
    hit_off = np.zeros(4, np.int64)
    dev = ia.lib.fmx_query_lines_of_hits_dev

    def dcall(h=fm._h, n=3, q=2, qoff_=qoff, kinds_=kinds, n_hits=2, lo=line_off):
        return dev(h, n, q, None if qoff_ is None else qoff_.ctypes.data, None if kinds_ is None else kinds_.ctypes.data, hit_off.ctypes.data,
                   ids.ctypes.data, n_hits, 0, None if lo is None else lo.ctypes.data, ids.ctypes.data, None, None, 0, None)

    assert dcall() == E_NO_DEVICE
    for bad in (dict(h=None), dict(n=-1), dict(q=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(qoff_=None), dict(kinds_=None), dict(lo=None),
                dict(qoff_=np.array([1, 2, 3], np.int32)), dict(qoff_=np.array([0, 3, 2], np.int32)), dict(qoff_=np.array([0, 1, 2], np.int32)),
                dict(kinds_=np.array([0, 1, 9], np.uint8))):
        assert dcall(**bad) == E_ARG, bad
    assert (line_off == SENT).all()
    sb = ia.lib.fmx_query_lines_scratch_bytes
    assert sb(0, 2, 5) == 0 and sb(5, 0, 5) == 0 and sb(5, 2, 0) == 0 and sb(5, 2, 1 << 31) == 0 and sb(-1, 2, 5) == 0
    assert sb(3, 2, 1000) >= 32 * 1000 and sb(3, 2, 1000) % 256 == 0
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert call(h=h) == E_ARG and dcall(h=h) == E_ARG
    # the Python mirror: an empty term raises as match_lines("") does, before anything runs; without a device the call says so
    for kw in (dict(all=[""]), dict(all=["is"], any=[""]), dict(all=["is"], none=["", "x"]), dict(all="")):
        with pytest.raises(IndexError, match="ArrayIndexOutOfBoundsException"):
            fm.match_query(**kw)
    with pytest.raises(ia.FmxError) as e:
        fm.match_query(all=["is"], none="long")
    assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        fm.match_query_batch(ch, off, qoff, kinds[:2])

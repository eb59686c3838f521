"""Patterns of character classes (fmx_class_*, fmx_*_class_batch) on the CPU: the functions k_class_search runs — fm_class_keep /
_rank / _first / _candidate / _advance / _survives / _slot of index4j_amd/csrc/fmx_device.hpp — compiled for the host and driven
by a serial mirror of the team loop (tests/class_search_hostsim.cpp: candidate order, compaction, both stages), over the tree
image and the compact image of the fixture and over synth_64k.  The judge is the oracle plus numpy: a class pattern's answer is
the union of the oracle's answers for the literal strings it spells (class_judge), its ranges are the pairs the literal search
(sim_count here, fmx_locate_all_ranges_dev on the GPU) leaves for those strings, ascending by start.  The GPU suite runs the kernel
itself over the same batch (tests/test_gpu_class_search.py, which shares the helpers below)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HD = hdfs_text()
SR = 16
SENT = -0x3C3C3C3D
ST_AIOOBE, ST_TOO_MANY = 9, 10
RANGES_MAX, ALTS_MAX = 1024, 64
BATCH_MAX_RANGES = 128  # the corner batch's cap: [0-9][0-9] (100 strings) fits, [0-9][0-9][0-9] does not
SMALL_MAX_RANGES = 32  # ... and a cap so small that a workgroup's teams are bounded by the `block` option, not by the LDS
_SIM = {}


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


# ---- the judge -------------------------------------------------------------------------------------------------------------
def position_units(position):
    """the distinct code units of a position's alternatives, in the order given"""
    a = ia.as_chars(position) if isinstance(position, str) else ia.as_chars([ord(x) if isinstance(x, str) else x for x in position])
    return list(dict.fromkeys(a.tolist()))


class Judged:
    """what the oracle says about ONE class pattern under a cap: status, count, the literal strings with hits (tuples of code
    units) and frontier[k - 1] = the number of distinct strings of its last k positions with oracle count > 0"""

    def __init__(self, o, pattern, max_ranges, stop_above=RANGES_MAX, threads=16):
        self.frontier, self.strings, self.count = [], [], 0
        if len(pattern) == 0:
            self.status = ST_AIOOBE
            return
        units = [position_units(p) for p in pattern]
        wide = any(len(ia.as_chars(p) if isinstance(p, str) else list(p)) > ALTS_MAX for p in pattern)
        alive = [()]
        for k in range(1, len(pattern) + 1):
            # every string of the last k positions whose suffix of k - 1 has hits (a string with hits has such a suffix)
            cand = [(u,) + s for u in units[-k] for s in alive]
            assert len(cand) <= 1 << 17
            if cand:
                ch = np.array([c for s in cand for c in s], np.uint16)
                off = (np.arange(len(cand) + 1) * k).astype(np.int32)
                counts, status = o.count_batch(ch, off, threads=threads)
                assert (status == 0).all()
            else:
                counts = np.zeros(0, np.int32)
            alive = [s for s, c in zip(cand, counts) if c > 0]
            self.frontier.append(len(alive))
            self.counts_alive = [int(c) for c in counts if c > 0]
            if not alive or len(alive) > stop_above:
                break
        if wide or max(self.frontier) > max_ranges:
            self.status = ST_TOO_MANY
            return
        self.status = 0
        if len(self.frontier) == len(pattern):
            self.strings = alive
            self.count = int(sum(self.counts_alive))


def class_judge(key, o, patterns, max_ranges, cache={}):  # noqa: B006 (computed once per key, never changed)
    if key not in cache:
        cache[key] = [Judged(o, p, max_ranges) for p in patterns]
    return cache[key]


def expected_arrays(judged, literal_ranges):
    """(range_off, ranges, counts, status) of a batch: literal_ranges(list of strings) -> their {start, end} pairs (n x 2)"""
    strings = [s for j in judged for s in j.strings]
    pairs = literal_ranges(strings) if strings else np.zeros((0, 2), np.int32)
    range_off, rows, at = [0], [], 0
    for j in judged:
        mine = pairs[at:at + len(j.strings)]
        at += len(j.strings)
        assert (mine[:, 1] > mine[:, 0]).all()
        mine = mine[np.argsort(mine[:, 0], kind="stable")]  # ascending by start
        assert (mine[1:, 0] >= mine[:-1, 1]).all()  # the ranges of different strings of one length are disjoint
        assert int((mine[:, 1] - mine[:, 0]).sum()) == j.count  # the literal search's widths are the oracle's counts
        rows.append(mine)
        range_off.append(range_off[-1] + len(mine))
    ranges = np.concatenate(rows + [np.zeros((0, 2), np.int32)]).astype(np.int32).reshape(-1)
    return (np.array(range_off, np.int64), ranges, np.array([j.count for j in judged], np.int32), np.array([j.status for j in judged], np.int32))


def pack_strings(strings):
    ch = np.array([c for s in strings for c in s], np.uint16)
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int32)
    return ch, off


# ---- the batch of the issue -------------------------------------------------------------------------------------------------
def corner_batch():
    """[(name, class pattern)]: every corner case in ONE batch"""
    lit = lambda s: [c for c in s]  # noqa: E731 (all positions singletons)
    b = [("first: no hits", ia.parse_classes("[xX]yzzy[0-9]"))]
    b += [("icase block", ia.ignore_case("block")), ("digit", ia.parse_classes("[0-9]"))]  # two heavy ones ...
    b += [("no hits %d" % i, ia.parse_classes("Qz[0-9a-c]k%d" % i)) for i in range(75)]  # ... 75 without hits between them ...
    b += [("icase info", ia.ignore_case("info")), ("icase namesystem", ia.ignore_case("namesystem")), ("icase delet", ia.ignore_case("delet"))]
    b += [("singletons", lit("NameSystem")), ("port", ia.parse_classes(":500[0-9][0-9]")), ("blk", ia.parse_classes("blk_-[0-9]"))]
    b += [("last position: first alternative unknown", lit("bloc") + ["€k"]), ("last position: all unknown", lit("bloc") + ["€é"]),
          ("unknown inside", ["b", "€l", "o", "c", "k"])]
    b += [("duplicates", ["bb", "lll", "oo", "c", "kkk"]), ("empty position", ["b", "", "o"]), ("no positions", [])]
    b += [("65 alternatives", ["b", [0x4E00 + i for i in range(64)] + [ord("l")], "o"]), ("64 alternatives", [[0x4E00 + i for i in range(63)] + [ord("l")], "o"])]
    b += [("three digits", ia.parse_classes("[0-9][0-9][0-9]")), ("six digits", ia.parse_classes("[0-9][0-9][0-9][0-9][0-9][0-9]"))]
    b += [("literal INFO", lit("INFO")), ("icase warn", ia.ignore_case("warn"))]
    b += [("last: no hits", ia.parse_classes("zz[qQ]x"))]
    return b


def assert_corner_cases(names, judged, o, t16):
    """on the JUDGE's answer, before anything else runs"""
    by = dict(zip(names, judged))
    text = ia.chars_to_str(t16)
    blk = by["icase block"]
    assert len(blk.strings) == 3 and 2 ** 5 == 32 and blk.count == 2662 == text.lower().count("block")
    assert by["icase namesystem"].count == text.lower().count("namesystem") and by["icase namesystem"].count >= 659 + 653
    for word in ("delet", "info"):
        assert by["icase " + word].count == text.lower().count(word) > 0
    assert by["singletons"].count == o.count("NameSystem") == 653 and len(by["singletons"].strings) == 1
    assert by["port"].count > 0 and by["blk"].count > 0 and len(by["blk"].strings) > 1
    assert by["last position: first alternative unknown"].count == o.count("block") == by["duplicates"].count == by["unknown inside"].count
    assert by["last position: all unknown"].count == 0 and by["last position: all unknown"].status == 0
    assert by["empty position"].status == 0 and by["empty position"].count == 0
    assert by["no positions"].status == ST_AIOOBE and by["65 alternatives"].status == ST_TOO_MANY
    assert by["64 alternatives"].status == 0 and by["64 alternatives"].count == o.count("lo")
    assert judged[0].count == 0 and judged[-1].count == 0 and judged[0].status == 0 == judged[-1].status
    quiet = [j.count == 0 and j.status == 0 for j in judged]
    run = best = 0
    for z in quiet:
        run = run + 1 if z else 0
        best = max(best, run)
    assert best >= 75 and by["digit"].count > 10000


# ---- the host build ---------------------------------------------------------------------------------------------------------
def class_lib(tmpdir, compact=False):
    if compact not in _SIM:
        so = os.path.join(str(tmpdir), "libclasssearchhostsim%s.so" % ("_compact" if compact else ""))
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared"] + (["-DFMX_COMPACT=1"] if compact else []) +
                              ["-o", so, os.path.join(HERE, "class_search_hostsim.cpp")])
        L = C.CDLL(so)
        L.sim_class_team_bytes.restype = C.c_int64
        L.sim_class_count.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p] * 4
        L.sim_class_fill.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p] * 2
        L.sim_class_hit_offsets.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.sim_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        _SIM[compact] = L
    return _SIM[compact]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("class_search_hostsim")


class ClassSim:
    """the host image of an index (tree or compact) through tests/class_search_hostsim.cpp"""

    def __init__(self, simdir, text, sr, compact=False):
        if compact:
            assert ia.lib.fmx_set_option(b"image_compact", 1) == 0
        try:
            self.fm = ia.FmIndex(text, sr, True, device=None)
            self.blob = self.fm.blob()
        finally:
            ia.lib.fmx_set_option(b"image_compact", 0)
        self.L = class_lib(simdir, compact)
        self.p = C.c_void_p(self.blob.ctypes.data)

    def literal_ranges(self, strings):
        """the {start, end} pairs the literal search (FM:455-474; the mirror of k_count) leaves"""
        ch, off = pack_strings(strings)
        n = len(strings)
        counts, rng = np.zeros(n, np.int32), np.zeros(2 * n, np.int32)
        self.L.sim_count(self.p, ptr(ch), ptr(off), n, ptr(counts), None, None, ptr(rng))
        return rng.reshape(n, 2)

    def search(self, patterns, max_ranges, teams=4, grid=3):
        """both stages; (range_off, ranges with a sentinel pair behind, counts, status, info)"""
        alt, pos_off, pat_off = ia.pack_class_patterns(patterns)
        n = len(patterns)
        range_off = np.full(n + 1, SENT, np.int64)
        counts, status = np.full(max(n, 1), SENT, np.int32), np.full(max(n, 1), SENT, np.int32)
        info = np.zeros(3, np.int64)
        self.L.sim_class_count(self.p, ptr(alt), ptr(pos_off), ptr(pat_off), n, max_ranges, teams, grid, ptr(range_off), ptr(counts), ptr(status),
                               ptr(info))
        m = int(range_off[n])
        ranges = np.full(2 * m + 2, SENT, np.int32)
        self.L.sim_class_fill(self.p, ptr(alt), ptr(pos_off), ptr(pat_off), n, max_ranges, teams, grid, ptr(range_off), ptr(ranges))
        assert (ranges[2 * m:] == SENT).all()
        return range_off, ranges[:2 * m], counts[:n], status[:n], info


def check(got, exp, what):
    for g, e, name in zip(got[:4], exp, ("range_off", "ranges", "counts", "status")):
        assert len(g) == len(e) and (np.asarray(g) == e).all(), "%s: %s differs at %r" % (what, name, np.flatnonzero(np.asarray(g) != e)[:5] if len(g) == len(e) else "length")


# ---- the mirror against the judge -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_judge():
    o = orc.OracleFmIndex(HD, SR, True)
    names, patterns = zip(*corner_batch())
    judged = class_judge(("hd", BATCH_MAX_RANGES), o, patterns, BATCH_MAX_RANGES)
    assert_corner_cases(names, judged, o, ia.as_chars(HD))
    return o, list(names), list(patterns), judged


@pytest.mark.parametrize("compact", [False, True])
def test_fixture_batch_over_tree_and_compact_image(simdir, fixture_judge, compact):
    o, names, patterns, judged = fixture_judge
    sim = ClassSim(simdir, HD, SR, compact=compact)
    exp = expected_arrays(judged, sim.literal_ranges)
    by = dict(zip(names, judged))
    assert by["three digits"].status == ST_TOO_MANY and by["six digits"].status == ST_TOO_MANY  # (under this batch's cap)
    first = None
    for teams, grid in ((4, 3), (32, 1), (1, 7), (48, 2)):
        got = sim.search(patterns, BATCH_MAX_RANGES, teams=teams, grid=grid)
        check(got, exp, "compact %r teams %d grid %d" % (compact, teams, grid))
        first = first or got
        assert (got[4] == first[4]).all()  # the same candidates and ranks whatever the launch shape
    assert first[4][2] <= BATCH_MAX_RANGES
    small = class_judge(("hd", SMALL_MAX_RANGES), o, patterns, SMALL_MAX_RANGES)
    assert small[names.index("port")].status == ST_TOO_MANY and small[names.index("icase block")].count == 2662
    check(sim.search(patterns, SMALL_MAX_RANGES, teams=64, grid=2), expected_arrays(small, sim.literal_ranges), "compact %r, the small cap" % compact)
    # grep -i keeps a handful of ranges where 2^k spellings were possible
    n_ns = names.index("icase namesystem")
    assert 2 <= exp[0][n_ns + 1] - exp[0][n_ns] <= 3
    # the hit layout: the ranges' widths summed per pattern
    m = int(exp[0][-1])
    range_hit_off, hit_off = np.full(m + 1, SENT, np.int64), np.full(len(patterns) + 1, SENT, np.int64)
    sim.L.sim_class_hit_offsets(ptr(exp[0]), len(patterns), ptr(exp[1]), m, ptr(range_hit_off), ptr(hit_off))
    assert (np.diff(hit_off) == exp[2]).all() and hit_off[0] == 0
    assert (np.diff(range_hit_off) == exp[1][1::2] - exp[1][0::2]).all()


def test_the_cap_is_exact(simdir, fixture_judge):
    """[0-9][0-9][0-9] is answered with max_ranges = the judge's largest frontier S and refused with S - 1; [0-9] x 6 passes 1,024
    after four positions"""
    o, names, patterns, _ = fixture_judge
    three, six = patterns[names.index("three digits")], patterns[names.index("six digits")]
    sim = ClassSim(simdir, HD, SR)
    free = Judged(o, three, RANGES_MAX)
    S = max(free.frontier)
    assert free.status == 0 and 100 < S <= RANGES_MAX and len(free.frontier) == 3
    for cap, status in ((S, 0), (S - 1, ST_TOO_MANY)):
        judged = class_judge(("three", cap), o, [three, ia.ignore_case("block")], cap)
        assert judged[0].status == status and judged[1].status == 0
        got = sim.search([three, ia.ignore_case("block")], cap, teams=3, grid=1)
        check(got, expected_arrays(judged, sim.literal_ranges), "three digits under a cap of %d" % cap)
        if status:
            assert got[0][1] == 0 and got[2][0] == 0  # no ranges, count 0
    wide = Judged(o, six, RANGES_MAX)
    assert wide.status == ST_TOO_MANY and len(wide.frontier) == 4 and wide.frontier[3] > RANGES_MAX >= wide.frontier[2]
    got = sim.search([six], RANGES_MAX, teams=1, grid=1)
    assert got[3].tolist() == [ST_TOO_MANY] and got[2].tolist() == [0] and got[0].tolist() == [0, 0]


def test_synth_64k(simdir):
    text = np.frombuffer(open(os.path.join(GOLDEN, "synth_64k.txt"), "rb").read(), dtype=np.uint8).astype(np.uint16)
    o = orc.OracleFmIndex(text, 8, True)
    s = ia.chars_to_str(text)
    words = sorted({w for w in s.replace("\n", " ").split(" ") if 4 <= len(w) <= 8 and w.isalpha()})[:12]
    assert len(words) >= 4
    patterns = [ia.ignore_case(w) for w in words] + [ia.parse_classes("[0-9][0-9]:[0-9]"), ia.parse_classes("[a-z][a-z]"), [], ["", "a"]]
    patterns += [ia.parse_classes(w[:2] + "[a-zA-Z]" + w[3:]) for w in words[:4]]
    judged = class_judge(("synth", 1000), o, patterns, 1000)
    assert sum(j.count for j in judged) > 1000 and judged[-5].status == 0 and judged[-6].status == ST_AIOOBE
    for i, w in enumerate(words):
        assert judged[i].count == s.lower().count(w.lower())
    sim = ClassSim(simdir, text, 8)
    exp = expected_arrays(judged, sim.literal_ranges)
    check(sim.search(patterns, 1000, teams=4, grid=2), exp, "synth_64k")
    check(sim.search(patterns, 1000, teams=3, grid=5), exp, "synth_64k, another shape")
    got = sim.search([], 16)
    assert got[0].tolist() == [0] and len(got[1]) == 0


# ---- the Python helpers -------------------------------------------------------------------------------------------------------
def test_ignore_case_and_parse_classes():
    assert ia.ignore_case("Straße") == ["Ss", "tT", "rR", "aA", "ß", "eE"]  # 'ß'.upper() is two code units: it stays alone
    assert ia.ignore_case("a1_") == ["aA", "1", "_"]
    assert ia.ignore_case("ı") == ["ıI"]  # dotless i: its upper case is one unit, so it is an alternative
    assert ia.parse_classes("blk_[0-9a-f]x\\[") == ["b", "l", "k", "_", "0123456789abcdef", "x", "["]
    assert ia.parse_classes("[a\\]b][-x][x-]") == ["a]b", "-x", "x-"]
    assert ia.parse_classes("[aab-ca]") == ["abc"]
    for bad in ("[^a]", "[ab", "[]", "x[", "[z-a]", "ab\\"):
        with pytest.raises(ValueError):
            ia.parse_classes(bad)
    alt, pos_off, pat_off = ia.pack_class_patterns([ia.ignore_case("ab"), [], ["", [ord("x"), "y"]]])
    assert alt.tolist() == [97, 65, 98, 66, 120, 121] and pos_off.tolist() == [0, 2, 4, 4, 6] and pat_off.tolist() == [0, 2, 2, 4]
    assert alt.dtype == np.uint16 and pos_off.dtype == np.int32 and pat_off.dtype == np.int32
    alt, pos_off, pat_off = ia.pack_class_patterns([])
    assert len(alt) == 0 and pos_off.tolist() == [0] and pat_off.tolist() == [0]


def test_status_and_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    names = ("fmx_count_class_batch", "fmx_locate_all_class_batch", "fmx_match_query_class_batch", "fmx_class_ranges_scratch_bytes",
             "fmx_class_ranges_count_dev", "fmx_class_ranges_fill_dev", "fmx_class_hit_offsets_scratch_bytes", "fmx_class_hit_offsets_dev",
             "fmx_class_fold_status_dev")
    for name in names:
        assert name in ia.SYMBOLS
    assert ia.lib.fmx_status_message(ST_TOO_MANY).decode() == "Class pattern keeps more than max_ranges ranges"
    assert ia.lib.fmx_status_kind(ST_TOO_MANY) == 0 and ia._lib.ST_TOO_MANY_RANGES == ST_TOO_MANY
    with pytest.raises(RuntimeError, match="max_ranges"):
        ia.raise_for_status(ST_TOO_MANY)
    fm = ia.FmIndex("This is a long string\0", 4, True, device=None)
    alt, pos_off, pat_off = ia.pack_class_patterns([ia.ignore_case("is"), ia.parse_classes("[a-z]ong")])
    n_pos, n = len(pos_off) - 1, len(pat_off) - 1
    counts, status, hit_off = np.full(n, SENT, np.int32), np.full(n, SENT, np.int32), np.full(n + 1, SENT, np.int64)
    buf = C.c_void_p(0x1234)

    def count(h=fm._h, alt_=alt, pos=pos_off, npos=n_pos, pat=pat_off, n_=n, cap=16, out=counts):
        return ia.lib.fmx_count_class_batch(h, ptr(alt_), ptr(pos), npos, ptr(pat), n_, cap, ptr(out), ptr(status))

    def locate(h=fm._h, pos=pos_off, pat=pat_off, n_=n, cap=16, off=hit_off, out=buf):
        return ia.lib.fmx_locate_all_class_batch(h, ptr(alt), ptr(pos), n_pos, ptr(pat), n_, cap, ptr(off), C.byref(out) if out is not None else None,
                                                 ptr(status))

    assert count() == E_NO_DEVICE and locate() == E_NO_DEVICE and buf.value is None
    assert (counts == SENT).all() and (status == SENT).all() and (hit_off == SENT).all()  # nothing written
    for bad in (dict(h=None), dict(n_=-1), dict(npos=-1), dict(pos=None), dict(pat=None), dict(cap=0), dict(cap=RANGES_MAX + 1), dict(cap=-5)):
        assert count(**bad) == E_ARG, bad
    assert count(cap=RANGES_MAX) == E_NO_DEVICE
    assert count(pos=np.array([-1, 2, 4, 14, 15, 16, 17], np.int32)) == E_ARG  # starts below 0
    assert count(pos=np.array([0, 2, 1, 14, 15, 16, 17], np.int32)) == E_ARG  # decreases
    assert count(pat=np.array([0, 3, 2], np.int32)) == E_ARG
    assert count(pat=np.array([0, 2, n_pos + 1], np.int32)) == E_ARG  # pat_off[n] above the number of positions
    assert count(alt_=None) == E_ARG
    for bad in (dict(h=None), dict(cap=0), dict(cap=1025), dict(off=None), dict(out=None), dict(pat=np.array([0, 3, 2], np.int32))):
        buf.value = 0x1234
        assert locate(**bad) == E_ARG, bad
        assert bad.get("out", buf) is None or buf.value is None  # *locs = NULL on every failure
    qoff, kinds = np.array([0, 2], np.int32), np.array([0, 2], np.uint8)
    line_off = np.full(2, SENT, np.int64)

    def query(h=fm._h, cap=16, qo=qoff, kd=kinds, q=1, lo=line_off):
        return ia.lib.fmx_match_query_class_batch(h, ptr(alt), ptr(pos_off), n_pos, ptr(pat_off), n, cap, ptr(qo), ptr(kd), q, 0, ptr(lo), C.byref(buf),
                                                  None, None, None)

    assert query() == E_NO_DEVICE and query(h=None) == E_ARG and query(cap=0) == E_ARG and query(q=-1) == E_ARG and query(lo=None) == E_ARG
    assert (line_off == SENT).all()
    p = alt.ctypes.data  # (any non-null pointer: the arguments are judged before anything is touched)
    nbytes = ia.lib.fmx_class_ranges_scratch_bytes(1000)
    assert nbytes >= 8 * 1001 and ia.lib.fmx_class_hit_offsets_scratch_bytes(1000) >= 8 * 1001
    cnt, fill, hits, fold = (ia.lib.fmx_class_ranges_count_dev, ia.lib.fmx_class_ranges_fill_dev, ia.lib.fmx_class_hit_offsets_dev,
                             ia.lib.fmx_class_fold_status_dev)
    assert cnt(fm._h, p, p, p, 2, 16, p, p, p, p, nbytes, None) == E_NO_DEVICE
    assert cnt(fm._h, p, p, p, 2, 0, p, p, p, p, nbytes, None) == E_ARG and cnt(fm._h, p, p, p, 2, 1025, p, p, p, p, nbytes, None) == E_ARG
    assert cnt(fm._h, p, p, p, -2, 16, p, p, p, p, nbytes, None) == E_ARG and cnt(fm._h, p, p, p, 2, 16, None, p, p, p, nbytes, None) == E_ARG
    assert fill(fm._h, p, p, p, 2, 16, p, p, None) == E_NO_DEVICE and fill(fm._h, p, p, p, 2, 16, p, None, None) == E_ARG
    assert fill(fm._h, p, p, p, 2, 2000, p, p, None) == E_ARG
    assert hits(fm._h, 2, p, p, 5, p, p, p, nbytes, None) == E_NO_DEVICE and hits(fm._h, 2, p, p, 2 ** 31, p, p, p, nbytes, None) == E_ARG
    assert hits(fm._h, 2, p, p, 5, None, p, p, nbytes, None) == E_ARG
    assert fold(fm._h, 2, p, 5, p, p, None) == E_NO_DEVICE and fold(fm._h, 2, p, -1, p, p, None) == E_ARG
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert count(h=h) == E_ARG and locate(h=h) == E_ARG and query(h=h) == E_ARG
        assert cnt(h, p, p, p, 2, 16, p, p, p, p, nbytes, None) == E_ARG and fill(h, p, p, p, 2, 16, p, p, None) == E_ARG
    with pytest.raises(ValueError):
        fm.locate_all("is", maxMatches=3, ignore_case=True)


def test_host_simulation_is_sanitizer_clean(tmp_path):
    """tests/cpp/san_class_search.cpp: the mirror as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer,
    every array exactly as large as the contract makes it"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "index4j_amd", "csrc")
    exe = str(tmp_path / "san_class_search")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + csrc, "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "san_class_search.cpp")]
    cmd += [os.path.join(csrc, f) for f in ("fmx_build.cpp", "fmx_serial.cpp", "fmx_blob.cpp", "fmx_synth.cpp")]
    cmd += ["-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.count(" ok: ") == 4

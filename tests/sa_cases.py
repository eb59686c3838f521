"""Shared by the SuffixArray tests: a line-by-line restatement of suffixarray/SuffixArray.java's searches (SA:56-157), the
banana known answers, the test shim of the device search routines, and the pattern sets the CPU and GPU suites draw."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# pattern -> (the reference's count, the true number of occurrences) on "banana", SA = [6, 5, 3, 1, 0, 4, 2]
BANANA = {"": (6, 7), "a": (3, 3), "an": (2, 2), "n": (1, 2), "na": (1, 2), "nana": (0, 1), "b": (1, 1), "z": (0, 0)}


def compare_to(s1, f1, t1, s2, f2, t2):  # SA:56-68
    lim = min(t1 - f1, t2 - f2)
    for k in range(lim):
        c1, c2 = int(s1[f1 + k]), int(s2[f2 + k])
        if c1 != c2:
            return c1 - c2
    return (t1 - f1) - (t2 - f2)


def starts_with(s1, f1, t1, s2, f2, t2):  # SA:70-87
    len1, len2 = t1 - f1, t2 - f2
    if len2 > len1:
        return False
    for k in range(min(len1, len2)):
        if s1[f1 + k] != s2[f2 + k]:
            return False
    return True


def ref_left_right(text, sa, p):
    """searchUpperInterval / searchLowerInterval (SA:131-157) over uint16 arrays"""
    n = len(text)
    lo, r = 0, len(sa) - 1
    while lo < r:
        mid = (lo + r) // 2
        if compare_to(p, 0, len(p), text, int(sa[mid]), n) > 0:
            lo = mid + 1
        else:
            r = mid
    left = lo
    up, r = left, len(sa) - 1
    while up < r:
        mid = (up + r) // 2
        if starts_with(text, int(sa[mid]), n, p, 0, len(p)):
            up = mid + 1
        else:
            r = mid
    return left, r


_SIM = {}


def sim_lib(tmpdir):
    """tests/sa_hostsim.cpp compiled for the host (g++), in `tmpdir`"""
    if "lib" not in _SIM:
        so = os.path.join(str(tmpdir), "libsahostsim.so")
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "sa_hostsim.cpp")])
        L = C.CDLL(so)
        L.sim_sa_search.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p]
        L.sim_sa_search.restype = C.c_int32
        _SIM["lib"] = L
    return _SIM["lib"]


def sim_search(L, text, sa, pats, most=4096, chars=8):
    """(left, right, fences) of every pattern through the device search routines compiled for the host"""
    t = np.ascontiguousarray(text, dtype=np.uint16)
    s = np.ascontiguousarray(sa, dtype=np.int32)
    off = np.zeros(len(pats) + 1, dtype=np.int32)
    np.cumsum([len(p) for p in pats], out=off[1:])
    chars_all = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint16) for p in pats] + [np.zeros(1, np.uint16)]))
    left = np.zeros(len(pats), dtype=np.int32)
    right = np.zeros(len(pats), dtype=np.int32)
    nf = L.sim_sa_search(t.ctypes.data, len(t), s.ctypes.data, most, chars, chars_all.ctypes.data, off.ctypes.data, len(pats),
                         left.ctypes.data, right.ctypes.data)
    return left, right, nf


def reference_draws(text16, count=1000, seed=42):
    """SuffixArrayTest.java:36-48: start = nextInt(len - 32), substring of nextInt(1, 32) chars, from java.util.Random(42)"""
    from common import JavaRandom

    rnd = JavaRandom(seed)
    out = []
    for _ in range(count):
        start = rnd.next_int(len(text16) - 32)
        out.append(np.asarray(text16[start:start + rnd.next_int(1, 32)], dtype=np.uint16))
    return out


def suffix_less(text, a, b):
    """suffix a < suffix b by compareTo (chunked, for long texts)"""
    n = len(text)
    k = 0
    while True:
        la, lb = n - a - k, n - b - k
        if la <= 0 or lb <= 0:
            return la < lb
        m = min(la, lb, 64)
        x, y = text[a + k:a + k + m], text[b + k:b + k + m]
        d = np.nonzero(x != y)[0]
        if len(d):
            return int(x[d[0]]) < int(y[d[0]])
        k += m


def assert_is_reference_array(text, sa):
    """[n] + the suffixes in compareTo order: a permutation of 0..n starting at n whose neighbours are strictly ordered"""
    n = len(text)
    sa = np.asarray(sa)
    assert len(sa) == n + 1 and sa[0] == n
    assert (np.sort(sa) == np.arange(n + 1)).all()
    for i in range(1, n):
        assert suffix_less(text, int(sa[i]), int(sa[i + 1])), i


# ---- the edge table: texts at the fence table's, the sort's and the locate scan's edges, one pattern set per text ----

NAIVE_MAX = 4200  # naive_suffix_array holds every suffix as a key: for texts up to here only


def naive_suffix_array(text):
    """[n] + sorted(range(n), key=lambda i: text[i:]) as int32: independent of SA-IS and of the device.  The keys are the
    suffixes' big-endian bytes, whose order is the order of the uint16 sequences (a proper prefix first, as compareTo)."""
    t = np.ascontiguousarray(text, dtype=np.uint16)
    n = len(t)
    assert n <= NAIVE_MAX
    b = t.astype(">u2").tobytes()
    return np.array([n] + sorted(range(n), key=lambda i: b[2 * i:]), dtype=np.int32)


def _fibonacci_word(n):
    a, b = "a", "ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _edge_texts():
    from common import hdfs_text

    u16 = lambda s: np.frombuffer(s.encode("utf-16-le"), dtype=np.uint16).copy()
    word = np.random.default_rng(17).integers(0, 3, 17) + ord("a")
    nul13 = [0, 5, 0, 0, 5, 5, 0, 1, 0, 0, 0, 5, 0]  # the text of test_text_with_nul_and_short_suffixes
    mix = np.array([0, 0, 1, 0xD800, 0xFFFF])[np.random.default_rng(257).integers(0, 5, 257)]
    texts = {
        "empty": u16(""),
        "x": u16("x"),
        "ba": u16("ba"),
        "a300": u16("a" * 300),
        "a4096": u16("a" * 4096),
        "ab2048": u16("ab" * 2048),
        "word17x20": np.tile(word, 20),
        "fibonacci4181": u16(_fibonacci_word(4181)),
        "nul40": np.zeros(40),
        "nulmix257": mix,
        "binary4097": np.random.default_rng(4097).integers(0, 2, 4097),  # one more than 4,096 fences: shift 1, a partial group
        "nul13": np.array(nul13),
        "hdfs20000": u16(hdfs_text())[:20000],
    }
    return {k: np.ascontiguousarray(v, dtype=np.uint16) for k, v in texts.items()}


EDGE_TEXTS = _edge_texts()
NUL_TEXTS = ("nul40", "nulmix257", "nul13")
EDGE_SEED = 20


def fence_rows(n, most, chars):
    """(n_fences, shift) as sa_fence_settings derives them, and whether the key table fits the 64 KiB that are staged"""
    s = 0
    while most > 0 and ((n + (1 << s) - 1) >> s) > most:
        s += 1
    nf = ((n + (1 << s) - 1) >> s) if most > 0 else 0
    return nf, s, nf * chars * 2 <= 64 * 1024


def edge_patterns(text, sa, rng):
    """the pattern set of one text (uint16 arrays): the fixed ones first (edge_fixed_patterns), then 300 substrings in four
    forms each, then the keys of about 64 fence rows of the default table cut at, below and above K = 8 and K = 16"""
    t = np.ascontiguousarray(text, dtype=np.uint16)
    n = len(t)
    pats = edge_fixed_patterns(t, sa)
    for _ in range(300 if n else 0):
        ln = int(rng.integers(1, min(39, n) + 1))
        s = int(rng.integers(0, n - ln + 1))
        cut = t[s:s + ln]
        up, down = cut.copy(), cut.copy()
        up[-1] = (int(cut[-1]) + 1) & 0xFFFF  # (0xFFFF + 1 = 0, 0 - 1 = 0xFFFF)
        down[-1] = (int(cut[-1]) - 1) & 0xFFFF
        pats += [cut, up, down, np.append(cut, np.uint16(0))]
    _, shift, _ = fence_rows(n, 4096, 8)
    step = -(-max(1, n // 64) >> shift) << shift  # a multiple of the fence distance: every row taken is a fence
    for j in range(0, n, step):
        pos = int(sa[j])
        pats += [t[pos:pos + ln] for ln in (1, 7, 8, 9, 15, 16, 17)]
    return pats


def edge_fixed_patterns(text, sa):
    """empty, [0], [0xFFFF], the whole text, the text plus its first char and plus '\\0' (longer than every suffix), and the
    largest suffix itself"""
    t = np.ascontiguousarray(text, dtype=np.uint16)
    n = len(t)
    z = np.zeros(1, np.uint16)
    return [t[:0], z, np.array([0xFFFF], np.uint16), t, np.concatenate([t, t[:1]]), np.concatenate([t, z]), t[int(sa[n]):]]


def occurrences16(text, p):
    """how often p occurs in text (the empty pattern: at every position and at the end), by comparing at every position"""
    n, m = len(text), len(p)
    if m > n:
        return 0
    hit = np.ones(n - m + 1, dtype=bool)
    for k in range(m):
        hit &= text[k:k + n - m + 1] == p[k]
    return int(hit.sum())


class EdgeCase:
    """one text of the table: its array (naive_suffix_array up to NAIVE_MAX chars, else the host's SA-IS checked by
    assert_is_reference_array), its patterns, their (left, right) by ref_left_right, and what the set was checked to hold"""

    def __init__(self, name):
        self.name = name
        self.text = EDGE_TEXTS[name]
        n = len(self.text)
        if n <= NAIVE_MAX:
            self.sa = naive_suffix_array(self.text)
        else:
            import index4j_amd as ia

            self.sa = ia.SuffixArray(self.text, device=None, build_device=-1).construct().getSuffixArray()
            assert_is_reference_array(self.text, self.sa)
        self.pats = edge_patterns(self.text, self.sa, np.random.default_rng(EDGE_SEED))
        tl, sl = self.text.tolist(), self.sa.tolist()
        lr = np.array([ref_left_right(tl, sl, p.tolist()) for p in self.pats], dtype=np.int32).reshape(-1, 2)
        self.left, self.right = lr[:, 0].copy(), lr[:, 1].copy()
        self.counts = self.right - self.left
        self.pat, self.off = pack(self.pats)
        self.stats = self._non_vacuity()

    def _non_vacuity(self):
        """from the reference alone: patterns with and without hits, quirk hits, and (NUL texts) short fences / real NULs"""
        t, sa, n = self.text, self.sa, len(self.text)
        top = int(sa[n])
        quirk = 0
        for p, c in zip(self.pats, self.counts):
            if len(p) <= n - top and (t[top:top + len(p)] == p).all():  # the largest suffix starts with p
                assert int(c) == occurrences16(t, p) - 1, self.name
                quirk += 1
        nf, shift, _ = fence_rows(n, 4096, 8)
        short = real_nul = 0
        for j in range(nf):
            pos = int(sa[j << shift])
            flen = min(8, n - pos)
            short += flen < 8
            real_nul += bool((t[pos:pos + flen] == 0).any())
        stats = {"patterns": len(self.pats), "hits": int((self.counts > 0).sum()), "misses": int((self.counts == 0).sum()),
                 "quirk": quirk, "short_fences": int(short), "nul_fences": int(real_nul)}
        if n >= 40:
            assert stats["hits"] >= 50 and stats["misses"] >= 50 and quirk >= 1, (self.name, stats)
        if self.name in NUL_TEXTS:
            assert short >= 1 and real_nul >= 1, (self.name, stats)
        return stats


def pack(pats):
    """(chars, offsets) of a list of uint16 patterns, in the layout the batch calls take"""
    off = np.zeros(len(pats) + 1, dtype=np.int32)
    np.cumsum([len(p) for p in pats], out=off[1:])
    chars = np.concatenate([np.asarray(p, dtype=np.uint16) for p in pats] + [np.zeros(0, np.uint16)])
    return np.ascontiguousarray(chars, dtype=np.uint16), off


_CASES = {}


def edge_case(name):
    """the EdgeCase of a text, computed once per process and never changed"""
    if name not in _CASES:
        _CASES[name] = EdgeCase(name)
    return _CASES[name]

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

"""index4j's SuffixArray and BurrowsWheelerTransform on the host side (CPU only): arrays built by host SA-IS
(build_device=-1), the device search routines through a test-only host build (tests/sa_hostsim.cpp) against a line-by-line
restatement of SA:100-157, the stream form, hashCode, damaged streams (also under AddressSanitizer), and the BWT's
known answers."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
from common import GOLDEN, hdfs_text
from sa_cases import (BANANA, EDGE_TEXTS, NAIVE_MAX, ROOT, assert_is_reference_array, edge_case, fence_rows,
                      naive_suffix_array, ref_left_right, reference_draws, sim_lib, sim_search)


def host_sa(text):
    return ia.SuffixArray(text, device=None, build_device=-1).construct()


def java_hash(text16, sa):
    h = 0
    for c in text16:
        h = (31 * h + int(c)) & 0xFFFFFFFF
    a = 1
    for v in sa:
        a = (31 * a + int(v)) & 0xFFFFFFFF
    s = (h + a) & 0xFFFFFFFF
    return s - (1 << 32) if s >= (1 << 31) else s


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return sim_lib(tmp_path_factory.mktemp("sahostsim"))


def test_banana_array():
    assert host_sa("banana").getSuffixArray().tolist() == [6, 5, 3, 1, 0, 4, 2]
    assert host_sa("").getSuffixArray().tolist() == [0]


def test_hdfs_array_is_the_reference_array():
    t = ia.as_chars(hdfs_text())
    assert_is_reference_array(t, host_sa(t).getSuffixArray())


@pytest.mark.parametrize("sigma", [2, 3, 70, 1099])
def test_random_texts(sigma):
    """64 K chars over `sigma` symbols, with '\\0' and chars >= 0xD800 among them"""
    rng = np.random.default_rng(sigma)
    symbols = np.unique(np.concatenate([[0, 0xD800, 0xFFFF], rng.integers(1, 65536, sigma)]))[:sigma].astype(np.uint16)
    t = symbols[rng.integers(0, len(symbols), 1 << 16)]
    assert_is_reference_array(t, host_sa(t).getSuffixArray())


def test_banana_known_answers_through_the_device_routines(sim):
    t = ia.as_chars("banana")
    sa = host_sa(t).getSuffixArray()
    pats = [ia.as_chars(p) for p in BANANA]
    for most in (0, 1, 2, 4096):
        left, right, _ = sim_search(sim, t, sa, pats, most=most)
        for i, p in enumerate(BANANA):
            assert ref_left_right(t, sa, pats[i]) == (left[i], right[i]), p
            assert right[i] - left[i] == BANANA[p][0], p


def test_reference_draws_on_hdfs(sim):
    """1,000 substrings drawn as SuffixArrayTest.java:36-48 draws them; how many hit the largest-suffix case is reported"""
    t = ia.as_chars(hdfs_text())
    sa = host_sa(t).getSuffixArray()
    pats = reference_draws(t)
    n = len(t)
    exp = [ref_left_right(t, sa, p) for p in pats]
    for most, chars in ((4096, 8), (0, 8), (64, 3), (1 << 15, 1)):
        left, right, nf = sim_search(sim, t, sa, pats, most=most, chars=chars)
        assert [(int(a), int(b)) for a, b in zip(left, right)] == exp, (most, chars)
    # the largest suffix (row n) starts with p: the reference counts one fewer than the occurrences
    largest = sa[n]
    hits = sum(1 for p in pats if len(p) <= n - largest and (t[largest:largest + len(p)] == p).all())
    print("reference draws that hit the largest-suffix case: %d of %d" % (hits, len(pats)))


def test_edge_patterns(sim):
    """absent patterns, patterns longer than K, patterns equal to a fence key, the empty pattern"""
    t = ia.as_chars(hdfs_text())[:20000]
    sa = host_sa(t).getSuffixArray()
    n = len(t)
    rng = np.random.default_rng(5)
    pats = [np.zeros(0, np.uint16), ia.as_chars("zzzzqqq"), ia.as_chars("￿"), np.array([0], np.uint16)]
    for _ in range(200):
        s = int(rng.integers(0, n - 40))
        pats.append(t[s:s + int(rng.integers(9, 40))])  # longer than K
        q = t[s:s + 12].copy()
        q[-1] = 0xFFFF
        pats.append(q)  # absent past K
    for j in range(0, n, max(1, n // 4096)):  # the fence keys themselves (and one char shorter / longer)
        pos = int(sa[j])
        for ln in (7, 8, 9):
            if j % 7 == 0:
                pats.append(t[pos:pos + ln])
    pats.append(t[int(sa[n]):])  # the largest suffix itself
    exp = [ref_left_right(t, sa, p) for p in pats]
    for most, chars in ((4096, 8), (8192, 4), (0, 8)):
        left, right, _ = sim_search(sim, t, sa, pats, most=most, chars=chars)
        assert [(int(a), int(b)) for a, b in zip(left, right)] == exp, (most, chars)


def test_text_with_nul_and_short_suffixes(sim):
    """'\\0' chars in the text and suffixes shorter than K among the fences"""
    t = np.array([0, 5, 0, 0, 5, 5, 0, 1, 0, 0, 0, 5, 0], np.uint16)
    sa = host_sa(t).getSuffixArray()
    pats = [t[i:j] for i in range(len(t)) for j in range(i, len(t) + 1)] + [np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint16)]
    exp = [ref_left_right(t, sa, p) for p in pats]
    for most in (1, 2, 4, 16):
        for chars in (1, 2, 3, 8):
            left, right, _ = sim_search(sim, t, sa, pats, most=most, chars=chars)
            assert [(int(a), int(b)) for a, b in zip(left, right)] == exp, (most, chars)


def test_edge_table(sim):
    """every text of sa_cases.EDGE_TEXTS with its whole pattern set through the device search routines, at fence tables from
    none to one fence per row and keys of 1 to 16 chars (odd ones too), against ref_left_right; and host SA-IS against the
    naive sort.  What each set was checked to hold (from the reference alone) is printed."""
    for name in EDGE_TEXTS:
        c = edge_case(name)
        print(name, c.stats)
        if len(c.text) <= NAIVE_MAX:
            assert host_sa(c.text).getSuffixArray().tolist() == naive_suffix_array(c.text).tolist(), name
        for most in (0, 1, 2, 16, 64, 4096, 32768):
            for chars in (1, 2, 3, 8, 15, 16):
                left, right, nf = sim_search(sim, c.text, c.sa, c.pats, most=most, chars=chars)
                assert nf == fence_rows(len(c.text), most, chars)[0], (name, most, chars)
                bad = np.nonzero((left != c.left) | (right != c.right))[0]
                assert len(bad) == 0, (name, most, chars, c.pats[bad[0]].tolist(), int(left[bad[0]]), int(right[bad[0]]),
                                       int(c.left[bad[0]]), int(c.right[bad[0]]))


def test_stream_bytes_of_banana():
    s = host_sa("banana")
    raw = b"\x00" + struct.pack(">i", 6) + b"banana" + struct.pack(">i", 7) + struct.pack(">7i", 6, 5, 3, 1, 0, 4, 2)
    assert s.write(framed=False) == raw
    assert s.write(framed=True) == b"\xac\xed\x00\x05" + b"\x77" + bytes([len(raw)]) + raw


def test_round_trips_and_hash_code():
    for text, back in (("banana", "banana"), ("a\U0001F600b", "a\U0001F600b"), ("x\ud800y", "x?y"), ("", "")):
        t = ia.as_chars(text) if "\ud800" not in text else np.array([ord("x"), 0xD800, ord("y")], np.uint16)
        s = host_sa(t)
        assert s.hashCode() == java_hash(t, s.getSuffixArray())
        for framed in (False, True):
            r = ia.SuffixArray.read(s.write(framed=framed), device=None)
            b = ia.as_chars(back)
            assert r.getSuffixArray().tolist() == s.getSuffixArray().tolist()
            assert r.hashCode() == java_hash(b, s.getSuffixArray())
            assert len(r) == len(b)


def _load(b):
    h = C.c_void_p()
    rc = ia.lib.fmx_sa_load(b, len(b), C.byref(h))
    if rc == 0:
        ia.lib.fmx_free(h)
    return rc


def test_damaged_streams_are_refused():
    raw = host_sa("banana").write(framed=False)
    for cut in range(len(raw)):
        assert _load(raw[:cut]) == ia._lib.E_FORMAT, cut
    framed = host_sa("banana").write(framed=True)
    for cut in range(len(framed)):  # (a cut inside the magic reads as a raw stream of another version)
        assert _load(framed[:cut]) in ((ia._lib.E_FORMAT, ia._lib.E_VERSION) if 0 < cut < 4 else (ia._lib.E_FORMAT,)), cut
    bad_len = raw[:11] + struct.pack(">i", 6) + raw[15:]
    assert _load(bad_len) == ia._lib.E_FORMAT
    bad_entry = raw[:-4] + struct.pack(">i", 7)
    assert _load(bad_entry) == ia._lib.E_FORMAT
    assert _load(raw[:-4] + struct.pack(">i", -1)) == ia._lib.E_FORMAT
    assert _load(b"\x00" + struct.pack(">i", 2) + b"\xc3\x28" + struct.pack(">i", 3) + struct.pack(">3i", 2, 1, 0)) == ia._lib.E_FORMAT
    assert _load(b"\x00" + struct.pack(">i", 3) + b"\xed\xa0\x80" + struct.pack(">i", 2) + struct.pack(">2i", 1, 0)) == ia._lib.E_FORMAT
    assert _load(b"\x00" + struct.pack(">i", -2)) == ia._lib.E_FORMAT
    assert _load(b"\x01" + raw[1:]) == ia._lib.E_VERSION
    assert _load(raw + b"trailing") == 0


def test_accepted_mutations_search_clean_under_asan(tmp_path):
    exe = str(tmp_path / "sa_fuzz")
    csrc = os.path.join(ROOT, "index4j_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-DSA_FUZZ_MAIN", "-I" + csrc,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sa_hostsim.cpp")]
    cmd += [os.path.join(csrc, f) for f in ("fmx_sa_serial.cpp", "fmx_serial.cpp", "fmx_build.cpp", "fmx_blob.cpp", "fmx_synth.cpp")]
    subprocess.check_call(cmd + ["-lpthread", "-o", exe])
    r = subprocess.run([exe, "12000", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr, r.stdout[-2000:] + r.stderr[-6000:]
    assert r.stdout.startswith("sa fuzz ok:"), r.stdout
    assert int(r.stdout.split()[3]) >= 2000, r.stdout  # accepted streams that were searched


def test_queries_need_construct_and_a_device():
    s = ia.SuffixArray("banana", device=None, build_device=-1)
    with pytest.raises(RuntimeError):
        s.count("a")
    s.construct()
    with pytest.raises(ia.FmxError) as e:
        s.count("a")
    assert e.value.code == ia._lib.E_NO_DEVICE
    assert ia.lib.fmx_device_of(s._h) == -1 and ia.lib.fmx_input_length(s._h) == 6


def test_fm_entry_points_refuse_a_suffix_array_handle():
    s = host_sa("banana")
    h = s._h
    pat, off = ia.pack_patterns(["an"])
    counts = np.zeros(1, np.int32)
    E = ia._lib.E_ARG
    assert ia.lib.fmx_count_batch(h, pat.ctypes.data, off.ctypes.data, 1, counts.ctypes.data, None, None) == E
    locs = np.zeros(4, np.int32)
    found = np.zeros(1, np.int32)
    assert ia.lib.fmx_locate_batch(h, pat.ctypes.data, off.ctypes.data, 1, 4, locs.ctypes.data, 4, found.ctypes.data, None, None) == E
    buf, ln = C.c_void_p(), C.c_size_t()
    assert ia.lib.fmx_save(h, 0, C.byref(buf), C.byref(ln)) == E
    assert ia.lib.fmx_blob(h, C.byref(buf), C.byref(ln)) == E
    assert ia.lib.fmx_suffix_table_info(h, None, None) == E
    assert ia.lib.fmx_rrr_rank_ones_batch(h, locs.ctypes.data, 1, locs.ctypes.data) == E
    out = np.zeros(1, np.int64)
    assert ia.lib.fmx_wavelet_inverse_select_batch(h, out.ctypes.data, 1, out.ctypes.data, None) == E
    # and the SuffixArray calls refuse an FM-index handle
    f = ia.FmIndex("banana", 4, True, device=None)
    v = C.c_int32()
    assert ia.lib.fmx_sa_hash_code(f._h, C.byref(v)) == E


def test_bwt_known_answers():
    cases = json.load(open(os.path.join(GOLDEN, "bwt_kats.json")))["cases"]
    assert len(cases) == 4
    for c in cases:
        bwt = ia.createBurrowsWheelerTransform(c["text"], build_device=-1)
        assert bwt == c["bwt"], c["name"]
        assert ia.computeRedundancyOfText(bwt) > ia.computeRedundancyOfText(c["text"]), c["name"]


def test_bwt_charset_limit():
    ok = np.arange(1, 32767, dtype=np.uint16)  # 32,766 chars + '\0' = 32,767 symbols
    assert len(ia.createBurrowsWheelerTransform(ok, build_device=-1)) == len(ok) + 1
    over = np.arange(1, 32768, dtype=np.uint16)  # + '\0' = 32,768
    with pytest.raises(ValueError, match="Charset has more than 32767 different characters."):
        ia.createBurrowsWheelerTransform(over, build_device=-1)


def test_redundancy_is_n_over_runs():
    assert ia.computeRedundancyOfText("aaabbc") == 6 / 3
    assert ia.computeRedundancyOfText(np.array([1, 1, 2, 2, 2, 1, 3], np.int16)) == 7 / 4
    assert ia.computeRedundancyOfText("ANNB\0AA") == 7 / 5
    with pytest.raises(IndexError):
        ia.computeRedundancyOfText("")


def test_cpp_mirror(tmp_path):
    """include/index4j/SuffixArray.hpp: construct on the host, getSuffixArray, write / read, hashCode, the BWT"""
    exe = str(tmp_path / "test_sa_mirror")
    lib_dir = os.path.dirname(ia.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sa_mirror.cpp"), "-L" + lib_dir, "-lfmx",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["7", "6", str(java_hash(ia.as_chars("banana"), [6, 5, 3, 1, 0, 4, 2]))] * 1 + \
        [str(java_hash(ia.as_chars("banana"), [6, 5, 3, 1, 0, 4, 2])), "7", "1.400"]

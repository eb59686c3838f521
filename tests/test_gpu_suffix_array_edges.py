"""index4j's SuffixArray and BurrowsWheelerTransform on the GPU at their edges: the texts and pattern sets of
sa_cases.EDGE_TEXTS (one or two chars, runs of one char, periodic and Fibonacci words, '\\0' in the text, suffixes shorter
than a fence key, a text one char longer than the fence count) at every shape of the fence table, locate over scans of
`found` with zeros in every place, arrays sorted on the device at the alphabet sizes where the 16-bit codes turn over, the
BWT gather, and the launch shapes.  Every expected value comes from outside the device code: sa_cases.naive_suffix_array
(or host SA-IS checked by assert_is_reference_array) and the restatement ref_left_right.  All comparisons are exact."""
import json
import os

import numpy as np
import pytest

import index4j_amd as ia
from common import GOLDEN
from sa_cases import (EDGE_TEXTS, NAIVE_MAX, assert_is_reference_array, edge_case, edge_fixed_patterns, fence_rows,
                      naive_suffix_array, pack, ref_left_right)

pytestmark = pytest.mark.gpu

E_ARG = ia._lib.E_ARG
FILL = -7

# (sa_fences, sa_fence_chars): no table, one and two fences, odd key lengths, tables of exactly 64 KiB ((4096, 8), (8192, 4),
# (2048, 16), (32768, 1)); the last two rows fit the 64 KiB that are staged only for the shorter texts
FENCE_SETTINGS = [(0, 8), (1, 8), (2, 3), (16, 5), (64, 7), (4096, 8), (4096, 3), (8192, 4), (2048, 16), (32768, 1), (4096, 15),
                  (4096, 16)]


def _torch():
    import torch

    return torch


def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _set(name, value):
    assert ia.lib.fmx_set_option(name.encode(), value) == 0, (name, value)


def _restore(*names):
    defaults = {"sa_fences": 4096, "sa_fence_chars": 8, "block": 512, "groups_per_cu": 16}
    for name in names:
        ia.lib.fmx_set_option(name.encode(), ia._lib.ENV_OPTIONS.get(name, defaults[name]))


def _host_sa(text):
    return ia.SuffixArray(text, device=None, build_device=-1).construct().getSuffixArray()


def _assert_counts(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))


# ---- a. search at every fence shape, against the restatement ----

@pytest.mark.parametrize("name", list(EDGE_TEXTS))
def test_search_at_every_fence_shape(name):
    """one construct() per text; every setting then rebuilds the fence table alone (fmx_to_device -> sa_to_device).  A table
    above 64 KiB is refused with E_ARG, the handle goes on answering from the table it had, and fmx_to_device succeeds again
    once the options are back."""
    c = edge_case(name)
    n = len(c.text)
    s = ia.SuffixArray(c.text, device=0).construct()
    refused = 0
    try:
        for most, chars in FENCE_SETTINGS:
            _set("sa_fences", most)
            _set("sa_fence_chars", chars)
            rc = ia.lib.fmx_to_device(s._h, 0)
            if fence_rows(n, most, chars)[2]:
                assert rc == 0, (name, most, chars, rc)
            else:
                assert rc == E_ARG, (name, most, chars, rc)
                refused += 1
            _assert_counts(s.count_batch(c.pat, c.off), c.counts, (name, most, chars))
    finally:
        _restore("sa_fences", "sa_fence_chars")
    assert ia.lib.fmx_to_device(s._h, 0) == 0
    _assert_counts(s.count_batch(c.pat, c.off), c.counts, (name, "restored"))
    if name == "hdfs20000":
        assert refused == 2  # (4096, 15) and (4096, 16): 2,500 fences of 30 and 32 bytes


# ---- b. locate, host and device-pointer forms ----

def _check_locate(c, idx, m, locs, found, counts, what):
    """found = min(count, m); the first `found` rows of the pattern's range, in order; the fill value after them"""
    idx = np.asarray(idx)
    exp = c.counts[idx]
    if counts is not None:
        _assert_counts(counts, exp, (what, "counts"))
    _assert_counts(found, np.minimum(exp, m), (what, "found"))
    if m == 0:
        return
    k = np.arange(m)[None, :]
    rows = np.minimum(c.left[idx][:, None] + k, len(c.sa) - 1)
    want = np.where(k < found[:, None], c.sa[rows], FILL)
    bad = np.nonzero((locs != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), locs[bad[0]][:8].tolist(), want[bad[0]][:8].tolist())


def _locate_host(s, c, idx, m, what):
    pat, off = pack([c.pats[i] for i in idx])
    locs, found, counts = s.locate_batch(pat, off, max_matches=m, fill=FILL)
    assert locs.shape == (len(idx), m)
    _check_locate(c, idx, m, locs, found, counts, (what, "host", m))


def _locate_dev(s, c, idx, m, what, with_counts=True, with_locs=True):
    torch = _torch()
    pat, off = pack([c.pats[i] for i in idx])
    n = len(idx)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_pat = torch.from_numpy(pat.view(np.int16)).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_locs = torch.full((n, m), FILL, dtype=torch.int32, device="cuda") if with_locs else None
        d_found = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        d_counts = torch.full((n,), -9, dtype=torch.int32, device="cuda") if with_counts else None
        s.locate_batch_dev(d_pat, d_off, n, m, d_locs, d_found, d_counts, stream=st)
    st.synchronize()
    locs = d_locs.cpu().numpy() if with_locs else None
    _check_locate(c, idx, m, locs, d_found.cpu().numpy(), d_counts.cpu().numpy() if with_counts else None, (what, "dev", m))


def _locate_batches(c):
    """index lists into c.pats whose scans of `found` have zeros in every place"""
    hit = np.nonzero(c.counts > 0)[0]
    miss = np.nonzero(c.counts == 0)[0]
    assert len(hit) > 56 and len(miss) >= 50
    runs = []
    for j, gap in enumerate((0, 1, 5, 17, 2, 40, 1, 0, 3)):
        runs += [hit[7 * j]] + miss[j:j + gap].tolist()
    many = hit[c.counts[hit] > 3]
    assert len(many) >= 1  # (so that found = m cuts a range short)
    return {
        "one hit": [many[0]],
        "one absent": [miss[0]],
        "all absent": miss[:200].tolist(),
        "only the first hits": [hit[0]] + miss[:50].tolist(),
        "only the last hits": miss[:50].tolist() + [hit[-1]],
        "absent runs between hits": runs + miss[:9].tolist(),
        "the whole set": list(range(len(c.pats))),
    }


@pytest.mark.parametrize("name", ["a300", "nulmix257", "hdfs20000"])
def test_locate_scans_with_zeros(name):
    """max_matches 0 (nothing is copied), 1, 3, and 5,000, which is above every count of the two short texts"""
    c = edge_case(name)
    s = ia.SuffixArray(c.text, device=0).construct()
    first = True
    for what, idx in _locate_batches(c).items():
        for m in (0, 1, 3, 5000):
            _locate_host(s, c, idx, m, (name, what))
            _locate_dev(s, c, idx, m, (name, what), with_counts=not first)
            first = False
        _locate_dev(s, c, idx, 0, (name, what), with_locs=False)
    # 1,025 patterns: one more than a workgroup of 1,024 lanes has, at both workgroup sizes
    idx = list(range(1025))
    try:
        for block in (512, 1024):
            _set("block", block)
            _locate_host(s, c, idx, 3, (name, "1025 patterns", block))
            _locate_dev(s, c, idx, 3, (name, "1025 patterns", block))
    finally:
        _restore("block")


def test_locate_refusals_touch_nothing():
    """n * max_matches >= 2^31 and max_matches < 0: E_ARG, and the caller's arrays are as they were"""
    torch = _torch()
    c = edge_case("a300")
    s = ia.SuffixArray(c.text, device=0).construct()
    pat, off = pack([c.pats[1], c.pats[3]])
    d_pat = torch.from_numpy(pat.view(np.int16)).cuda()
    d_off = torch.from_numpy(off).cuda()
    for n, m in ((2, 1 << 30), (2, (1 << 31) - 1), (2, -1), (2, -(1 << 31))):
        locs = np.full(8, 11, np.int32)
        found = np.full(2, 12, np.int32)
        counts = np.full(2, 13, np.int32)
        before = [a.tobytes() for a in (locs, found, counts)]
        rc = ia.lib.fmx_sa_locate_batch(s._h, pat.ctypes.data, off.ctypes.data, n, m, locs.ctypes.data, found.ctypes.data,
                                        counts.ctypes.data)
        assert rc == E_ARG, (n, m, rc)
        assert [a.tobytes() for a in (locs, found, counts)] == before, (n, m)
        d = [torch.full((8,), 11, dtype=torch.int32, device="cuda"), torch.full((2,), 12, dtype=torch.int32, device="cuda"),
             torch.full((2,), 13, dtype=torch.int32, device="cuda")]
        rc = ia.lib.fmx_sa_locate_batch_dev(s._h, d_pat.data_ptr(), d_off.data_ptr(), n, m, d[0].data_ptr(), d[1].data_ptr(),
                                            d[2].data_ptr(), None)
        assert rc == E_ARG, (n, m, rc)
        torch.cuda.synchronize()
        assert [t.cpu().numpy().tobytes() for t in d] == before, (n, m)
    # the handle still answers
    _assert_counts(s.count_batch(c.pat, c.off), c.counts, "after the refusals")


# ---- c. arrays built on the device, against an independent sort ----

@pytest.mark.parametrize("name", [k for k, t in EDGE_TEXTS.items() if len(t) <= NAIVE_MAX])
def test_device_array_equals_naive_sort(name):
    text = EDGE_TEXTS[name]
    got = ia.SuffixArray(text, device=0).construct().getSuffixArray()
    assert got.tolist() == naive_suffix_array(text).tolist()


def _alphabet_text(distinct, length, seed):
    """`length` chars with exactly `distinct` different values, '\\0', 0xD800, 0xDFFF and 0xFFFF among them"""
    rng = np.random.default_rng(seed)
    must = np.array([0, 0xD800, 0xDFFF, 0xFFFF])
    rest = np.setdiff1d(np.arange(65536), must)
    symbols = np.concatenate([must, rng.permutation(rest)[:distinct - len(must)]])
    t = np.concatenate([symbols, symbols[rng.integers(0, distinct, length - distinct)]])
    t = rng.permutation(t).astype(np.uint16)
    assert len(np.unique(t)) == distinct and len(t) == length
    return t


@pytest.mark.parametrize("distinct", [40000, 32767, 32768, 65535, 65536])
def test_device_sort_where_the_codes_turn_over(distinct):
    """sa_sort's rule: with build_device >= 0 the device sorts when the alphabet — the distinct chars and the terminator —
    is at most 65,536, i.e. up to 65,535 distinct chars; 65,536 distinct chars are sorted by host SA-IS.  (The ABI does not
    tell which of the two sorted.)  The codes are 1 + rank: 32,767 distinct chars fill 15 bits, 32,768 are the first to
    need 16, and from there on the codes pass through int16_t as negative values.  The array a device build leaves
    resident is the one the queries read, so a wrong device array fails the counts even if the host copy were right."""
    text = _alphabet_text(distinct, 75000, seed=distinct)
    s = ia.SuffixArray(text, device=0).construct()
    sa = s.getSuffixArray()
    assert (sa == _host_sa(text)).all()
    assert_is_reference_array(text, sa)
    rng = np.random.default_rng(distinct + 1)
    pats = edge_fixed_patterns(text, sa)
    for _ in range(2000):
        ln = int(rng.integers(1, 6))
        start = int(rng.integers(0, len(text) - ln + 1))
        pats.append(text[start:start + ln])
    tl, sl = text.tolist(), sa.tolist()
    exp = np.array([r - l for l, r in (ref_left_right(tl, sl, p.tolist()) for p in pats)], dtype=np.int32)
    assert (exp > 0).sum() >= 1000
    _assert_counts(s.count_batch(*pack(pats)), exp, distinct)


# ---- d. the BWT gather ----

def _bwt_of(text, sa1):
    """BWT:100-108 as k_bwt_gather and fmx_bwt's host loop state it: text1 = text + '\\0', sa1 its array of len(text1) + 1
    rows; row 0 (the empty suffix) is dropped, and row i + 1 gives the char before its suffix, '\\0' before suffix 0"""
    text1 = np.append(np.ascontiguousarray(text, dtype=np.uint16), np.uint16(0))
    p = sa1[1:].astype(np.int64)
    return np.where(p == 0, 0, text1[np.maximum(p - 1, 0)]).astype(np.uint16)


def _sa_of_text1(text):
    text1 = np.append(np.ascontiguousarray(text, dtype=np.uint16), np.uint16(0))
    if len(text1) <= NAIVE_MAX:
        return naive_suffix_array(text1)
    sa1 = _host_sa(text1)
    assert_is_reference_array(text1, sa1)
    return sa1


def test_bwt_convention_on_the_known_answers():
    """the numpy statement of the transform gives the reference's four known answers (so it is the convention), and so
    does the device"""
    cases = json.load(open(os.path.join(GOLDEN, "bwt_kats.json")))["cases"]
    assert len(cases) == 4
    for case in cases:
        t = ia.as_chars(case["text"])
        assert ia.chars_to_str(_bwt_of(t, _sa_of_text1(t))) == case["bwt"], case["name"]
        assert ia.createBurrowsWheelerTransform(case["text"], build_device=0) == case["bwt"], case["name"]


@pytest.mark.parametrize("name", list(EDGE_TEXTS))
def test_bwt_gather(name):
    text = EDGE_TEXTS[name]
    assert len(np.unique(text)) <= 32766  # (with the '\0' appended: at most 32,767 symbols)
    exp = _bwt_of(text, _sa_of_text1(text))
    got = ia.createBurrowsWheelerTransform(text, build_device=0)
    assert got.dtype == np.uint16 and len(got) == len(text) + 1
    assert (got == exp).all(), int(np.nonzero(got != exp)[0][0])
    assert (ia.createBurrowsWheelerTransform(text, build_device=-1) == exp).all()


# ---- e. launch shapes on an edge text ----

@pytest.mark.parametrize("block,gpc", [(1024, 1), (512, 16)])
def test_launch_shapes_on_the_binary_text(block, gpc):
    """the 4,097-char text's set tiled past 3 * n_cu * 1024 patterns: at one workgroup per CU the grid loops at least three
    times over a staged table with a partial last fence group; then locate with max_matches = 2 over the same batch"""
    c = edge_case("binary4097")
    tiles = 3 * n_cu() * 1024 // len(c.pats) + 1
    pat = np.tile(c.pat, tiles)
    lens = np.tile(np.diff(c.off), tiles)
    off = np.zeros(len(lens) + 1, dtype=np.int32)
    assert int(lens.sum()) < (1 << 31)
    np.cumsum(lens, out=off[1:])
    idx = np.tile(np.arange(len(c.pats)), tiles)
    assert len(idx) > 3 * n_cu() * 1024
    try:
        _set("block", block)
        _set("groups_per_cu", gpc)
        s = ia.SuffixArray(c.text, device=0).construct()
        assert (s.getSuffixArray() == c.sa).all()
        _assert_counts(s.count_batch(pat, off), c.counts[idx], (block, gpc))
        locs, found, counts = s.locate_batch(pat, off, max_matches=2, fill=FILL)
        _check_locate(c, idx, 2, locs, found, counts, (block, gpc, "locate"))
    finally:
        _restore("block", "groups_per_cu")

"""index4j's SuffixArray and BurrowsWheelerTransform on the GPU: the known answers through every query form, the device-built
array against the host-built one, the full-size 256 MiB log against FmIndex, and every new kernel at 512 / 1024 lanes and
1 / 16 workgroups per CU on batches that loop the grid at least three times."""
import json
import os

import numpy as np
import pytest

import index4j_amd as ia
from common import GOLDEN
from sa_cases import BANANA, ref_left_right, sim_lib, sim_search

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def test_banana_known_answers_every_form():
    torch = _torch()
    s = ia.SuffixArray("banana", device=0).construct()
    assert s.getSuffixArray().tolist() == [6, 5, 3, 1, 0, 4, 2]
    pats = list(BANANA)
    counts = s.count_batch(pats)
    assert counts.tolist() == [BANANA[p][0] for p in pats]
    assert [s.count(p) for p in pats] == [BANANA[p][0] for p in pats]
    locs, found, c2 = s.locate_batch(pats, max_matches=2, fill=-7)
    assert (c2 == counts).all() and found.tolist() == [min(c, 2) for c in counts]
    sa = s.getSuffixArray()
    t = ia.as_chars("banana")
    for i, p in enumerate(pats):
        left, _ = ref_left_right(t, sa, ia.as_chars(p))
        assert locs[i, :found[i]].tolist() == sa[left:left + found[i]].tolist(), p
        assert (locs[i, found[i]:] == -7).all(), p
    offs = [9, 9, 9]
    assert s.locate("a", offs) == 3 and sorted(offs) == [1, 3, 5]
    offs = [9]
    assert s.locate("a", offs) == 1
    assert s.locate("a", []) == 0
    # the device-pointer forms on a torch stream
    pat, off = ia.pack_patterns(pats)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_pat = torch.from_numpy(pat.view(np.int16)).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_counts = torch.full((len(pats),), -1, dtype=torch.int32, device="cuda")
        d_locs = torch.full((len(pats), 2), -7, dtype=torch.int32, device="cuda")
        d_found = torch.zeros(len(pats), dtype=torch.int32, device="cuda")
        d_c2 = torch.zeros(len(pats), dtype=torch.int32, device="cuda")
        s.count_batch_dev(d_pat, d_off, len(pats), d_counts, stream=st)
        s.locate_batch_dev(d_pat, d_off, len(pats), 2, d_locs, d_found, d_c2, stream=st)
    st.synchronize()
    assert d_counts.cpu().numpy().tolist() == counts.tolist()
    assert d_found.cpu().numpy().tolist() == found.tolist() and d_c2.cpu().numpy().tolist() == counts.tolist()
    assert (d_locs.cpu().numpy() == locs).all()
    # empty text: every count 0
    e = ia.SuffixArray("", device=0).construct()
    assert e.getSuffixArray().tolist() == [0] and e.count_batch(["", "a"]).tolist() == [0, 0]


def test_bwt_known_answers_on_the_device():
    for c in json.load(open(os.path.join(GOLDEN, "bwt_kats.json")))["cases"]:
        assert ia.createBurrowsWheelerTransform(c["text"], build_device=0) == c["bwt"], c["name"]
    with pytest.raises(ValueError, match="Charset has more than 32767"):
        ia.createBurrowsWheelerTransform(np.arange(1, 32768, dtype=np.uint16), build_device=0)


def test_device_array_equals_host_array_16mib():
    text = ia.synth_log(1 << 23, seed=11)  # 16 MiB of UTF-16
    d = ia.SuffixArray(text, device=0).construct()
    h = ia.SuffixArray(text, device=None, build_device=-1).construct()
    raw = d.write(framed=False)
    assert raw == h.write(framed=False)
    assert d.hashCode() == h.hashCode()
    pat, off, _ = ia.synth_patterns(text, 8, 50000, seed=3)
    loaded = ia.SuffixArray.read(d.write(framed=True), device=0)
    assert (loaded.count_batch(pat, off) == d.count_batch(pat, off)).all()
    l1, f1, c1 = loaded.locate_batch(pat, off, max_matches=5)
    l2, f2, c2 = d.locate_batch(pat, off, max_matches=5)
    assert (l1 == l2).all() and (f1 == f2).all() and (c1 == c2).all()
    # a text with chars >= 0xD800 and more distinct chars than 16-bit codes leave room for is built on the host
    wide = np.arange(65536, dtype=np.uint16)[np.random.default_rng(1).permutation(65536)]
    a = ia.SuffixArray(wide, device=0).construct()
    b = ia.SuffixArray(wide, device=None, build_device=-1).construct()
    assert (a.getSuffixArray() == b.getSuffixArray()).all()


@pytest.fixture(scope="module")
def full():
    """the 256 MiB log (2^28 chars): SuffixArray built in HBM, FmIndex beside it, the host's array and its inverse"""
    text = ia.synth_log(1 << 28, seed=42)
    s = ia.SuffixArray(text, device=0).construct()
    fm = ia.FmIndexBuilder().setSampleRate(32).setEnableExtraction(False).setBuildDevice(0).build(text, device=0)
    sa = s.getSuffixArray()
    yield text, s, fm, sa
    s.close()


def _largest_starts_with(text, sa, pat, off):
    """[the suffix at row n starts with p] for a batch of patterns of one length"""
    n = len(text)
    top = int(sa[n])
    m = int(off[1] - off[0])
    assert (np.diff(off) == m).all()
    if m > n - top:
        return np.zeros(len(off) - 1, dtype=np.int32)
    return (pat.reshape(-1, m) == text[top:top + m]).all(axis=1).astype(np.int32)


def test_full_size_counts_equal_fm_index(full):
    text, s, fm, sa = full
    pat, off, _ = ia.synth_patterns(text, 8, 1 << 20, seed=43)
    sets = [(pat, off)]
    rng = np.random.default_rng(7)
    absent = pat[: 8 * 20000].copy().reshape(-1, 8)
    absent[:, rng.integers(0, 8, len(absent))] = 0x7F  # no log line holds DEL
    sets.append((absent.ravel(), np.arange(0, 8 * len(absent) + 1, 8, dtype=np.int32)))
    for m in range(1, 65):
        sets.append(ia.synth_patterns(text, m, 3000, seed=100 + m)[:2])
    for p, o in sets:
        got = s.count_batch(p, o)
        exp, status = fm.count_batch(p, o)
        assert (status == 0).all()
        exp = exp - _largest_starts_with(text, sa, p, o)
        assert (got == exp).all(), int(np.nonzero(got != exp)[0][0])


def test_full_size_locate(full):
    text, s, fm, sa = full
    pat, off, _ = ia.synth_patterns(text, 8, 100000, seed=44)
    locs, found, counts = s.locate_batch(pat, off, max_matches=16)
    assert (found == np.minimum(counts, 16)).all()
    flocs, ffound, fst = fm.locate_batch(pat, off, 16)
    small = np.nonzero(counts <= 16)[0]
    assert len(small) > 1000
    for i in small[:20000]:
        assert sorted(locs[i, :found[i]].tolist()) == sorted(flocs[i, :ffound[i]].tolist()), i
    inv = np.empty(len(sa), dtype=np.int64)
    inv[sa] = np.arange(len(sa))
    for i in range(0, len(found), 7):
        k = int(found[i])
        if k == 0:
            continue
        rows = inv[locs[i, :k]]
        assert (rows == rows[0] + np.arange(k)).all(), i
        first = int(rows[0])  # the first matching row: the row before it does not start with the pattern
        p = pat[off[i]:off[i + 1]]
        q = int(sa[first - 1])
        assert first == 0 or not (len(p) <= len(text) - q and (text[q:q + len(p)] == p).all()), i


@pytest.mark.parametrize("block,gpc", [(512, 1), (1024, 1), (512, 16), (1024, 16)])
def test_launch_shapes(block, gpc, tmp_path_factory):
    """every new kernel at the four shapes; at one workgroup per CU every batch loops the grid at least three times"""
    sim = sim_lib(tmp_path_factory.mktemp("sahostsim"))
    text = ia.synth_log(1 << 20, seed=9)
    h = ia.SuffixArray(text, device=None, build_device=-1).construct()
    sa = h.getSuffixArray()
    lanes = 3 * n_cu() * 1024 + 17
    pat, off, _ = ia.synth_patterns(text, 8, lanes, seed=21)
    pats = [pat[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    left, right, _ = sim_search(sim, text, sa, pats)
    exp = right - left
    try:
        assert ia.lib.fmx_set_option(b"block", block) == 0
        assert ia.lib.fmx_set_option(b"groups_per_cu", gpc) == 0
        s = ia.SuffixArray(text, device=0).construct()
        assert (s.getSuffixArray() == sa).all()
        assert (s.count_batch(pat, off) == exp).all()
        m = 4  # locate: n * m flattened hit lanes, at least three passes as well
        locs, found, counts = s.locate_batch(pat, off, max_matches=m, fill=-3)
        assert (counts == exp).all() and (found == np.minimum(exp, m)).all()
        assert int(found.sum()) >= 3 * n_cu() * 1024
        for i in range(0, len(pats), 97):
            k = int(found[i])
            assert locs[i, :k].tolist() == sa[left[i]:left[i] + k].tolist() and (locs[i, k:] == -3).all(), i
        t = text[: 1 << 16]
        assert len(ia.createBurrowsWheelerTransform(t, build_device=0)) == len(t) + 1
        assert (ia.createBurrowsWheelerTransform(t, build_device=0) == ia.createBurrowsWheelerTransform(t, build_device=-1)).all()
    finally:
        ia.lib.fmx_set_option(b"block", ia._lib.ENV_OPTIONS.get("block", 512))
        ia.lib.fmx_set_option(b"groups_per_cu", ia._lib.ENV_OPTIONS.get("groups_per_cu", 16))


@pytest.fixture(scope="module")
def fence_reference(tmp_path_factory):
    """the text and patterns of test_fence_settings_change_no_answer, and right - left of every pattern by the search routines
    on the host (no fence table) over the array of host SA-IS: nothing of it comes from the device"""
    sim = sim_lib(tmp_path_factory.mktemp("sahostsim"))
    text = ia.synth_log(1 << 20, seed=13)
    pat, off, _ = ia.synth_patterns(text, 12, 200000, seed=5)
    sa = ia.SuffixArray(text, device=None, build_device=-1).construct().getSuffixArray()
    left, right, nf = sim_search(sim, text, sa, [pat[off[i]:off[i + 1]] for i in range(len(off) - 1)], most=0)
    assert nf == 0
    return text, pat, off, right - left


@pytest.mark.parametrize("fences,chars", [(0, 8), (4096, 8), (8192, 4), (32768, 1)])
def test_fence_settings_change_no_answer(fences, chars, fence_reference):
    text, pat, off, exp = fence_reference
    base = None
    try:
        assert ia.lib.fmx_set_option(b"sa_fences", fences) == 0
        assert ia.lib.fmx_set_option(b"sa_fence_chars", chars) == 0
        s = ia.SuffixArray(text, device=0).construct()
        got = s.count_batch(pat, off)
    finally:
        ia.lib.fmx_set_option(b"sa_fences", 4096)
        ia.lib.fmx_set_option(b"sa_fence_chars", 8)
    base = ia.SuffixArray(text, device=0).construct().count_batch(pat, off)
    assert (got == base).all()
    assert (got == exp).all() and (base == exp).all(), int(np.nonzero((got != exp) | (base != exp))[0][0])

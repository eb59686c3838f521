"""The values that follow a pattern, with counts on the GPU (grep -o 'blk_[^ ]*' | sort | uniq -c): packed hits -> the distinct values
behind each pattern (fmx_values_of_hits_dev / fmx_values_fill_dev: the kernels of fmx_hit_values.hip around the packed extract and
rocPRIM's sorts and scans) and the host forms fmx_field_values_batch / fmx_field_values_class_batch, with their Python and C++
mirrors.

The judge is the oracle plus Python/numpy (tests/test_field_values_cpu.py: judge_values — expected_packed's hits, the oracle's
extract over every window, a dict per pattern, `sorted` on tuples of code units), computed once per batch.  Outputs are prefilled
with a sentinel, and everything behind the answer must keep it.  Options are set inside the tests and put back in `finally`."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import K_TEXT, NAMED, SENT16, assert_named, check_values, judge_values
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import _torch, options, run_block_text
from test_locate_all_cpu import SENT, assert_corner_cases, corner_batch, expected_packed
from test_match_sequence_cpu import occurrences_in_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel
SENT64 = -0x3C3C3C3C3C3C3C3D
ST_NOT_ENABLED, ST_AIOOBE, ST_TOO_MANY = 1, 9, 10


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def host_values(fm, ch, off, stop, max_len):
    """(chars, text_off, counts, val_off) with sentinels behind, status, occurrences"""
    chars, text_off, counts, val_off, st, occ = fm.field_values_batch(ch, off, stop, max_len)
    return padded(chars, text_off, counts, val_off), st, occ


def padded(chars, text_off, counts, val_off):
    return (np.concatenate([chars, np.full(PAD, SENT16, np.uint16)]), np.concatenate([text_off, np.full(PAD, SENT64, np.int64)]),
            np.concatenate([counts, np.full(PAD, SENT, np.int32)]), val_off)


def check_sentinels(got, want, what):
    chars, text_off, counts, val_off = got
    G, T = int(want.val_off[-1]), int(want.text_off[-1])
    assert len(counts) > G and (counts[G:] == SENT).all(), what + ": stored behind the last group's count"
    assert len(text_off) > G + 1 and (text_off[G + 1:] == SENT64).all(), what + ": stored behind text_off[G]"
    assert len(chars) > T and (chars[T:] == SENT16).all(), what + ": stored behind the last value"


def check(got, want, what):
    check_values(got, want, what)
    check_sentinels(got, want, what)


def filled(fm, ch, off):
    d = DevAll(fm, ch, off, -1)
    d.fill(0, d.total)
    return d


def dev_values(d, lens, stop, max_len, extra_hits=0, ws_bytes=None, with_status=True):
    """both device stages over what a DevAll (the two packed locate stages) left; extra_hits: n_hits beyond hit_off[n].
    Returns rc, (chars, text_off, counts, val_off), status"""
    torch, n = d.torch, d.n
    n_hits = d.total + extra_hits
    assert extra_hits <= 64  # (d.locs has that many slots behind the hits)
    need = ia.lib.fmx_values_of_hits_scratch_bytes(n, n_hits, max_len)
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    val_off = torch.full((n + 1,), SENT64, dtype=torch.int64, device="cuda")
    counts = torch.full((n_hits + PAD,), SENT, dtype=torch.int32, device="cuda")
    text_off = torch.full((n_hits + 1 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    tl = np.array(lens, np.int32)  # the call's own copies: scribbled over once it is back
    sp = ia.as_chars(stop).copy()
    rc = ia.lib.fmx_values_of_hits_dev(d.fm.handle, n, tl.ctypes.data, sp.ctypes.data, len(sp), max_len, d.hit_off.data_ptr(), d.locs.data_ptr(),
                                       n_hits, val_off.data_ptr(), counts.data_ptr(), text_off.data_ptr(), d.st.data_ptr() if with_status else None,
                                       ws.data_ptr(), use, d.stream)
    tl[:] = -9  # (the call has copied what it needs before it returns)
    sp[:] = 0x41
    torch.cuda.synchronize()
    out = [None, text_off.cpu().numpy(), counts.cpu().numpy(), val_off.cpu().numpy()]
    status = d.st.cpu().numpy()[:n]
    if rc or out[3][n] == SENT64:
        return rc, tuple(out), status
    G = int(out[3][n])
    T = int(out[1][G])
    chars = torch.full((T + PAD,), SENT16 - 65536, dtype=torch.int16, device="cuda")
    rc = ia.lib.fmx_values_fill_dev(d.fm.handle, G, text_off.data_ptr(), chars.data_ptr(), ws.data_ptr(), use, d.stream)
    torch.cuda.synchronize()
    out[0] = chars.cpu().numpy().view(np.uint16)
    return rc, tuple(out), status


def judged(key, o, ch, off, stop, max_len, lens=None):
    locs, hit_off, status, _, counts = expected_packed(key, o, ch, off, -1)
    return judge_values(o, locs, hit_off, np.diff(off) if lens is None else lens, stop, max_len), status, counts


def named_batch(pattern):
    ch, off = ia.pack_patterns([pattern])
    return ch, off.astype(np.int32)


@pytest.fixture(scope="module")
def hd():
    t16 = ia.as_chars(HD)
    assert len(t16) == 315118 and len(np.unique(t16)) == 762 and int(t16.max()) == 40670
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    yield t16, o, fm
    fm.close()


_NAMED = {}


def named_judged(o):
    """the judge's answers for the named cases, computed once; the fixture's numbers asserted on them"""
    if not _NAMED:
        for k, (pattern, stop, max_len, hits, values, top) in enumerate(NAMED):
            ch, off = named_batch(pattern)
            locs = expected_packed("hd16 values " + repr(pattern), o, ch, off, -1)[0]
            assert (np.sort(locs) == occurrences_in_text(HD, pattern)).all()  # the oracle's hits are exactly the text's occurrences
            want, status, counts = judged("hd16 values " + repr(pattern), o, ch, off, stop, max_len)
            assert_named(want, 0, pattern, hits, values, top)
            if pattern == "/10.":
                assert want.runs[0] > values  # in the ORACLE's hit order: more runs than values — runs alone are not the answer
            _NAMED[k] = (ch, off, want, counts)
    return _NAMED


def run_named(hd, what):
    t16, o, fm = hd
    for k, (pattern, stop, max_len, hits, values, top) in enumerate(NAMED):
        ch, off, want, counts = named_judged(o)[k]
        w = "%s: %r stop %r max_len %d" % (what, pattern, stop, max_len)
        got, st, occ = host_values(fm, ch, off, stop, max_len)
        check(got, want, w + ", host form")
        assert list(st) == [0] and list(occ) == [hits]
        rc, dev, dst = dev_values(filled(fm, ch, off), np.diff(off), stop, max_len)
        assert rc == 0, last_error()
        check(dev, want, w + ", device form")
        assert list(dst) == [0]
        pairs = fm.field_values(pattern, stop=stop, max_len=max_len)
        assert pairs == want.strings(0), w + ", FmIndex.field_values"
        assert sum(c for _, c in pairs) == hits and len(pairs) == values
        by_count = sorted(want.strings(0), key=lambda vc: (-vc[1], vc[0]))
        assert fm.field_values(pattern, stop=stop, max_len=max_len, top=3) == by_count[:3]
        if top:
            assert fm.field_values(pattern, stop=stop, max_len=max_len, top=len(top)) == top


def test_named_cases(hd):
    run_named(hd, "defaults")
    t16, o, fm = hd
    assert fm.field_values("INFO ", stop=" \n:", max_len=64, top=3) == NAMED[3][5]
    assert fm.field_values("blk_", top=0) == [] and len(fm.field_values("blk_")) == 2199  # (the default stop set and max_len)
    assert fm.field_values("zzqq#") == []
    with pytest.raises(IndexError):
        fm.field_values("")


@pytest.mark.parametrize("opts", [dict(block=1024), dict(groups_per_cu=1)])
def test_named_cases_launch_shapes(hd, opts):
    with options(**opts):
        run_named(hd, repr(opts))


def small_case(text, patterns, stop, max_len, key, lens=None, sr=4):
    """a text of a few dozen characters: host and device forms against the judge; returns the judge's answer"""
    o = orc.OracleFmIndex(text, sr, True)
    fm = ia.FmIndex(text, sr, True, device=0)
    try:
        ch, off = ia.pack_patterns(patterns)
        off = off.astype(np.int32)
        want, status, counts = judged(key, o, ch, off, stop, max_len, lens)
        what = "%s stop %r max_len %d" % (key, stop, max_len)
        if lens is None:
            got, st, occ = host_values(fm, ch, off, stop, max_len)
            check(got, want, what + ", host form")
            assert (st == status).all() and (occ == counts).all()
        rc, dev, dst = dev_values(filled(fm, ch, off), np.diff(off) if lens is None else lens, stop, max_len)
        assert rc == 0, last_error()
        check(dev, want, what + ", device form")
        return want
    finally:
        fm.close()


def test_synthetic_texts():
    want = small_case(K_TEXT, ["k="], " .", 8, "k text")
    assert want.strings(0) == [("a", 4), ("a-", 1), ("ab", 1)]  # "a" by two terminators, "a-" between them; the prefix order
    # values that differ only in the 4th, 5th, 8th and 9th code unit (the edges of the sort's chunks); the last occurrence of the
    # pattern ends at textLength (the empty value); max_len 1 and 64
    base = "abcdefghij"
    variants = [base] + [base[:k] + c + base[k + 1:] for k in (3, 4, 7, 8) for c in ("A", "z")]
    text = "".join("v=%s;" % v for v in variants + variants[::-2]) + "v="
    for max_len in (1, 9, 64):
        want = small_case(text, ["v=", "=", "zz"], ";", max_len, "chunk edges 3")
        got = want.strings(0)
        assert [v for v, _ in got] == sorted({v[:max_len] for v in variants} | {""}) and dict(got)[""] == 1
        assert want.strings(1) == got and want.strings(2) == []  # two patterns that share their values: two answers
    # a value and the same value followed by U+0000, in a text that holds U+0000 and whose stop set does not
    text0 = "v=ab;v=ab\0;v=ab\0\0;v=ab;v=a;v=ab\0c;v=ab\0;"
    want = small_case(text0, ["v="], ";", 12, "nul")
    assert want.strings(0) == [("a", 1), ("ab", 2), ("ab\0", 2), ("ab\0\0", 1), ("ab\0c", 1)]
    # n_stop = 0: every value is its window; n_stop = 64 with duplicates in the set
    want = small_case(text0, ["v="], "", 3, "nul")
    assert all(len(v) == 3 for v, _ in want.per[0]) and sum(c for _, c in want.per[0]) == 7
    small_case(text0, ["v="], ";" * 40 + "c" * 24, 12, "nul")
    # the caller's lengths (device form): a length that runs over the text's end leaves the empty value alone
    want = small_case(text0, ["v="], ";", 12, "nul", lens=[2 ** 31 - 1])
    assert want.strings(0) == [("", 7)]


@pytest.fixture(scope="module")
def mixed(hd):
    """the corner-case batch of tests/test_gpu_locate_all.py (about 10^6 hits) with "blk_" twice and "lk_" behind it"""
    t16, o, fm = hd
    ch, off = corner_batch(t16, np.random.default_rng(16), 2900, min_len=2)
    more = ia.pack_patterns(["blk_", "lk_", "blk_"])
    ch2 = np.concatenate([ch, more[0]])
    off2 = np.concatenate([off, off[-1] + more[1][1:]]).astype(np.int32)
    want, status, counts = judged("hd16 values mixed", o, ch2, off2, " \n", 12)
    n = len(off2) - 1
    assert_corner_cases(counts[:n - 3], status[:n - 3])
    assert int(counts.sum()) > 900_000 and (counts == 0).sum() > 75 and (status == ST_AIOOBE).sum() == 1
    assert want.per[n - 3] == want.per[n - 1] == want.per[n - 2] and len(want.per[n - 1]) == 2199  # the same pattern twice; shared values
    assert want.per[int(np.flatnonzero(status == ST_AIOOBE)[0])] == []
    return ch2, off2, want, status, counts


def test_mixed_batch(hd, mixed):
    t16, o, fm = hd
    ch, off, want, status, counts = mixed
    got, st, occ = host_values(fm, ch, off, " \n", 12)
    check(got, want, "mixed batch, host form")
    assert (st == status).all() and (occ == counts).all()
    d = filled(fm, ch, off)
    rc, dev, dst = dev_values(d, np.diff(off), " \n", 12)
    assert rc == 0, last_error()
    check(dev, want, "mixed batch, device form")  # (the host arrays were scribbled over when the call returned)
    assert (dst == status).all()
    rc, dev, dst = dev_values(d, np.diff(off), " \n", 12, extra_hits=37, with_status=False)
    assert rc == 0, last_error()
    check(dev, want, "mixed batch, n_hits beyond hit_off[n]")
    # a workspace one byte too small: FMX_E_ARG, nothing launched, sentinels intact
    need = ia.lib.fmx_values_of_hits_scratch_bytes(d.n, d.total, 12)
    rc, dev, dst = dev_values(d, np.diff(off), " \n", 12, ws_bytes=need - 1)
    assert rc == ia._lib.E_ARG and (dev[1] == SENT64).all() and (dev[2] == SENT).all() and (dev[3] == SENT64).all()


def test_class_form(hd):
    t16, o, fm = hd
    words = ["block", "info ", "src: /", "zzqqzz"]
    patterns = [ia.ignore_case(w) for w in words]
    alt, pos_off, pat_off = ia.pack_class_patterns(patterns)
    # the judge over the union of the spellings' hits: every spelling the text holds, as a literal
    spellings = [sorted(set(re.findall("(?i)" + re.escape(w), HD))) for w in words]
    assert len(spellings[0]) > 1 and spellings[3] == []
    flat = [s for sp in spellings for s in sp]
    ch, off = ia.pack_patterns(flat)
    off = off.astype(np.int32)
    locs, hit_off, _, _, lit_counts = expected_packed("hd16 values spellings", o, ch, off, -1)
    bounds = np.concatenate([[0], np.cumsum([len(sp) for sp in spellings])])
    class_hit_off = hit_off[bounds]
    lens = [len(w) for w in words]
    want = judge_values(o, locs, class_hit_off, lens, " \n:", 20)
    chars, text_off, counts, val_off, st, occ = fm.field_values_class_batch(alt, pos_off, pat_off, " \n:", 20)
    check(padded(chars, text_off, counts, val_off), want, "class form")
    assert (st == 0).all() and (occ == np.diff(class_hit_off)).all() and occ[0] == 2662
    assert fm.field_values("BLOCK", stop=" \n:", max_len=20, ignore_case=True) == want.strings(0)
    assert fm.field_values("bLOCK", stop=" \n:", max_len=20) == []
    # a frontier larger than max_ranges: FMX_ST_TOO_MANY_RANGES and no values; the others keep their answers
    _, cst = fm.count_class_batch(alt, pos_off, pat_off, max_ranges=1)
    assert ST_TOO_MANY in cst.tolist()
    chars, text_off, counts, val_off, st, occ = fm.field_values_class_batch(alt, pos_off, pat_off, " \n:", 20, max_ranges=1)
    assert (st == cst).all()
    for i in range(len(words)):
        mine = [(tuple(chars[text_off[g]:text_off[g + 1]].tolist()), int(counts[g])) for g in range(val_off[i], val_off[i + 1])]
        assert mine == ([] if cst[i] == ST_TOO_MANY else want.per[i]), words[i]


def test_index_without_extraction(hd):
    t16, o, fm0 = hd
    fm = ia.FmIndex(HD, 16, False, device=0)
    try:
        ch, off = ia.pack_patterns(["blk_", "", "INFO", "zzqq#"])
        off = off.astype(np.int32)
        counts = expected_packed("hd16 values not enabled", o, ch, off, -1)[4]
        chars, text_off, vcounts, val_off, st, occ = fm.field_values_batch(ch, off, " \n", 8)
        assert (st == ST_NOT_ENABLED).all() and (val_off == 0).all() and len(vcounts) == 0 and len(chars) == 0
        assert (occ == counts).all() and occ[0] == 2468
        rc, dev, dst = dev_values(filled(fm, ch, off), np.diff(off), " \n", 8)
        assert rc == 0, last_error()
        assert (dst == ST_NOT_ENABLED).all() and (dev[3] == 0).all() and dev[1][0] == 0 and (dev[1][1:] == SENT64).all() and (dev[2] == SENT).all()
        with pytest.raises(RuntimeError):
            fm.field_values("blk_")
    finally:
        fm.close()


def test_errors_and_edges(hd):
    t16, o, fm = hd
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    torch = _torch()
    ch, off = named_batch("blk_")
    stop = ia.as_chars(" \n")
    host = ia.lib.fmx_field_values_batch
    val_off = np.full(2, SENT64, np.int64)

    def call(handle=None, n_stop=2, max_len=8, stop_at=stop.ctypes.data, vo=val_off):
        a, b, c = C.c_void_p(0x1234), C.c_void_p(0x1234), C.c_void_p(0x1234)
        rc = host(fm.handle if handle is None else handle, ch.ctypes.data, off.ctypes.data, 1, stop_at, n_stop, max_len,
                  None if vo is None else vo.ctypes.data, C.byref(a), C.byref(b), C.byref(c), None, None)
        assert rc == 0 or (a.value is None and b.value is None and c.value is None)  # every output pointer is NULL on every failure
        if rc == 0:
            ia.lib.fmx_free_buffer(a)
        return rc

    assert call() == 0 and val_off[1] == 2199
    val_off[:] = SENT64
    for bad in (dict(max_len=0), dict(max_len=65), dict(n_stop=-1), dict(n_stop=65), dict(stop_at=None), dict(vo=None)):
        assert call(**bad) == E_ARG and (val_off == SENT64).all(), bad
    assert call(n_stop=0, stop_at=None) == 0  # (no stop set needs no array)
    # the device form: each FMX_E_ARG leaves the sentinels alone
    d = filled(fm, ch, off)
    untouched = lambda dev: (dev[1] == SENT64).all() and (dev[2] == SENT).all() and (dev[3] == SENT64).all()
    for lens, stp, max_len in (([4], " \n", 0), ([4], " \n", 65), ([-1], " \n", 8), ([4], " " * 65, 8)):
        rc, dev, _ = dev_values(d, lens, stp, max_len)
        assert rc == E_ARG and untouched(dev), (lens, stp, max_len)
    dv = ia.lib.fmx_values_of_hits_dev
    sizes = ia.lib.fmx_values_of_hits_scratch_bytes
    one = np.array([4], np.int32)
    p = torch.zeros(16, dtype=torch.int64, device="cuda")
    for n_hits, max_len in ((2 ** 31, 1), (2 ** 30, 64), (-1, 8)):  # more than 2^31 - 1 hits; n_hits * max_len above 2^35; negative
        assert sizes(1, n_hits, max_len) == 0
        assert dv(fm.handle, 1, one.ctypes.data, stop.ctypes.data, 2, max_len, p.data_ptr(), p.data_ptr(), n_hits, p.data_ptr(), p.data_ptr(),
                  p.data_ptr(), None, p.data_ptr(), 128, d.stream) == E_ARG
    assert dv(fm.handle, 1, one.ctypes.data, stop.ctypes.data, 2, 8, p.data_ptr(), p.data_ptr(), 5, None, p.data_ptr(), p.data_ptr(), None,
              p.data_ptr(), 128, d.stream) == E_ARG  # a null output
    assert ia.lib.fmx_values_fill_dev(fm.handle, -1, p.data_ptr(), p.data_ptr(), p.data_ptr(), 128, d.stream) == E_ARG
    assert ia.lib.fmx_values_fill_dev(fm.handle, 64, p.data_ptr(), p.data_ptr(), p.data_ptr(), 128, d.stream) == E_ARG  # (64 groups: 512 bytes)
    torch.cuda.synchronize()
    assert int(p.cpu().abs().sum()) == 0
    # n == 0 and n_hits == 0: the n + 1 offsets and d_text_off[0] are zeroed, nothing else is written
    vo = torch.full((2,), SENT64, dtype=torch.int64, device="cuda")
    to = torch.full((2,), SENT64, dtype=torch.int64, device="cuda")
    assert dv(fm.handle, 0, None, None, 0, 8, None, None, 0, vo.data_ptr(), None, to.data_ptr(), None, None, 0, d.stream) == 0
    torch.cuda.synchronize()
    assert vo.cpu().tolist() == [0, SENT64] and to.cpu().tolist() == [0, SENT64]
    ch0, off0 = ia.pack_patterns(["zzzzqq#", "", "qqqqzz#"])
    off0 = off0.astype(np.int32)
    d0 = filled(fm, ch0, off0)
    assert d0.total == 0
    rc, dev, dst = dev_values(d0, np.diff(off0), " ", 8)
    assert rc == 0 and (dev[3] == 0).all() and dev[1][0] == 0 and (dev[1][1:] == SENT64).all() and (dev[2] == SENT).all() and list(dst) == [0, 9, 0]
    chars, text_off, counts, val_off0, st, occ = fm.field_values_batch(ch0, off0, " ", 8)
    assert len(chars) == 0 and len(counts) == 0 and (val_off0 == 0).all() and list(st) == [0, 9, 0] and (occ == 0).all()
    out = fm.field_values_batch(np.zeros(0, np.uint16), [0], " ", 8)
    assert len(out[2]) == 0 and list(out[3]) == [0]
    # the wrong handle kinds; a handle that is not resident
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for other in (sa._h, rrr._h, wt._h):
        assert call(handle=other) == E_ARG
        assert dv(other, 1, one.ctypes.data, stop.ctypes.data, 2, 8, p.data_ptr(), p.data_ptr(), 5, p.data_ptr(), p.data_ptr(), p.data_ptr(), None,
                  p.data_ptr(), 128, d.stream) == E_ARG
    bare = ia.FmIndex("abracadabra", 4, True, device=None)
    assert call(handle=bare.handle) == E_NO_DEVICE
    assert dv(bare.handle, 1, one.ctypes.data, stop.ctypes.data, 2, 8, p.data_ptr(), p.data_ptr(), 5, p.data_ptr(), p.data_ptr(), p.data_ptr(), None,
              p.data_ptr(), 128, d.stream) == E_NO_DEVICE


def test_quirk_rows_follow_the_reference_extract():
    """the fixture followed by the run-block text (quirk Q1: its rows derail the reference's walks, the packed extract's redo list is
    not empty): the answer equals the judge built on the ORACLE's extract, not on the text"""
    text = HD + run_block_text()
    t16 = ia.as_chars(text)
    o = orc.OracleFmIndex(text, 16, True)
    pats = [chr(0x30A9), "log line ", chr(0x30AC) * 3, "\n"]
    ch, off = ia.pack_patterns(pats)
    off = off.astype(np.int32)
    want, status, counts = judged("hd+runblocks values", o, ch, off, " \n", 16)
    # the oracle's windows are not the text's: the same grouping over the TEXT behind the oracle's hits gives another answer
    locs, hit_off = expected_packed("hd+runblocks values", o, ch, off, -1)[:2]

    def text_value(p):
        w = t16[p:p + 16].tolist()
        return tuple(w[:next((k for k, u in enumerate(w) if u in (32, 10)), len(w))])

    by_text = collections.Counter(text_value(int(h) + 1) for h in locs[hit_off[0]:hit_off[1]])
    assert counts[0] == 70_000 and dict(want.per[0]) != dict(by_text)
    fm = ia.FmIndex(text, 16, True, device=0)
    try:
        got, st, occ = host_values(fm, ch, off, " \n", 16)
        assert ia.lib.fmx_extract_packed_last_redo() > 0  # the redo list IS non-empty on this index
        check(got, want, "quirk rows, host form")
        assert (occ == counts).all()
        rc, dev, dst = dev_values(filled(fm, ch, off), np.diff(off), " \n", 16)
        assert rc == 0, last_error()
        check(dev, want, "quirk rows, device form")
    finally:
        fm.close()


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_field_values_mirror.cpp prints what fieldValuesBatch / fieldValues return"""
    t16, o, fm = hd
    exe = str(tmp_path / "test_field_values_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_field_values_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    ch, off = ia.pack_patterns(["blk_", "zzqq#", "INFO ", "\n"])
    off = off.astype(np.int32)
    want, status, counts = judged("hd16 values mirror", o, ch, off, " \n:", 24)
    assert out["batch_val_off"] == list(want.val_off) and out["batch_counts"] == list(want.counts)
    assert out["batch_text_off"] == list(want.text_off) and out["batch_chars"] == list(want.chars)
    assert out["batch_occurrences"] == list(counts) == [2468, 0, 1920, 2000] and out["batch_status"] == [0, 0, 0, 0]
    top = sorted(want.per[2], key=lambda vc: (-vc[1], vc[0]))[:3]
    assert out["one_counts"] == [c for _, c in want.per[2]] and out["top_counts"] == [c for _, c in top] == [525, 480, 283]
    assert out["top_chars"] == [u for v, _ in top for u in v] and out["icase_values"] == [len(judged_icase_block(o))]


def judged_icase_block(o):
    spellings = sorted(set(re.findall("(?i)block", HD)))
    ch, off = ia.pack_patterns(spellings)
    off = off.astype(np.int32)
    locs, hit_off = expected_packed("hd16 values block spellings", o, ch, off, -1)[:2]
    return judge_values(o, locs, hit_off[[0, len(spellings)]], [5], " \n:", 24).per[0]

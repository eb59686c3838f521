"""The ORDER the plan stage of a count batch produces, against a plain numpy model of its contract (tests/plan_model.py).

The other plan tests assert that counts, hits and statuses do not depend on the order — which holds by construction (results are
written at the original index), so any permutation passes them.  Here the records themselves are read back and compared:

  a  the ordered records are a permutation of the batch;
  b  record i carries the code word and the length field of pattern a[i]; bits 22..31 of `m` are zero where k_plan_fine ran and
     the fine bin of the pattern's key where it did not;
  c  the coarse bins of the keys are non-decreasing along the bucket order, each bin's run as long as the histogram of the keys
     says (behind k_plan_fine: every window holds those bins as a multiset, and the run without it is checked as well);
  d  under the code key (plan_sa_key 0, or no suffix table) the device's keys equal the model's, bit for bit, at sort_bits
     1 / 9 / 28 / 32 x coarse_bits 4 / 12 / 13;
  e  where k_plan_fine ran, the fine bins are non-decreasing inside every window of 1,024 records and no record left its window;
  f  plan_sa_key 1: the key is the first SA row of the pattern's tabulated suffix (the model's sorted suffixes);
  g  plan_sa_key 2: the estimate stays within a derived float32 tolerance of the row range of the suffix's first two characters
     and is monotone in the suffix's lexicographic order, as plan_record's comment states;
  h  k_plan_fused gives the same (its documented abort — the caller's order, with code words — only at plan_spin_limit 0);
  i  back-to-back plans on one stream find the workspace head (histogram, cursors, ticket) clean;
  j  fmx_count_ordered_dev over the plan just checked gives the oracle's counts and statuses.

How the records are read.  fmx_count_plan_dev returns the device address of PlanRec[n] in processing order, 16 bytes each
{u64 cw, u32 a, u32 m}; torch copies them to the host from an object whose __cuda_array_interface__ names that address (hipMemcpy
through the HIP runtime already mapped into the process only if torch refuses) — no export is added.  The workspace layout
documented above count_workspace_bytes() puts the records BY PATTERN — k_plan_codes' output {cw, key, length | fine bin << 22} —
directly in front of the handle, at handle - 16 * n: they give the keys exactly as the device computed them.  That is a white-box
read, and the exact-key check (d) is what proves it looks at the right bytes: a block that was not k_plan_codes' output would not
hold, for every pattern of every batch, the model's code word, key and length.  The block is filled with a marker before a plan,
which also tells the two-kernel path (block rewritten) from k_plan_fused (block untouched).

Not covered: the walk order of locate (k_walk_hist + k_plan_scatter<true>) and the position order of extractUntilBoundary.  Their
records stay in private scratch and cannot be read without a new export; they share the scatter and fine kernels tested here, but
their zero bin (patterns with nothing to locate) is not exercised.  The `mixed` flag is not observable either.  Nor is which of
the two plan_sa_key 2 paths a plan took: index L's order-1 table fits k_plan_codes' LDS behind 4,096 bins but not behind 8,192, so
(g) on L covers the LDS path at coarse_bits <= 12 only; at 13 — and on B, R12, R16 always — it covers the table lookups."""
import contextlib
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import index4j_amd as ia
import orc
import plan_model as pm
from index4j_amd import workload

pytestmark = pytest.mark.gpu

SENT = -0x3C3C3C3D  # (as tests/test_gpu_launch_shapes.py) int32 outputs: no count or status the kernels write
THREADS = 16
REC = np.dtype([("cw", "<u8"), ("a", "<u4"), ("m", "<u4")])
MARK = 0xA5  # fills the by-pattern block before a plan: 0xA5A5... is no record of these batches (lengths stay below it)
SIZES = [1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 16384, 100000, 1048576]  # 1,024: the fine window; 4,096: the tile

# the value every option this module sets goes back to (the four that conftest.py holds for GPU tests are not touched)
LIB_DEFAULTS = {"sort_min": 16384, "sort_bits": 28, "coarse_bits": 12, "plan_fine": 1, "plan_sa_key": 2, "plan_fused": 0,
                "plan_spin_limit": 4096, "code_bits_12": 1, "suffix_table_mb": 256, "suffix_table_image_fraction": 8}
CUR = {k: ia._lib.ENV_OPTIONS.get(k, v) for k, v in LIB_DEFAULTS.items()}  # what the library holds right now


@contextlib.contextmanager
def options(**kw):
    before = {k: CUR[k] for k in kw}
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
            CUR[k] = int(v)
        yield
    finally:
        for k, v in before.items():
            ia.lib.fmx_set_option(k.encode(), v)
            CUR[k] = v


def _torch():
    import torch

    return torch


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def ok(rc, what):
    assert rc == 0, "%s: %s" % (what, (ia.lib.fmx_last_error() or b"").decode())


# ---- device memory behind a raw address -------------------------------------------------------------------------------------------

class _Span:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


_HIP = []


def _hip():
    """the HIP runtime this process already has mapped (never a second copy)"""
    if not _HIP:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        lib = C.CDLL(path)
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        _HIP.append(lib)
    return _HIP[0]


def _alias(ptr, nbytes):
    try:
        return _torch().as_tensor(_Span(ptr, nbytes), device="cuda")
    except TypeError:  # (torch refuses the interface: hipMemcpy / hipMemset below; any other error is an error)
        return None


def dev_read(ptr, nbytes):
    """bytes [ptr, ptr + nbytes) of device memory, after everything queued on the current stream"""
    t = _alias(ptr, nbytes)
    if t is not None:
        out = t.cpu().numpy().copy()
        _torch().cuda.synchronize()
        return out
    _torch().cuda.synchronize()
    out = np.empty(nbytes, dtype=np.uint8)
    assert _hip().hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def dev_fill(ptr, nbytes, byte):
    t = _alias(ptr, nbytes)
    if t is not None:
        t.fill_(byte)  # (on the current stream: ordered with the plans around it)
        return
    _torch().cuda.synchronize()
    assert _hip().hipMemset(ptr, byte, nbytes) == 0
    _torch().cuda.synchronize()


# ---- texts, indexes, batches --------------------------------------------------------------------------------------------------------

def wide_byte_text(log):
    """~200 distinct symbols below 256 out of the log text: three dialects of its alphabet, one per line in turn"""
    syms = np.unique(log)
    idx = np.searchsorted(syms, log)
    line = np.cumsum(log == 10) - (log == 10)
    shifted = idx + len(syms) * (line % 3)
    shifted[log == 10] = idx[log == 10]
    out = (1 + shifted).astype(np.uint16)
    assert out.max() < 256
    return out


class Batch:
    def __init__(self, name, ch, off, skew=False):
        torch = _torch()
        self.name = name
        self.ch = np.ascontiguousarray(ch, dtype=np.uint16)
        self.off = np.ascontiguousarray(off, dtype=np.int32)
        self.n = len(self.off) - 1
        self.m = pm.lengths(self.off)
        if skew:  # d_pat one uint16 into its allocation: half-word aligned, not dword aligned
            self._base = torch.empty(len(self.ch) + 1, dtype=torch.int16, device="cuda")
            self.d_ch = self._base[1:]
            self.d_ch.copy_(torch.from_numpy(self.ch.view(np.int16)))
            assert self.d_ch.data_ptr() % 4 == 2
        else:
            self.d_ch = torch.from_numpy(self.ch.view(np.int16)).cuda()
        self.d_off = torch.from_numpy(self.off).cuda()
        self._words = {}

    def words(self, ix):
        if ix.key not in self._words:
            self._words[ix.key] = pm.code_words(ix.al, self.ch, self.off, ix.code_bits)
        return self._words[ix.key]


def absent_chars(al):
    lo = next(c for c in range(1, 256) if c not in al.symbols)
    hi = next(c for c in (0x7A7B, 0xFFFD, 0xE000, 0xE001) if c not in al.symbols)
    return lo, hi


def make_patterns(text, al, n, rng, lo, hi):
    """n substrings of lo..hi characters, cut wherever they fall (odd and even offsets); the first eight have lengths 0..7 when
    lo == 0; every 50th holds an absent character — below 256 and above in turn — at a random place or at its end"""
    lens = rng.integers(lo, hi + 1, n).astype(np.int64)
    if lo == 0:
        lens[:8] = np.arange(8)
    starts = rng.integers(0, len(text) - hi - 1, n).astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ch = text[np.repeat(starts - off[:-1], lens) + np.arange(off[-1])].copy()
    a_lo, a_hi = absent_chars(al)
    k = np.arange(0, n, 50)
    k = k[lens[k] > 0]
    where = np.where(rng.random(len(k)) < 0.3, lens[k] - 1, rng.integers(0, 1 << 30, len(k)) % lens[k])
    ch[off[k] + where] = np.where(np.arange(len(k)) % 2 == 0, a_lo, a_hi)
    return ch, off.astype(np.int32)


def _resident(text, **opts):
    with options(suffix_table_image_fraction=0, **opts):  # (only the budget cuts the table: as deep as the key width allows)
        return ia.FmIndex(text, 32, True, device=0)


@pytest.fixture(scope="module", autouse=True)
def _known_options():
    """The library has no getter, and a module that ran earlier in the session may have left an option off its default.  Which
    path a plan takes is asserted here, so every option this module reads is first SET to the value CUR holds for it."""
    for k, v in CUR.items():
        assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
    yield


@pytest.fixture(scope="module")
def world(_known_options):
    w = SimpleNamespace()
    w.ixs = {}
    w.n_max = max(1 << 20, 4096 * n_cu() + 1)
    log = ia.synth_log(1 << 20)
    texts = {"L": log, "B": wide_byte_text(log), "R": workload.reference_text(20)}
    try:
        for name, tname, opts in (("L", "L", {}), ("B", "B", {}), ("R12", "R", {"code_bits_12": 1}), ("R16", "R", {"code_bits_12": 0}),
                                  ("L0", "L", {"suffix_table_mb": 0})):
            # held: the option that has to stay as it was when the index became resident
            ix = SimpleNamespace(name=name, key=name, text=texts[tname], held={"code_bits_12": opts.get("code_bits_12", CUR["code_bits_12"])})
            ix.fm = _resident(ix.text, **opts)
            w.ixs[name] = ix
            ix.al = pm.Alphabet(ix.text)
            assert ix.fm.getAlphabetLength() == ix.al.sigma and ix.fm.getInputLength() == ix.al.text_length
            ix.code_bits = pm.code_bits_for(ix.al.sigma, bool(opts.get("code_bits_12", 1)))
            ix.table_chars = ix.fm.suffix_table_info()[0]
            ix.rows = pm.SaRows(ix.al, ix.text, ix.code_bits)
            ix.tname = tname
        assert w.ixs["L"].al.sigma <= 78 and w.ixs["L"].code_bits == 8  # the order-1 table fits LDS at 4,096 bins
        assert 90 < w.ixs["B"].al.sigma <= 256 and w.ixs["R12"].al.sigma == 1100
        assert (w.ixs["R12"].code_bits, w.ixs["R16"].code_bits) == (12, 16)
        assert w.ixs["L0"].table_chars == 0 and all(w.ixs[k].table_chars >= 2 for k in ("L", "B", "R12", "R16"))
        w.oracles = {t: orc.OracleFmIndex(texts[t], 32, True) for t in texts}
        w.batches = {}
        for seed, (tname, text) in enumerate(texts.items()):
            al = w.ixs[{"L": "L", "B": "B", "R": "R12"}[tname]].al
            rng = np.random.default_rng(100 + seed)
            w.batches[tname, "mixed"] = Batch("mixed 0..31", *make_patterns(text, al, w.n_max, rng, 0, 31))
            w.batches[tname, "len8"] = Batch("length 8", *make_patterns(text, al, 100000, rng, 8, 8))
            w.batches[tname, "skew"] = Batch("mixed 0..31, d_pat half-word aligned", *make_patterns(text, al, 20000, rng, 0, 31),
                                             skew=True)
        # one pattern longer than the length field holds, among ordinary ones
        ch, off = make_patterns(log, w.ixs["L"].al, 4097, np.random.default_rng(7), 0, 31)
        long_len = pm.LONG_PATTERN + 6
        at = 2051
        ch = np.concatenate([ch[:off[at]], np.resize(log, long_len), ch[off[at + 1]:]])
        off = off.astype(np.int64)
        off[at + 1:] += long_len - (off[at + 1] - off[at])
        w.batches["L", "long"] = Batch("one pattern of 0x3fffff + 6 characters", ch, off)
        assert w.batches["L", "long"].m[at] == long_len
        yield w
    finally:
        for ix in w.ixs.values():
            if getattr(ix, "fm", None) is not None:
                ix.fm.close()


def batch(w, ix, kind):
    return w.batches[ix.tname, kind]


# ---- one plan, read back -----------------------------------------------------------------------------------------------------------

def expected_path(ix, n):
    sh = pm.Shape(ix.al.sigma, CUR["sort_bits"], CUR["coarse_bits"], CUR["code_bits_12"], CUR["plan_sa_key"], ix.table_chars > 0,
                  ix.al.text_length)
    fine = CUR["plan_fine"] == 2 or (CUR["plan_fine"] == 1 and not sh.sa_key)
    fused = bool(CUR["plan_fused"]) and not fine and -(-n // pm.TILE) <= n_cu()
    return sh, fine, fused


def plan_call(ix, b, n):
    h = C.c_void_p()
    ok(ia.lib.fmx_count_plan_dev(ix.fm.handle, b.d_ch.data_ptr(), b.d_off.data_ptr(), n, C.byref(h), stream()), "fmx_count_plan_dev")
    return h.value


def what(ix, b, n):
    return "index %s, batch '%s', n = %d, options %r" % (ix.name, b.name, n, {k: v for k, v in CUR.items() if v != LIB_DEFAULTS[k]})


def run_plan(ix, b, n, mark=True):
    """plans the batch's first n patterns under the current options; mark: the by-pattern block is filled with MARK first (one
    plan in front finds the workspace's address), so that the records found there are this plan's"""
    p = SimpleNamespace()
    p.shape, p.fine, p.fused = expected_path(ix, n)
    p.what = what(ix, b, n)
    handle = plan_call(ix, b, n)
    assert handle, "%s: no plan" % p.what
    if mark:
        dev_fill(handle - 16 * n, 16 * n, MARK)
        again = plan_call(ix, b, n)
        assert again == handle, "%s: the workspace moved between two plans of one size" % p.what
    p.handle = handle
    raw = dev_read(handle - 16 * n, 32 * n)
    p.by_pattern = raw[:16 * n].view(REC)
    p.ordered = raw[16 * n:].view(REC)
    p.untouched = bool((raw[:16 * n] == MARK).all()) if mark else None
    return p


def first(mask):
    return int(np.flatnonzero(mask)[0])


def check_plan(ix, b, n, mark=True, keys=None, may_abort=False):
    """(a) (b) (c), (d) where the key is the code key, (e) where k_plan_fine ran; returns the Plan with .a and .K (keys by pattern).
    keys: the keys to take for a fused plan under an SA-row key (a two-kernel run's)"""
    p = run_plan(ix, b, n, mark)
    sh, tag = p.shape, p.what
    words, m = b.words(ix)[:n], b.m[:n]
    a = p.ordered["a"].astype(np.int64)
    p.a = a
    # a. permutation
    srt = np.sort(a)
    bad = srt != np.arange(n)
    assert not bad.any(), "(a) %s: the ordered records are no permutation; sorted a[%d] = %d" % (tag, first(bad), srt[first(bad)])
    # which path ran, and the keys by pattern
    if mark:
        assert p.untouched == p.fused, "(h) %s: by-pattern block %s, but %s was expected to run" % (
            tag, "untouched" if p.untouched else "rewritten", "k_plan_fused" if p.fused else "k_plan_codes + k_plan_scatter")
    model_keys = pm.code_keys(words, sh) if not sh.sa_key else None
    if p.fused:
        K = model_keys if model_keys is not None else keys
        assert K is not None
    else:
        K = p.by_pattern["a"].copy()
        bad = p.by_pattern["cw"] != words
        assert not bad.any(), "(b) %s: k_plan_codes' code word of pattern %d is %#x, model %#x" % (
            tag, first(bad), p.by_pattern["cw"][first(bad)], words[first(bad)])
        want_m = pm.length_field(m) | (pm.fine_bin(K, sh).astype(np.uint32) << 22)
        bad = p.by_pattern["m"] != want_m
        assert not bad.any(), "(b) %s: k_plan_codes' length | fine bin of pattern %d is %#x, want %#x" % (
            tag, first(bad), p.by_pattern["m"][first(bad)], want_m[first(bad)])
        # d. exact keys
        if model_keys is not None:
            bad = K != model_keys
            assert not bad.any(), "(d) %s (shape %r): key of pattern %d is %#x, model %#x" % (
                tag, sh.as_tuple(), first(bad), K[first(bad)], model_keys[first(bad)])
    p.K = K
    aborted = False
    if may_abort and p.fused and (a == np.arange(n)).all():
        aborted = True  # the documented abort of k_plan_fused: the caller's order, with code words
    p.aborted = aborted
    # b. records carry the pattern
    bad = p.ordered["cw"] != words[a]
    assert not bad.any(), "(b) %s: record %d (pattern %d) has code word %#x, model %#x" % (
        tag, first(bad), a[first(bad)], p.ordered["cw"][first(bad)], words[a][first(bad)])
    bad = (p.ordered["m"] & pm.LONG_PATTERN) != pm.length_field(m)[a]
    assert not bad.any(), "(b) %s: record %d (pattern %d) has length field %d, model %d" % (
        tag, first(bad), a[first(bad)], p.ordered["m"][first(bad)] & pm.LONG_PATTERN, pm.length_field(m)[a][first(bad)])
    top = (p.ordered["m"] >> 22).astype(np.int64)
    want_top = np.zeros(n, np.int64) if p.fine else pm.fine_bin(K, sh)[a]
    bad = top != want_top
    assert not bad.any(), "(b) %s: bits 22..31 of record %d are %d, want %d (k_plan_fine %s)" % (
        tag, first(bad), top[first(bad)], want_top[first(bad)], "ran" if p.fine else "did not run")
    if aborted:
        return p
    # c. bucket order.  k_plan_fine then reorders every window of 1,024 by fine bins that hold only the two lowest coarse bits, so
    # behind it the bins are what the bucket order put into each window, as a multiset; the run without it is checked under (e)
    bins = pm.coarse_bin(K, sh)
    along = bins[a]
    hist = np.bincount(bins, minlength=sh.bins)
    want_along = np.repeat(np.arange(sh.bins), hist)
    win = np.arange(n) // pm.FINE_WINDOW
    if p.fine:
        got = along[np.lexsort((along, win))]
        bad = got != want_along
        assert not bad.any(), "(c) %s: window %d holds bin %d where the histogram of the keys puts bin %d" % (
            tag, first(bad) // pm.FINE_WINDOW, got[first(bad)], want_along[first(bad)])
    else:
        bad = along[1:] < along[:-1]
        assert not bad.any(), "(c) %s: bin %d at position %d follows bin %d" % (
            tag, along[first(bad) + 1], first(bad) + 1, along[first(bad)])
        bad = along != want_along
        assert not bad.any(), "(c) %s: position %d holds bin %d, the histogram of the keys puts bin %d there" % (
            tag, first(bad), along[first(bad)], want_along[first(bad)])
    # e. fine order
    if p.fine:
        fine = pm.fine_bin(K, sh)[a]
        bad = (fine[1:] < fine[:-1]) & (np.arange(1, n) % pm.FINE_WINDOW != 0)
        assert not bad.any(), "(e) %s: fine bin %d at position %d follows %d inside one window" % (
            tag, fine[first(bad) + 1], first(bad) + 1, fine[first(bad)])
        # every window holds what the bucket order put there: against a run without the fine pass.  The scatter order inside a
        # bin is not deterministic, so: the bins of a window as a multiset (the check above pins them position by position), and
        # for every bin whose whole run lies inside ONE window the very same patterns in that window
        with options(plan_fine=0):
            q = run_plan(ix, b, n, mark)
        a0 = q.ordered["a"].astype(np.int64)
        assert (np.sort(a0) == np.arange(n)).all(), "(e) %s: the run without the fine pass is no permutation" % tag
        along0 = bins[a0]
        bad = along0 != want_along  # ((c) of the bucket order itself: non-decreasing, every run as long as the histogram says)
        assert not bad.any(), "(c) %s: without the fine pass position %d holds bin %d, not %d" % (
            tag, first(bad), along0[first(bad)], want_along[first(bad)])
        pos1, pos0 = np.empty(n, np.int64), np.empty(n, np.int64)
        pos1[a], pos0[a0] = win, win
        bad = pos1 != pos0  # (a pattern whose bin straddles a window border, or fills several, may sit in either: left out below)
        cum = np.concatenate([[0], np.cumsum(hist)])
        whole = (cum[:-1] // pm.FINE_WINDOW) == ((np.maximum(cum[1:], 1) - 1) // pm.FINE_WINDOW)
        bad &= whole[bins]
        assert not bad.any(), "(e) %s: pattern %d sits in window %d, the bucket order put it in window %d" % (
            tag, first(bad), pos1[first(bad)], pos0[first(bad)])
        # (not vacuous: among 4,096 bins or more some lie inside one window — at coarse_bits 4 the 16 bins span many windows and
        # only the multiset of bins above is compared)
        checked = int(whole[bins].sum())
        assert checked > 0 or sh.coarse_bits < 12, "(e) %s: no bin lies inside one window: nothing compared" % tag
    return p


# ---- the SA-row keys ----------------------------------------------------------------------------------------------------------------

def check_sa_key_1(ix, b, n, p):
    """f. the table's own answer"""
    words, m = b.words(ix)[:n], b.m[:n]
    want = pm.sa_row_keys(ix.al, ix.rows, words, m, ix.table_chars, ix.code_bits)
    # (every string of up to the depth the table reports is tabulated, and `len` is cut at that depth: all are checked exactly,
    # but for the one string that reads as a free slot)
    lens = pm.sa_key_len(m, ix.table_chars, ix.code_bits)
    bits = lens * ix.code_bits
    mask = np.where(bits >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << np.minimum(bits, 63).astype(np.uint64)) - np.uint64(1))
    exact = (words & mask) != np.uint64(0xFFFFFFFFFFFFFFFF)
    share = exact.mean()
    bad = exact & (p.K != want)
    assert not bad.any(), "(f) %s: key of pattern %d (length %d) is %d, the model's first SA row %d; %d of %d patterns checked exactly" % (
        p.what, first(bad), m[first(bad)], p.K[first(bad)], want[first(bad)], exact.sum(), n)
    assert share >= 0.9, "(f) %s: only %d of %d patterns checked exactly" % (p.what, exact.sum(), n)


def check_sa_key_2(ix, b, n, p):
    """g. the estimate from the two-character strings"""
    cb = ix.code_bits
    words, m = b.words(ix)[:n], b.m[:n]
    K = p.K.astype(np.int64)
    C_ = ix.al.C
    tol = int(8 * pm.ulp32(ix.al.text_length) + 1)  # at most 8 float32 accumulations of values bounded by the text length
    lens = pm.sa_key_len(m, ix.table_chars, cb)
    c_last = pm.word_code(words, 0, cb).astype(np.int64)
    dead = (m == 0) | (c_last == 0)
    bad = dead & (K != 0)
    assert not bad.any(), "(g) %s: pattern %d ends at once, its key is %d, not 0" % (p.what, first(bad), K[first(bad)])
    one = ~dead & (lens < 2)
    bad = one & (K != C_[c_last])
    assert not bad.any(), "(g) %s: pattern %d of one character has key %d, C = %d" % (p.what, first(bad), K[first(bad)], C_[c_last][first(bad)])
    two = ~dead & (lens >= 2)
    L = np.where(two, lens, 2)
    x = np.where(two, pm.word_code(words >> ((L - 1) * cb).astype(np.uint64), 0, cb), 0).astype(np.int64)
    y = np.where(two, pm.word_code(words >> ((L - 2) * cb).astype(np.uint64), 0, cb), 0).astype(np.int64)
    xy = (y.astype(np.uint64) | (x.astype(np.uint64) << np.uint64(cb)))
    s2, e2 = ix.rows.ranges_of_words(xy, np.full(n, 2))
    occurs = two & (e2 > s2)
    # no first character to start from: the search starts at the last character's rows; no second one, or a pair the text does
    # not hold: at the first character's
    bad = two & (x == 0) & (K != C_[c_last])
    assert not bad.any(), "(g) %s: pattern %d (absent first character of the suffix) has key %d, C[last] = %d" % (
        p.what, first(bad), K[first(bad)], C_[c_last][first(bad)])
    bad = two & (x != 0) & ~occurs & (K != C_[x])
    assert not bad.any(), "(g) %s: pattern %d (no such pair) has key %d, C[first] = %d" % (p.what, first(bad), K[first(bad)], C_[x][first(bad)])
    bad = occurs & ((K < s2 - tol) | (K > e2 + tol))
    assert not bad.any(), "(g) %s: key %d of pattern %d lies outside the rows [%d, %d) of its first two characters (tolerance %d)" % (
        p.what, K[first(bad)], first(bad), s2[first(bad)], e2[first(bad)], tol)
    bad = occurs & (lens == 2) & (np.abs(K - s2) > 1)
    assert not bad.any(), "(g) %s: pattern %d, suffix of two characters: key %d, first row %d" % (p.what, first(bad), K[first(bad)], s2[first(bad)])
    # monotone over the distinct suffixes in lexicographic order of their codes (first character first, a prefix before its
    # extensions) — over EVERY pattern that has a search to start.  Taken literally the claim does not hold for a suffix whose
    # first character is absent: by its codes it sorts in front of all others, while its key is C[last character] (asserted
    # above), anywhere up to the text length.  plan_record's comment states that exception — such a suffix is keyed, and so
    # ordered, as its last character alone — and that is how it takes part here: as the one-character string of that character.
    sel = np.flatnonzero(~dead)
    if len(sel) == 0:
        return
    depth = 64 // cb
    ln = np.where(two & (x == 0), 1, lens)[sel]
    bits = ln * cb
    mask = np.where(bits >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << np.minimum(bits, 63).astype(np.uint64)) - np.uint64(1))
    lead = (words[sel] & mask) << ((depth - ln) * cb).astype(np.uint64)
    order = np.lexsort((ln, lead))
    lead, ln, k = lead[order], ln[order], K[sel][order]
    new = np.concatenate([[True], (lead[1:] != lead[:-1]) | (ln[1:] != ln[:-1])])
    same = ~new[1:] & (k[1:] != k[:-1])
    assert not same.any(), "(g) %s: two patterns with one suffix have keys %d and %d" % (p.what, k[:-1][first(same)], k[1:][first(same)])
    k = k[new]
    drop = np.maximum.accumulate(k) - k
    bad = drop > tol
    assert not bad.any(), "(g) %s: the estimate is not monotone: distinct suffix %d of %d has key %d after a key of %d (tolerance %d)" % (
        p.what, first(bad), len(k), k[first(bad)], np.maximum.accumulate(k)[first(bad)], tol)
    assert n < 1000 or occurs.mean() > 0.8, p.what  # (the bounds above were not vacuous)


def check_all(ix, b, n, **kw):
    p = check_plan(ix, b, n, **kw)
    if not p.fused and p.shape.sa_key == 1:
        check_sa_key_1(ix, b, n, p)
    if not p.fused and p.shape.sa_key == 2:
        check_sa_key_2(ix, b, n, p)
    return p


INDEXES = ["L", "B", "R12", "R16", "L0"]


# ---- the tests ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", INDEXES)
def test_order_at_every_size(world, name):
    """(a)-(g) at n = 1 .. 1,048,576 under each of the three keys, mixed lengths 0..31 with absent characters"""
    ix = world.ixs[name]
    b = batch(world, ix, "mixed")
    with options(**ix.held):
        assert plan_call(ix, b, 4097) is None, "a batch below sort_min is not planned: the handle is NULL"
        assert plan_call(ix, b, 16384), "a batch of sort_min patterns is planned"
        with options(sort_min=1):
            for sa_key in (0, 1, 2):
                with options(plan_sa_key=sa_key):
                    for n in SIZES:
                        p = check_all(ix, b, n)
                        assert p.shape.sa_key == (sa_key if ix.table_chars else 0) and not p.fused
                        assert p.fine == (p.shape.sa_key == 0)


@pytest.mark.parametrize("name", INDEXES)
def test_exact_keys_at_every_shape(world, name):
    """(d) with (a)-(c), (e): sort_bits 1 / 9 / 28 / 32 x coarse_bits 4 / 12 / 13 under the code key — total_bits < coarse_bits
    among them — and plan_fine 0 / 2 under every key (2: the fine pass over SA-row keys)"""
    ix = world.ixs[name]
    b = batch(world, ix, "mixed")
    n = 20000
    with options(sort_min=1, **ix.held):
        narrow = 0
        with options(plan_sa_key=0):
            for sort_bits in (1, 9, 28, 32):
                for coarse_bits in (4, 12, 13):
                    with options(sort_bits=sort_bits, coarse_bits=coarse_bits):
                        p = check_all(ix, b, n)
                        assert p.shape.sa_key == 0 and p.fine
                        narrow += p.shape.total_bits < coarse_bits
        assert narrow >= 2
        for sa_key in (0, 1, 2):
            for fine in (0, 2):
                for coarse_bits in (4, 12, 13):
                    with options(plan_sa_key=sa_key, plan_fine=fine, coarse_bits=coarse_bits):
                        p = check_all(ix, b, n)
                        assert p.fine == (fine == 2)


@pytest.mark.parametrize("name", INDEXES)
def test_order_of_other_batches(world, name):
    """one length of 8 (pattern_tail_load's dwords at every alignment), a d_pat that is half-word but not dword aligned, and — on
    the log index — a pattern longer than the length field holds"""
    ix = world.ixs[name]
    kinds = ["len8", "skew"] + (["long"] if name == "L" else [])
    with options(sort_min=1, **ix.held):
        for kind in kinds:
            b = batch(world, ix, kind)
            for sa_key in (0, 1, 2):
                with options(plan_sa_key=sa_key):
                    p = check_all(ix, b, b.n)
                    if kind == "long":
                        i = first(b.m > pm.LONG_PATTERN)
                        at = first(p.a == i)
                        assert p.ordered["m"][at] & pm.LONG_PATTERN == pm.LONG_PATTERN and (b.m <= pm.LONG_PATTERN).sum() == b.n - 1


@pytest.mark.parametrize("name", INDEXES)
def test_fused_kernel(world, name):
    """h. k_plan_fused: the same order as the two kernels at the default spin limit; at plan_spin_limit 0 that or its documented
    abort; above one tile per CU the two kernels run"""
    ix = world.ixs[name]
    b = batch(world, ix, "mixed")
    n_top = pm.TILE * n_cu()  # the largest batch of one tile per CU
    assert n_top + 1 <= b.n
    with options(sort_min=1, **ix.held):
        for sa_key in ((0, 1, 2) if ix.table_chars else (0,)):  # (without a table every key is the code key)
            # (the fused kernel is not used when a fine pass follows: under the code key plan_fine goes to 0)
            with options(plan_sa_key=sa_key, plan_fine=0 if (sa_key == 0 or not ix.table_chars) else 1):
                for n in (1, 4097, 100000, n_top):
                    two = check_all(ix, b, n)
                    assert not two.fused
                    with options(plan_fused=1):
                        p = check_plan(ix, b, n, keys=two.K)
                        assert p.fused and not p.aborted
                        if n in (100000, n_top):
                            with options(plan_spin_limit=0):
                                p = check_plan(ix, b, n, keys=two.K, may_abort=True)
                                assert p.fused
                with options(plan_fused=1):
                    p = check_all(ix, b, n_top + 1)
                    assert not p.fused  # (the by-pattern keys were there: check_plan's path assertion)


def test_the_head_is_left_clean(world):
    """i. plans back to back on one stream, nothing in between: the last one finds histogram, cursors and ticket zeroed"""
    ix = world.ixs["L"]
    A, B = batch(world, ix, "mixed"), batch(world, ix, "len8")
    with options(sort_min=1):
        for sa_key in (0, 2):
            with options(plan_sa_key=sa_key):
                plan_call(ix, A, 100000)
                plan_call(ix, B, 4097)
                check_all(ix, A, 100000, mark=False)
                # a histogram of 8,192 bins must not leak into 16
                with options(coarse_bits=13):
                    plan_call(ix, A, 100000)
                with options(coarse_bits=4):
                    check_all(ix, A, 100000, mark=False)
                with options(coarse_bits=13):
                    check_all(ix, A, 100000, mark=False)
                # fused, then the two kernels — and the other way round
                with options(plan_fine=0):
                    two = check_all(ix, A, 100000, mark=False)
                    with options(plan_fused=1):
                        plan_call(ix, A, 100000)
                    check_all(ix, B, 4097, mark=False)
                    check_all(ix, A, 100000, mark=False)
                    with options(plan_fused=1):
                        check_plan(ix, A, 100000, mark=False, keys=two.K)
                        plan_call(ix, B, 4097)
                        check_plan(ix, A, 100000, mark=False, keys=two.K)


@pytest.mark.parametrize("name", INDEXES)
def test_consumers_agree(world, name):
    """j. fmx_count_ordered_dev over the plan just checked, outputs prefilled with a sentinel, against the oracle"""
    torch = _torch()
    ix = world.ixs[name]
    o = world.oracles[ix.tname]
    for kind in ["mixed"] + (["long"] if name == "L" else []):
        b = batch(world, ix, kind)
        n = min(b.n, 100000)
        exp = o.count_batch(b.ch[:b.off[n]], b.off[:n + 1], threads=THREADS)
        with options(sort_min=1, **ix.held):
            p = check_all(ix, b, n)
            handle = plan_call(ix, b, n)  # (check_all may have planned once more without the fine pass: the stream's live plan)
            assert handle == p.handle
            cnt, st = (torch.full((n,), SENT, dtype=torch.int32, device="cuda") for _ in range(2))
            ok(ia.lib.fmx_count_ordered_dev(ix.fm.handle, b.d_ch.data_ptr(), b.d_off.data_ptr(), p.handle, n, cnt.data_ptr(), None,
                                            st.data_ptr(), stream()), "fmx_count_ordered_dev")
            torch.cuda.synchronize()
            cnt, st = cnt.cpu().numpy(), st.cpu().numpy()
        bad = (cnt != exp[0]) | (st != exp[1])
        assert not bad.any(), "(j) %s: pattern %d counts %d / status %d, the oracle %d / %d" % (
            p.what, first(bad), cnt[first(bad)], st[first(bad)], exp[0][first(bad)], exp[1][first(bad)])

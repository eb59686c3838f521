"""The row table of a resident FmIndex (option "locate_rows"; index4j_amd/csrc/fmx_device.hpp DevIndex.rows) on the CPU: the
functions k_rows_fill and k_locate_rows run — fm_row_word, fm_locate_share, fm_rows_hit, fm_rows_gather — compiled for the host
(tests/rows_hostsim.cpp) against the oracle, which is the judge of every position, found count, status and LF-step total.
The GPU suite runs the kernels themselves (tests/test_gpu_locate_rows.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HD = hdfs_text()
REPLAY = 0x80000000
_SIM = {}


def sim_lib(tmpdir, compact=False):
    if compact not in _SIM:
        so = os.path.join(str(tmpdir), "librowshostsim%s.so" % ("_compact" if compact else ""))
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared"] + (["-DFMX_COMPACT=1"] if compact else []) +
                              ["-o", so, os.path.join(HERE, "rows_hostsim.cpp")])
        L = C.CDLL(so)
        L.sim_rows_fill.restype = C.c_int64
        L.sim_win_attach.restype = C.c_int64
        L.sim_set_entry_bytes.argtypes = [C.c_int]
        L.sim_rows_size.restype = C.c_int64
        _SIM[compact] = L
    return _SIM[compact]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("rows_hostsim")


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class RowsSim:
    """the host image of an index, its window directory (any form) and its row table, through tests/rows_hostsim.cpp"""

    def __init__(self, simdir, text, sr, extract=True, compact=False):
        if compact:
            assert ia.lib.fmx_set_option(b"image_compact", 1) == 0
        try:
            self.fm = ia.FmIndex(text, sr, extract, device=None)
            self.blob = self.fm.blob()
        finally:
            ia.lib.fmx_set_option(b"image_compact", 0)
        self.L = sim_lib(simdir, compact)
        self.p = C.c_void_p(self.blob.ctypes.data)
        self.n = int(self.L.sim_rows_size(self.p))  # wt_size: one BWT row per character of the indexed text
        self.attached = False

    def directory(self, form):
        """None: the tree alone; 4 / 6: cells with entries of that many bytes; -1: the flat form"""
        if self.attached:
            self.L.sim_win_detach(self.p)
            self.attached = False
        if form is not None:
            self.L.sim_set_entry_bytes(int(form))
            try:
                self.L.sim_win_attach(self.p, None)
            finally:
                self.L.sim_set_entry_bytes(0)
            self.attached = True

    def __del__(self):
        try:
            if self.attached:
                self.L.sim_win_detach(self.p)
        except Exception:  # noqa: BLE001
            pass

    def fill(self):
        rows = np.full(self.n, 0xDEADBEEF, np.uint32)
        replay = self.L.sim_rows_fill(self.p, ptr(rows))
        assert replay == int((rows >> 31).sum())
        return rows, int(replay)

    def walk_all(self):
        at, dist, st = (np.zeros(self.n, np.int32) for _ in range(3))
        self.L.sim_row_walk_all(self.p, ptr(at), ptr(dist), ptr(st))
        return at, dist, st

    def count(self, ch, off):
        n = len(off) - 1
        counts, lf, st, rng = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2 * n, np.int32)
        self.L.sim_count(self.p, ptr(np.ascontiguousarray(ch, np.uint16)), ptr(np.ascontiguousarray(off, np.int32)), n, ptr(counts), ptr(lf),
                         ptr(st), ptr(rng))
        return counts, st, lf, rng

    def locate(self, rows, ch, off, mm, cap, order=None, fill=-7):
        """locate_batch through the table: the count phase, then k_locate_rows' mirror"""
        counts, st, lf, rng = self.count(ch, off)
        n = len(counts)
        locs = np.full((n, max(cap, 0)), fill, np.int32)
        found = np.full(n, fill, np.int32)
        self.L.sim_locate_rows(self.p, ptr(rows), ptr(rng), n, int(mm), ptr(locs), int(cap), ptr(found), ptr(lf), ptr(st), None,
                               ptr(order), None, C.c_int64(0))
        return locs, found, st, lf, rng


def oracle_rows(ref, sim, t16):
    """(value, symbol) the oracle's locate gives for every BWT row but the sentinel's: the rows of symbol c are C[c] .. C[c + 1], in
    the order locate stores them (FM:526-548), so locating every single-symbol pattern without a limit lists them all"""
    syms = np.unique(t16)
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in syms])
    counts, st, lf, rng = sim.count(ch, off)
    want = np.full(sim.n, -1, np.int64)
    sym_of = np.full(sim.n, -1, np.int64)
    steps = {}
    for i, s in enumerate(syms):
        orc.counters_reset()
        n, l = ref.locate(np.array([s], np.uint16), max_matches=-1, cap=int(counts[i]) + 1)
        steps[int(s)] = orc.counters()["lf_steps"]
        assert n == counts[i]
        start = int(rng[2 * i])
        want[start:start + n] = l
        sym_of[start:start + n] = int(s)
    return want, sym_of, syms, steps


def check_table_against_oracle(sim, rows, ref, t16, sr):
    """every clean word = the oracle's value for its row, and value % sampleRate = the walk's distance; returns what is needed for
    the quirk assertions: (oracle values, symbols, clean mask)"""
    want, sym_of, syms, steps = oracle_rows(ref, sim, t16)
    at, dist, st = sim.walk_all()
    known = want >= 0
    assert int(known.sum()) >= sim.n - 1  # all rows but the sentinel's
    clean = (rows >> 31) == 0
    assert (rows[clean & known].astype(np.int64) == want[clean & known]).all()
    assert (rows[clean].astype(np.int64) % sr == dist[clean]).all() and (st[clean] == 0).all()
    # a row is marked "replay" only where a word cannot carry the answer
    need = (st != 0) | (dist != at.astype(np.int64) % sr) | (at < 0)
    assert (need == ~clean).all()
    return want, sym_of, syms, steps, clean


def check_locate_against_oracle(sim, rows, ref, pats, shapes, with_order=True):
    ch, off = ia.pack_patterns(pats)
    for mm, cap in shapes:
        for order_on in ((False, True) if with_order else (False,)):
            order = None
            if order_on:  # the walk-order stage's records {start, end, pattern, -} by the first row of the ranges
                _, _, _, rng = sim.count(ch, off)
                by = np.argsort(rng[0::2], kind="stable")
                order = np.zeros((len(pats), 4), np.int32)
                order[:, 0], order[:, 1], order[:, 2] = rng[0::2][by], rng[1::2][by], by
            locs, found, st, lf, _ = sim.locate(rows, ch, off, mm, cap, order=order)
            for i, p in enumerate(pats):
                orc.counters_reset()
                try:
                    n, l = ref.locate(p, max_matches=mm, cap=cap)
                    assert st[i] == 0 and n == found[i] and (l == locs[i, :n]).all(), (i, mm, cap)
                    assert (locs[i, n:] == -7).all()  # nothing stored beyond the hits
                    assert lf[i] == orc.counters()["lf_steps"], (i, mm, cap)
                except IndexError:  # more hits wanted than `locations` holds (Java AIOOBE): the first loc_cap are stored
                    assert st[i] == 9 and found[i] == cap
                    n, l = ref.locate(p, max_matches=cap, cap=cap)
                    assert (l == locs[i, :n]).all()


def sample_patterns(t16, rnd, n_q):
    L = len(t16)
    pats = [t16[s:s + int(rnd.integers(1, 12))] for s in rnd.integers(0, max(1, L - 12), n_q)]
    pats += [t16[s:s + 1] for s in rnd.integers(0, L, 6)]  # single symbols: many hits
    pats += [ia.as_chars("zzzzqq"), t16[:1], np.array([np.bincount(t16).argmax()], np.uint16)]  # (+ the symbol with the most hits)
    return pats


KATS = ["This is a long string\0", "This \0is a \0long string\0", "abracadabra abracadabra abracadabra\0", "a" * 300 + "b" * 40 + "\n"]
SYNTH = ia.synth_log(1 << 15, seed=11)


@pytest.mark.parametrize("sr", [1, 4, 32, 6])
@pytest.mark.parametrize("extract", [True, False])
def test_table_and_gather_equal_the_oracle(simdir, sr, extract):
    rnd = np.random.default_rng(1000 + sr)
    texts = KATS + [HD[:40_000] if extract else HD[40_000:70_000], SYNTH]
    for text in texts:
        t16 = ia.as_chars(text)
        sim = RowsSim(simdir, text, sr, extract)
        ref = orc.OracleFmIndex(text, sr, extract)
        rows, replay = sim.fill()
        check_table_against_oracle(sim, rows, ref, t16, sr)
        pats = sample_patterns(t16, rnd, 40)
        most = int(np.bincount(t16).max())
        assert most > 3  # (-1, 3) and (16, 2) below: a `locations` array smaller than the hit count
        check_locate_against_oracle(sim, rows, ref, pats, ((1, 1), (16, 16), (-1, most + 5), (-1, 3), (16, 2), (100, 70)))


def test_fixture_whole_at_both_rates_has_no_replay_rows(simdir):
    """the reference's fixture (2,061 symbols): no walk raises a status or leaves value % sampleRate, so no row may be marked —
    a fill that marks rows without need hides the table from every other test"""
    t16 = ia.as_chars(HD)
    for sr in (32, 6):
        sim = RowsSim(simdir, HD, sr)
        ref = orc.OracleFmIndex(HD, sr, True)
        rows, replay = sim.fill()
        check_table_against_oracle(sim, rows, ref, t16, sr)
        assert replay == 0
        check_locate_against_oracle(sim, rows, ref, sample_patterns(t16, np.random.default_rng(sr), 60), ((16, 16), (-1, 40)), with_order=False)


@pytest.mark.parametrize("case", ["log32", "log6", "multichar8"])
def test_clean_texts_have_no_replay_rows(simdir, case):
    text, sr = {"log32": (ia.synth_log(1 << 18), 32), "log6": (ia.synth_log(1 << 18), 6),
                "multichar8": (ia.synth_log_multichar(1 << 19, 600), 8)}[case]
    sim = RowsSim(simdir, text, sr)
    sim.directory(-1)  # (the flat directory: the fill is then a step per sector, as on a resident index; test 3 pins that the form is free)
    rows, replay = sim.fill()
    assert replay == 0
    ref = orc.OracleFmIndex(text, sr, True)
    check_locate_against_oracle(sim, rows, ref, sample_patterns(ia.as_chars(text), np.random.default_rng(3), 40), ((16, 16), (-1, 50)),
                                with_order=False)


def run_block_text():
    """the text of tests/test_window_cells.py::test_large_alphabet_with_run_blocks_of_wide_symbols, from its seed: symbols >= 256 in
    run blocks (quirk Q1: inverseSelect reports them masked to 8 bits, WFBB:1332) over a 900-symbol alphabet"""
    rng = np.random.default_rng(9)
    parts = []
    for i in range(12):
        parts.append("".join(chr(0x4E00 + int(x) * 7) for x in rng.integers(0, 900, 1500)))
        parts.append(chr(0x30A1 + i) * 70_000)
        parts.append("log line %d\n" % i * 50)
    return "".join(parts)


@pytest.mark.parametrize("sr", [16, 5])
def test_quirk_rows_hold_what_the_reference_returns(simdir, sr):
    """Derailed walks: the reference returns positions where the text does NOT hold the pattern's symbol (a table made from a true
    suffix array would differ on 39-46 % of the rows), and some walks take a number of steps other than value % sampleRate.
    Every word, and every replayed hit, must equal the oracle; rows are marked only where needed; and the table itself — not the
    replay — serves derailed rows."""
    text = run_block_text()
    t16 = ia.as_chars(text)
    sim = RowsSim(simdir, text, sr)
    ref = orc.OracleFmIndex(text, sr, True)
    sim.directory(-1)
    rows, replay = sim.fill()
    want, sym_of, syms, steps, clean = check_table_against_oracle(sim, rows, ref, t16, sr)
    assert 0 < replay < sim.n
    known = want >= 0
    served = clean & known
    wrong_symbol = np.zeros(sim.n, bool)
    inside = known & (want < len(t16))
    wrong_symbol[inside] = t16[want[inside]] != sym_of[inside]
    wrong_symbol |= known & (want >= len(t16))
    assert int(wrong_symbol.sum()) > sim.n // 4            # the reference's derailed answers (measured: 39 % / 46 %)
    assert int((wrong_symbol & served).sum()) > 0          # ... served from the table, bit 31 clear
    # every single-symbol pattern without a limit (all rows but the sentinel's): words and replayed hits against the oracle
    ch, off = ia.pack_patterns([np.array([s], np.uint16) for s in syms])
    most = int(np.bincount(t16).max())
    locs, found, st, lf, rng = sim.locate(rows, ch, off, -1, most)
    differ = 0
    for i, s in enumerate(syms):
        start, n = int(rng[2 * i]), int(found[i])
        assert st[i] == 0 and (locs[i, :n] == want[start:start + n]).all(), int(s)
        assert lf[i] == steps[int(s)], int(s)
        differ += int(steps[int(s)] != int((want[start:start + n] % sr).sum()))
    assert differ > 0  # patterns whose LF-step total the values alone would get wrong (measured: 6 / 5): what the replay mark is for
    check_locate_against_oracle(sim, rows, ref, sample_patterns(t16, np.random.default_rng(sr), 40), ((1, 1), (16, 16), (-1, 30), (100, 70)))


@pytest.mark.parametrize("case", ["fixture", "runblocks", "compact", "reference_route"])
def test_fill_is_the_same_over_tree_and_every_directory_form(simdir, case):
    import hostsim

    if case == "fixture":
        sim = RowsSim(simdir, HD[:60_000], 32)
    elif case == "runblocks":
        sim = RowsSim(simdir, run_block_text()[:440_000], 16)
    elif case == "compact":
        sim = RowsSim(simdir, HD[:40_000], 8, compact=True)
    else:
        sim = RowsSim(simdir, HD[:30_000], 8)
        sim.fm = hostsim.reference_route_index(HD[:30_000], 8)
        sim.blob = sim.fm.blob()
        sim.p = C.c_void_p(sim.blob.ctypes.data)
    tree, replay = sim.fill()
    if case == "runblocks":
        assert 0 < replay < sim.n
    for form in (4, 6, -1):
        sim.directory(form)
        other, replay2 = sim.fill()
        assert replay2 == replay and other.tobytes() == tree.tobytes(), (case, form)
    sim.directory(None)


def test_rows_outside_the_table_and_marked_rows_are_walked(simdir):
    """ranges as a count phase over a damaged image may hand them back: the gather never indexes the table with such a row, and
    answers as the walk does (status 9 for rows the bitmap does not have)"""
    text = HD[:20_000]
    sim = RowsSim(simdir, text, 4)
    rows, _ = sim.fill()
    n = sim.n
    rng = np.array([n - 3, n + 4, -5, 2, 0x7FFFFFF0, 0x7FFFFFF8, 5, 9, n, n + 2], np.int32)
    marked = rows.copy()
    marked[5:9] = REPLAY | 0x1234  # (a marked word's low bits are ignored)
    out = []
    for table in (rows, marked):
        locs, found, lf, st = np.full((5, 8), -7, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32)
        sim.L.sim_locate_rows(sim.p, ptr(table), ptr(rng), 5, -1, ptr(locs), 8, ptr(found), ptr(lf), ptr(st), None, None, None, C.c_int64(0))
        walk = np.full((5, 8), -7, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32)
        sim.L.sim_locate_walk(sim.p, ptr(rng), 5, -1, ptr(walk[0]), 8, ptr(walk[1]), ptr(walk[2]), ptr(walk[3]), None, None, None, None,
                              C.c_int64(0))
        assert (locs == walk[0]).all() and (found == walk[1]).all() and (lf == walk[2]).all() and (st == walk[3]).all()
        out.append(locs)
    assert (out[0] == out[1]).all() and st[0] == 9 and st[3] == 0


def test_segment_stores_carry_taken_and_base(simdir):
    text = HD[:20_000]
    sim = RowsSim(simdir, text, 8)
    rows, _ = sim.fill()
    ref = orc.OracleFmIndex(text, 8, True)
    pats = [ia.as_chars(p) for p in ("blk_", "INFO", "dfs", "nothing here")]
    ch, off = ia.pack_patterns(pats)
    counts, st, lf, rng = sim.count(ch, off)
    taken = np.array([2, 10, 0, 0], np.int32)
    cap = 10
    set_locs = np.full((4, cap), -7, np.int64)
    found = np.zeros(4, np.int32)
    sim.L.sim_locate_rows(sim.p, ptr(rows), ptr(rng), 4, cap, None, cap, ptr(found), ptr(lf), ptr(st), ptr(taken), None, ptr(set_locs),
                          C.c_int64(1 << 33))
    for i, p in enumerate(pats):
        left = cap - int(taken[i])
        n, l = ref.locate(p, max_matches=left, cap=cap) if left > 0 else (0, np.zeros(0, np.int32))
        assert found[i] == n and (set_locs[i, taken[i]:taken[i] + n] == l.astype(np.int64) + (1 << 33)).all()
        assert (set_locs[i, :taken[i]] == -7).all() and (set_locs[i, taken[i] + n:] == -7).all()


# THE TICKET (fmx_device.hpp fm_ticket_*, fm_locate_slots, fm_walk_lanes, fm_rows_lanes_log2): what k_locate_walk, k_locate_walk_c,
# k_locate_walk_q and k_locate_rows make of ticket t — run here by sim_locate_walk and sim_locate_rows over one small index, at
# sample rates 1 and 8, over the tree (fm_locate_hit<kWinNever>) and over a window directory (fm_locate_hit<kWinAlways> at rate 1,
# the instalment walk at rate 8).
TICKET_TEXT = HD[:6_000]
TICKET_ROUTES = [(1, None), (1, 4), (8, None), (8, 4)]
_TICKET = {}


class TicketSim:
    """an index over `text`, its patterns' ranges and count-phase results, and the oracle's locate() per shape, each made once"""

    def __init__(self, simdir, text, sr, form, pats):
        self.sim = RowsSim(simdir, text, sr)
        self.sim.directory(form)
        self.rows, _ = self.sim.fill()
        self.ref = orc.OracleFmIndex(text, sr, True)
        self.pats = pats
        ch, off = ia.pack_patterns(pats)
        self.counts, self.st0, self.lf0, rng = self.sim.count(ch, off)
        self.rng = rng.reshape(-1, 2)
        self._oracle = {}

    def oracle(self, mm, cap):
        """per pattern (found, positions, LF-steps of the whole locate() or None, status) as check_locate_against_oracle reads them"""
        if (mm, cap) not in self._oracle:
            out = []
            for p in self.pats:
                orc.counters_reset()
                try:
                    n, l = self.ref.locate(p, max_matches=mm, cap=cap)
                    out.append((n, l, orc.counters()["lf_steps"], 0))
                except IndexError:  # more hits wanted than `locations` holds (Java AIOOBE): the first loc_cap are stored
                    n, l = self.ref.locate(p, max_matches=cap, cap=cap)
                    out.append((cap, l, None, 9))
            self._oracle[(mm, cap)] = out
        return self._oracle[(mm, cap)]

    def walk(self, which, mm, cap, order=None, order_idle=0, taken=None, set_locs=None, set_base=0, rows=False):
        """sim_locate_walk (or sim_locate_rows) over patterns `which` (indices into self.pats, the caller's order of this call);
        returns (locs, found, status, LF-steps, lanes per pattern)"""
        which = np.asarray(which)
        n = len(which)
        rng = np.ascontiguousarray(self.rng[which])
        lf, st = self.lf0[which].copy(), self.st0[which].copy()
        locs, found = np.full((n, max(cap, 0)), -7, np.int32), np.full(n, -7, np.int32)
        if rows:
            lanes = self.sim.L.sim_locate_rows(self.sim.p, ptr(self.rows), ptr(rng), n, int(mm), ptr(locs), int(cap), ptr(found), ptr(lf),
                                               ptr(st), ptr(taken), ptr(order), ptr(set_locs), C.c_int64(set_base))
        else:
            idle = np.array([order_idle], np.uint32)
            lanes = self.sim.L.sim_locate_walk(self.sim.p, ptr(rng), n, int(mm), ptr(locs), int(cap), ptr(found), ptr(lf), ptr(st),
                                               ptr(taken), ptr(order), ptr(idle) if order is not None else None, ptr(set_locs),
                                               C.c_int64(set_base))
        return locs, found, st, lf, lanes

    def check(self, which, mm, cap, got):
        locs, found, st, lf, _ = got
        want = self.oracle(mm, cap)
        for i, j in enumerate(which):
            n, l, steps, status = want[j]
            assert st[i] == status and found[i] == n and (locs[i, :n] == l[:n]).all(), (i, j, mm, cap)
            assert (locs[i, n:] == -7).all()  # nothing stored beyond the hits
            assert steps is None or lf[i] == steps, (i, j, mm, cap)


def ticket_sim(simdir, sr, form):
    if (sr, form) not in _TICKET:
        t16 = ia.as_chars(TICKET_TEXT)
        pats = sample_patterns(t16, np.random.default_rng(77), 30)
        _TICKET[(sr, form)] = TicketSim(simdir, TICKET_TEXT, sr, form, pats)
    return _TICKET[(sr, form)]


@pytest.mark.parametrize("sr,form", TICKET_ROUTES)
def test_walk_order_with_an_idle_prefix(simdir, sr, form):
    """Records sorted by `start`, the patterns with nothing to locate first, *order_idle = their count: the walk kernels give WHOLE
    windows of kFineWindow such records one lane each and every other record `lanes` lanes.  A prefix of 0 windows (0, 1,
    kFineWindow - 1 idle records), of exactly one (kFineWindow, kFineWindow + 1) and of two with a remainder (2 kFineWindow + 3)."""
    ts = ticket_sim(simdir, sr, form)
    window = int(ts.sim.L.sim_fine_window())
    assert window == 1024
    hit = np.flatnonzero(ts.rng[:, 0] < ts.rng[:, 1])
    none = np.flatnonzero(ts.rng[:, 0] >= ts.rng[:, 1])
    assert len(hit) > 20 and len(none) >= 1
    mm, cap = 5, 8  # five lanes per pattern: ticket -> record is a division, not a shift
    rnd = np.random.default_rng(5)
    for n_idle in (0, 1, window - 1, window, window + 1, 2 * window + 3):
        which = np.concatenate([hit, none[rnd.integers(0, len(none), n_idle)]])
        which = which[rnd.permutation(len(which))]  # the caller's order: idle patterns anywhere
        start, end = ts.rng[which, 0], ts.rng[which, 1]
        idle = np.flatnonzero(start >= end)
        busy = np.flatnonzero(start < end)
        by = np.concatenate([idle, busy[np.argsort(start[busy], kind="stable")]])
        order = np.zeros((len(which), 4), np.int32)
        order[:, 0], order[:, 1], order[:, 2] = start[by], end[by], by
        assert len(idle) == n_idle
        plain = ts.walk(which, mm, cap)
        ordered = ts.walk(which, mm, cap, order=order, order_idle=n_idle)
        assert plain[4] == ordered[4] == 5
        for a, b in zip(plain[:4], ordered[:4]):
            assert (a == b).all(), n_idle
        ts.check(which, mm, cap, ordered)


@pytest.mark.parametrize("sr,form", TICKET_ROUTES)
def test_slots_up_to_and_beyond_the_walk_lanes(simdir, sr, form):
    """slots = maxMatches where it is positive and below the capacity, else the capacity, at least 1; a pattern gets
    min(slots, kWalkLanes) lanes and lane g walks hits g, g + lanes, ...: 1 and 2 lanes, kWalkLanes - 1, kWalkLanes itself, and
    one slot more than lanes.  (-1, 128): every pattern with more than 128 hits, and no other, raises the reference's AIOOBE."""
    ts = ticket_sim(simdir, sr, form)
    cap_lanes = int(ts.sim.L.sim_walk_lanes())
    assert cap_lanes == 128
    assert int(ts.counts.max()) > 2 * cap_lanes  # a pattern whose lanes take a second and a third hit each
    which = np.arange(len(ts.pats))
    for slots, (mm, cap) in ((1, (1, 1)), (2, (2, 5)), (127, (127, 200)), (128, (-1, 128)), (129, (129, 129))):
        got = ts.walk(which, mm, cap)
        assert got[4] == min(slots, cap_lanes), (mm, cap)
        ts.check(which, mm, cap, got)
        if mm == -1:
            over = ts.counts > cap
            assert over.any() and not over.all()
            assert ((got[2] == 9) == over).all() and (got[2][~over] == 0).all()
        via_rows = ts.walk(which, mm, cap, rows=True)  # the gather: the same share, publish and stores
        assert via_rows[4] == min(1 << (slots - 1).bit_length(), 64)
        for a, b in zip(got[:4], via_rows[:4]):
            assert (a == b).all(), (mm, cap)


@pytest.mark.parametrize("sr,form", TICKET_ROUTES)
def test_two_segments_of_a_set_share_one_row(simdir, sr, form):
    """Segment 0, then segment 1 with taken = segment 0's `found`, both into one set_locs: maxMatches less what segment 0 took.
    Patterns that segment 0 exhausts (limit <= 0 in segment 1), that segment 1 cuts in the middle, and that neither cuts."""
    texts = (TICKET_TEXT, HD[6_000:12_000])
    t16 = ia.as_chars(texts[0])
    pats = sample_patterns(t16, np.random.default_rng(78), 30) + [ia.as_chars(p) for p in ("blk_", "INFO", "dfs", "Receiving")]
    key = ("set", sr, form)
    if key not in _TICKET:
        _TICKET[key] = [TicketSim(simdir, text, sr, form, pats) for text in texts]
    segs = _TICKET[key]
    mm = cap = 10  # (a set's rows hold maxMatches slots)
    c0, c1 = segs[0].counts.astype(np.int64), segs[1].counts.astype(np.int64)
    exhausted, cut, untouched = c0 >= mm, (c0 > 0) & (c0 < mm) & (c0 + c1 > mm), (c0 > 0) & (c1 > 0) & (c0 + c1 < mm)
    assert exhausted.any() and cut.any() and untouched.any()
    which = np.arange(len(pats))
    bases = (0, 1 << 33)
    runs = []
    for rows in (False, True):
        set_locs = np.full((len(pats), cap), -7, np.int64)
        first = segs[0].walk(which, mm, cap, set_locs=set_locs, set_base=bases[0], rows=rows)
        taken = first[1].copy()
        second = segs[1].walk(which, mm, cap, taken=taken, set_locs=set_locs, set_base=bases[1], rows=rows)
        for i, p in enumerate(pats):
            n0, l0 = segs[0].ref.locate(p, max_matches=mm, cap=cap)
            left = mm - n0
            n1, l1 = segs[1].ref.locate(p, max_matches=left, cap=cap) if left > 0 else (0, np.zeros(0, np.int32))
            assert first[1][i] == n0 and second[1][i] == n1 and first[2][i] == 0 and second[2][i] == 0, i
            assert (set_locs[i, :n0] == l0[:n0].astype(np.int64) + bases[0]).all(), i
            assert (set_locs[i, n0:n0 + n1] == l1[:n1].astype(np.int64) + bases[1]).all(), i
            assert (set_locs[i, n0 + n1:] == -7).all(), i
            assert (n1 == 0) if exhausted[i] else (n0 + n1 == mm) if cut[i] else True
        assert (first[0] == -7).all() and (second[0] == -7).all()  # nothing goes to `locs` when a set's rows take the hits
        runs.append((set_locs, first[1], first[2], first[3], second[1], second[2], second[3]))
    for a, b in zip(*runs):  # the walk and the gather agree: rows, found, statuses, LF-steps
        assert (a == b).all()


def test_option_and_info_on_handles_without_a_table():
    """fails on a library without the feature: unknown option, missing symbol"""
    E = ia._lib.E_ARG
    try:
        assert ia.lib.fmx_set_option(b"locate_rows", 0) == 0
        assert ia.lib.fmx_set_option(b"locate_rows", 1) == 0
        assert ia.lib.fmx_set_option(b"locate_rows", -1) == E
        assert ia.lib.fmx_set_option(b"locate_rows", 2) == E
        for v, rc in ((0, 0), (1, 0), (2, E), (-1, E)):
            assert ia.lib.fmx_set_option(b"rows_order", v) == rc
        # host-only handles made while the option is on: nothing is resident, nothing is grown
        fm = ia.FmIndex("This is a long string\0", 4, True, device=None)
        assert fm.locate_rows_info() == (0, 0)
        nbytes, replay = C.c_int64(-1), C.c_int64(-1)
        assert ia.lib.fmx_locate_rows_info(fm._h, None, None) == 0
        rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
        assert ia.lib.fmx_locate_rows_info(rrr._h, C.byref(nbytes), C.byref(replay)) == 0 and (nbytes.value, replay.value) == (0, 0)
        wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
        nbytes, replay = C.c_int64(-1), C.c_int64(-1)
        assert ia.lib.fmx_locate_rows_info(wt._h, C.byref(nbytes), C.byref(replay)) == 0 and (nbytes.value, replay.value) == (0, 0)
        sa = ia.SuffixArray("banana", device=None, build_device=-1)
        sa.construct()
        assert ia.lib.fmx_locate_rows_info(sa._h, C.byref(nbytes), C.byref(replay)) == E  # documented: not an FM-index handle
        assert ia.lib.fmx_locate_rows_info(None, C.byref(nbytes), C.byref(replay)) == E
    finally:
        ia.lib.fmx_set_option(b"locate_rows", 0)
        ia.lib.fmx_set_option(b"rows_order", 0)
    assert "fmx_locate_rows_info" in ia.SYMBOLS


def test_damaged_images_never_leave_the_table(tmp_path):
    """tests/cpp/fuzz_rows.cpp: images the validators accept (mutated streams, mutated images with a matching checksum) get a row
    table — filled over the tree and over each directory form, into an exact-size heap block — and are located through it under
    AddressSanitizer with the watchdog.  A damaged image may answer wrongly or with a status; it never reads outside the table."""
    csrc = os.path.join(ROOT, "index4j_amd", "csrc")
    for name, defs, seed, iters in (("fuzz_rows", [], 1, 700), ("fuzz_rows_compact", ["-DFMX_COMPACT=1"], 3, 300)):
        exe = str(tmp_path / name)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer"] + defs + ["-I" + csrc,
               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fuzz_rows.cpp")]
        cmd += [os.path.join(csrc, f) for f in ("fmx_build.cpp", "fmx_serial.cpp", "fmx_blob.cpp", "fmx_synth.cpp")]
        subprocess.check_call(cmd + ["-lpthread", "-o", exe])
        r = subprocess.run([exe, str(iters), str(seed)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "HANG" not in r.stderr, r.stdout[-2000:] + r.stderr[-6000:]
        assert r.stdout.startswith("rows fuzz ok:"), r.stdout
        assert int(r.stdout.split()[3]) >= 20, r.stdout  # damaged images that were accepted, filled and located

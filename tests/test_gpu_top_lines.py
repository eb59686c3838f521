"""The lines ranked by the number behind a pattern, on the GPU: packed hits -> n x top rows (line, value, position) and the per-pattern
counters (fmx_top_lines_of_hits_dev: the kernels of fmx_hit_top.hip around the packed extract, rocPRIM's radix sorts, scan and
reduce_by_key) and the host forms fmx_top_lines_where_batch / fmx_top_lines_where_class_batch with their Python and C++ mirrors.

The judge is judge_top_lines (tests/test_top_lines_cpu.py): the oracle's windows, Python's integers, Where's kept hits
(tests/test_field_values_where_cpu.py), plain `sorted`, computed once per batch.  Every output is prefilled with a sentinel and padded
by 64 entries: the entries behind rows[i] inside n x top must be 0, and what lies beyond must keep the sentinel.  Every refused call
returns before a launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_where_cpu import EVERY_LINE, Where
from test_gpu_field_values import ST_NOT_ENABLED, last_error
from test_gpu_field_values_where import Filled
from test_gpu_locate_rows import _torch
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_top_lines_cpu import (FIXTURE_CASES, MIX_DESC, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, assert_fixture_figures, check_top, judge_top_lines,
                                judge_where_top)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64             # entries behind the answer that must keep the sentinel
LEAD, EXTRA = 3, 70  # slots in front of hit_off[0] and behind hit_off[n] that hold no hit
TILE, LANES = 1024, 256  # slots of a key kernel's workgroup a pass, items of an element-wise one's
NAMES = ("rows", "row_line", "row_value", "row_loc", "lines", "numbers", "not_number", "overflow")
WS_LIMIT = 2 << 30


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def up(a, dtype):
    return _torch().from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def dev_top(fm, n, d_hit_off_ptr, d_locs_ptr, n_hits, lens, descending, top=10, first=0, frac_digits=0, d_status_ptr=None, ws_bytes=None, skip=()):
    """fmx_top_lines_of_hits_dev; rc, a dict of the outputs cut to the answer's sizes — what lies behind them has kept the sentinel
    (asserted).  skip: outputs handed in as NULL"""
    torch = _torch()
    need = ia.lib.fmx_top_lines_of_hits_scratch_bytes(n, n_hits, top)
    assert need < WS_LIMIT
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    cells = n * max(top, 0)
    sizes = dict(rows=n, row_line=cells, row_value=cells, row_loc=cells, lines=n, numbers=n, not_number=n, overflow=n)
    out = {k: torch.full((sizes[k] + PAD,), SENT, dtype=torch.int64 if k == "row_value" else torch.int32, device="cuda") for k in NAMES}
    tl, de = np.array(lens, np.int32), np.array(descending, np.uint8)  # the call's own copies: scribbled over once it is back
    ptr = lambda k: None if k in skip else out[k].data_ptr()  # noqa: E731
    rc = ia.lib.fmx_top_lines_of_hits_dev(fm.handle, n, tl.ctypes.data if n else None, de.ctypes.data if n else None, d_hit_off_ptr, d_locs_ptr, n_hits,
                                          frac_digits, first, top, *(ptr(k) for k in NAMES), d_status_ptr, ws.data_ptr(), use, stream())
    tl[:] = -9  # (the call has copied what it needs before it returns)
    de[:] = 9
    torch.cuda.synchronize()
    got = {}
    for k in NAMES:
        a = out[k].cpu().numpy()
        assert (a[sizes[k]:] == SENT).all(), "stored beyond the answer: " + k
        assert k not in skip or (a == SENT).all(), "stored through a NULL's neighbour: " + k
        got[k] = a[:sizes[k]]
    return rc, got


def untouched(got):
    return all((np.asarray(v) == SENT).all() for v in got.values())


def dev_block(f, n_terms, n, lens, descending, top=10, first=0, frac_digits=0, n_hits=None, **kw):
    """... over the value patterns' part of a Filled block (hit_off + n_terms: it does not start at 0 when a term has a hit).
    n_hits: the slots of the block the call may look at (default: all hits; up to 64 more: slots without a hit)"""
    n_hits = f.total if n_hits is None else n_hits
    assert n_hits <= f.total + 64  # (d.locs has that many slots behind the hits)
    return dev_top(f.fm, n, f.d.hit_off.data_ptr() + 8 * n_terms, f.d.locs.data_ptr(), n_hits, lens, descending, top, first, frac_digits,
                   d_status_ptr=f.d.st.data_ptr() + 4 * n_terms, **kw)


def dev_hits(fm, hit_off, locs, lens, descending, top=10, first=0, frac_digits=0, lead=LEAD, extra=EXTRA, **kw):
    """... over packed hits of the host (the KEPT hits of a Where), with `lead` slots in front of them and `extra` behind"""
    torch = _torch()
    n = len(hit_off) - 1
    d_off = up(np.asarray(hit_off, np.int64) + lead, np.int64)
    d_locs = up(np.concatenate([np.full(lead, -5, np.int32), np.asarray(locs, np.int32), np.full(extra + 1, -5, np.int32)]), np.int32)
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rc, got = dev_top(fm, n, d_off.data_ptr(), d_locs.data_ptr(), lead + len(locs) + extra, lens, descending, top, first, frac_digits,
                      d_status_ptr=status.data_ptr(), **kw)
    got["status"] = status.cpu().numpy()[:n]
    return rc, got


def host_top(fm, w, descending, top=10, first=0, frac_digits=0):
    return fm.top_lines_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, descending, top, first,
                                    None if w.window == EVERY_LINE else w.window, frac_digits)


def check_host(fm, o, w, T, descending, top=10, first=0, frac_digits=0, what=""):
    """the host form against the judge; kept, occurrences and the statuses against the Where"""
    want = judge_where_top(o, w, T, descending, top, first, frac_digits)
    got = host_top(fm, w, descending, top, first, frac_digits)
    check_top(got, want, what)
    assert (got["kept"] == w.kept).all() and (got["occurrences"] == w.occurrences).all() and (got["status"] == w.status[w.n_terms:]).all(), what
    assert (got["term_status"] == w.term_status).all(), what
    assert (got["numbers"] + got["not_number"] + got["overflow"] == got["kept"]).all(), what + ": the invariant"
    return want, got


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


# ---- the fixture's figures ----
def test_fixture_figures(hd):
    """the issue's figures through FmIndex.top_lines_by_number (the host form), each call also against the judge, through the device
    stage over the kept hits (slots in front and behind) and, where nothing filters, over a Filled block; the class twin on "SIZE "
    in any case; the text of the rows"""
    o, fm, T = hd
    lines_of_text = HD.split("\n")

    def get(pattern, largest=True, first=0, top=10, where=None, lines=None, frac_digits=0):
        w = Where("hd16", o, T, [pattern], [where] if where else [], [0 if where else -1], lines or EVERY_LINE)
        desc = [1 if largest else 0]
        want, got = check_host(fm, o, w, T, desc, top, first, frac_digits, "%r %r %r" % (pattern, where, lines))
        rc, dev = dev_hits(fm, w.kept_off, w.kept_locs, w.lens, desc, top, first, frac_digits)
        assert rc == 0 and (dev.pop("status") == 0).all(), last_error()
        check_top(dev, want, "device stage over the kept hits, %r" % pattern)
        if not where and not lines:
            rc, dev = dev_block(Filled(fm, w.ch, w.off), 0, 1, w.lens, desc, top, first, frac_digits)
            assert rc == 0, last_error()
            check_top(dev, want, "device stage over a block, %r" % pattern)
        res = fm.top_lines_by_number(pattern, top, largest, first, where, lines, frac_digits, text=True)
        assert res.text == [lines_of_text[k] for k in res.line] and len(res) == want.rows[0] and res.occurrences == w.occurrences[0]
        return res

    assert_fixture_figures(get)
    assert "SIZE " not in HD and "Size " not in HD  # one spelling in the text: the class twin's answer is the literal's
    for pattern, kw, numbers, lines, rows, n_rows in FIXTURE_CASES[:6]:
        a, b = fm.top_lines_by_number("SIZE ", ignore_case=True, **kw), fm.top_lines_by_number(pattern, **kw)
        assert (a.numbers, a.lines, len(a)) == (numbers, lines, n_rows) and a.kept == b.kept and a.occurrences == b.occurrences == 608
        assert a.line.tolist() == b.line.tolist() and a.value.tolist() == b.value.tolist() and a.loc.tolist() == b.loc.tolist()
        assert fm.top_lines_by_number("SIZE ", **kw).lines == 0
    none = fm.top_lines_by_number("zzqq#", text=True)
    assert len(none) == 0 and none.text == [] and (none.lines, none.numbers, none.kept, none.occurrences) == (0, 0, 0, 0)


# ---- cross-checks against the existing calls on the same Where ----
def test_cross_checks_against_number_stats_and_field_values(hd):
    """numbers, not_number and overflow equal number_stats_where_batch's without edges; row 0 ascending is its min, row 0 descending
    its max; kept and occurrences equal field_values_where_batch's — mixed orders in one batch, a pattern without a hit, one whose
    hits never parse, one whose query has no line, top larger than every lines[i]"""
    o, fm, T = hd
    w = Where("hd16 top mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    stats = fm.number_stats_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, None, (), 0)
    fv = fm.field_values_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, " ", 8)
    for desc in (MIX_DESC, [1 - d for d in MIX_DESC]):
        want, got = check_host(fm, o, w, T, desc, 2500, 0, 0, "mix %r" % desc)
        assert (got["numbers"] == stats["count"][:, 0]).all() and (got["not_number"] == stats["not_number"]).all()
        assert (got["overflow"] == stats["overflow"]).all() and (got["kept"] == stats["kept"]).all()
        assert (got["kept"] == fv[6]).all() and (got["occurrences"] == fv[5]).all()
        best = np.where(np.asarray(desc) == 1, stats["max"][:, 0], stats["min"][:, 0])
        assert (got["row_value"][:, 0] == best).all() and (got["rows"] == got["lines"]).all()
    assert got["lines"][2] == 0 and got["lines"][3] == 0 and got["not_number"][3] == got["kept"][3] > 0 and got["kept"][6] == 0
    for top, first, F in ((1, 0, 3), (7, 100, 9), (10, 2000, 0)):
        check_host(fm, o, w, T, MIX_DESC, top, first, F, "mix top %d first %d" % (top, first))
    win = Where("hd16 top mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, (300, 1700))
    check_host(fm, o, win, T, MIX_DESC, 20, 3, 0, "mix in a window of lines")
    # the device stage with terms in front of the value patterns (hit_off[0] != 0), slots behind, outputs handed in as NULL
    raw = Where("hd16 top mix", o, T, MIX_PATTERNS, MIX_QUERIES, [-1] * len(MIX_PATTERNS))
    f = Filled(fm, raw.ch, raw.off)
    assert raw.hit_off[raw.n_terms] > 0
    want = judge_where_top(o, raw, T, MIX_DESC, 12, 1, 0)
    rc, got = dev_block(f, raw.n_terms, raw.n, raw.lens, MIX_DESC, 12, 1, 0, n_hits=f.total + 37)
    assert rc == 0, last_error()
    check_top(got, want, "raw hits, terms in front")
    rc, got = dev_block(f, raw.n_terms, raw.n, raw.lens, MIX_DESC, 12, 1, 0, skip=("row_line", "lines", "numbers", "overflow"))
    assert rc == 0 and (got["row_value"].reshape(raw.n, 12) == want.row_value).all() and (got["rows"] == want.rows).all(), last_error()
    assert (got["row_loc"].reshape(raw.n, 12) == want.row_loc).all() and (got["not_number"] == want.not_number).all()
    # n_hits == 0: rows and counters are zeroed; n == 0: nothing is written
    rc, got = dev_block(f, raw.n_terms, raw.n, raw.lens, MIX_DESC, 4, n_hits=0)
    assert rc == 0 and got["row_line"].shape == (4 * raw.n,) and all((v == 0).all() for v in got.values()), last_error()
    rc, got = dev_block(f, raw.n_terms, 0, [], [], 4)
    assert rc == 0 and got["rows"].shape == (0,), last_error()
    out = fm.top_lines_where_batch(np.zeros(0, np.uint16), [0], *ia.pack_patterns(["INFO"]), [0, 1], [0], [], [], 5)
    assert out["row_line"].shape == (0, 5) and list(out["term_status"]) == [0]


# ---- what the fixture cannot reach ----
def synthetic_text():
    """line 0: the same value twice and a larger one; lines 1 .. 40: equal values across lines (7, 8, 9 in turn) and the call's
    maximum on three of them; line 41: 3,000 hits (more than one tile of 1,024), the maximum twice among them; the last line has no
    line feed behind it"""
    rng = np.random.default_rng(11)
    head = ["x=5 x=5 x=9"] + ["x=%d y=%d" % (7 + i % 3, i) if i % 13 else "x=99999" for i in range(1, 41)]
    long_values = rng.integers(10, 90000, 3000).tolist()
    long_values[17] = long_values[2901] = 99999
    long_values[5] = long_values[2000] = 1
    return "\n".join(head + [" ".join("x=%d" % v for v in long_values), "x=1 x=0x", "x=3 x=12"])


def test_synthetic_text():
    """one line with 3,000 hits (the per-line reduction crosses workgroups of slots), equal values across several lines, the same value
    twice on one line, a last line without a line feed, hit_off[0] > 0 with slots behind the hits — through the device stage and the
    host form, in both orders"""
    text = synthetic_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    fm = ia.FmIndex(text, 4, True, device=0)
    try:
        assert fm.build_line_table("\n") == 44 and not text.endswith("\n")
        pats = ["x=", "=", "x=9"]
        raw = Where("synthetic top", o, T, pats, [dict(all=["x=7"])], [-1] * 3)
        f = Filled(fm, raw.ch, raw.off)
        assert raw.hit_off[raw.n_terms] > 0 and raw.kept[0] > 3 * TILE - 100
        for desc, top, first in (([1, 0, 1], 50, 0), ([0, 1, 0], 6, 0), ([1, 1, 0], 5, 2), ([0, 0, 1], 3, 41)):
            want = judge_where_top(o, raw, T, desc, top, first, 0)
            rc, got = dev_block(f, raw.n_terms, raw.n, raw.lens, desc, top, first, 0, n_hits=f.total + 41)
            assert rc == 0, last_error()
            check_top(got, want, "synthetic, device stage, %r" % desc)
            check_host(fm, o, raw, T, desc, top, first, 0, "synthetic, host form, %r" % desc)
        best = judge_where_top(o, raw, T, [1, 0, 1], 50).ranked[0]
        long_start = int(T[40]) + 1
        first_max = long_start + len(" ".join(text[long_start:].split(" ")[:17])) + 1  # the FIRST of the line's two maxima
        assert len(best) == 44 and best[:4] == [(13, 99999, text.index("x=99999")), (26, 99999, int(T[25]) + 1), (39, 99999, int(T[38]) + 1),
                                               (41, 99999, first_max)]
        low = judge_where_top(o, raw, T, [0, 0, 0], 50).ranked[0]
        assert [r[:2] for r in low[:4]] == [(42, 0), (41, 1), (43, 3), (0, 5)] and low[3][2] == 0  # "x=0x" is 0; 5 at its first position
        assert [r[1] for r in low[4:8]] == [7, 7, 7, 7] and [r[0] for r in low[4:8]] == [3, 6, 9, 12]  # equal values: by line
        kept = Where("synthetic top", o, T, pats, [dict(all=["x=7"]), dict(none=["y="], any=["x="])], [0, 1, -1], (1, 43))
        for desc in ([1, 0, 1], [0, 1, 0]):
            check_host(fm, o, kept, T, desc, 9, 0, 0, "synthetic, filtered, %r" % desc)
        res = fm.top_lines_by_number("x=", 2, text=True)
        assert res.line.tolist() == [13, 26] and res.text == ["x=99999"] * 2
    finally:
        fm.close()


# ---- the loops ----
def geometry(fm, items):
    key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
    assert ia.lib.fmx_hit_lines_geometry(fm.handle, int(items), C.byref(key_grid), C.byref(flat_grid)) == 0
    return key_grid.value, flat_grid.value


def key_passes(fm, slots):
    return -(-slots // (geometry(fm, slots)[0] * TILE))


def flat_passes(fm, items, grid_of=None):
    return -(-items // (geometry(fm, items if grid_of is None else grid_of)[1] * LANES))


def assert_loops(what, **passes):
    """every named loop runs at least three passes on this card; the figures are printed for the record"""
    print("%s: passes %s" % (what, ", ".join("%s %d" % kv for kv in passes.items())))
    assert min(passes.values()) >= 3, (what, passes)


def test_every_loop_runs_three_passes(hd):
    """(" ", "size ", "blk_") under a query, the batch repeated until its slots are more than three passes of the larger grid: every
    repetition's rows and counters are the one-repetition judge's.  Then the same hits as the first patterns of a batch of more
    than three grids of patterns, the others without a hit, at top = 1: the loops over the patterns and over the rows.  The sizes
    come from fmx_hit_lines_geometry and the pass counts are asserted first"""
    o, fm, T = hd
    key_grid, flat_grid = geometry(fm, 10 ** 9)
    KEY, FLAT = key_grid * TILE, flat_grid * LANES
    w = Where("hd16 top loops", o, T, [" ", "size ", "blk_"], [dict(all=["terminating"])], [-1, -1, 0])
    desc, per = [1, 0, 1], int(w.kept_off[-1])
    reps = 3 * max(KEY, FLAT) // per + 1
    n, total = 3 * reps, reps * per
    slots = LEAD + total + EXTRA
    top = -(-(3 * FLAT + 1) // n)
    assert_loops("top lines, hits", k_top_keys=key_passes(fm, slots), k_top_lines=key_passes(fm, slots),
                 k_top_parse=flat_passes(fm, slots + 1), k_top_fill=flat_passes(fm, slots), k_top_cands=flat_passes(fm, slots),
                 k_top_patterns=flat_passes(fm, slots), k_top_rows=flat_passes(fm, n * top))
    want = judge_where_top(o, w, T, desc, top, 2, 0)
    assert want.lines.min() > 0 and (want.rows < top).all()
    hit_off = np.concatenate([[0], np.cumsum(np.tile(w.kept, reps))])
    locs, lens = np.tile(w.kept_locs, reps), np.tile(w.lens, reps)
    rc, got = dev_hits(fm, hit_off, locs, lens, desc * reps, top, 2, 0)
    assert rc == 0, last_error()
    for name in NAMES:
        g, b = got[name].reshape(reps, -1), getattr(want, name).reshape(1, -1)
        bad = np.flatnonzero((g != b).any(axis=1))
        assert len(bad) == 0, "%s differs in the repetitions %r" % (name, bad[:8])
    # more patterns than three grids of lanes: the hits belong to the first n of them
    many = 3 * FLAT + 2
    assert_loops("top lines, patterns", k_top_tails=flat_passes(fm, many + 1), k_top_rows=flat_passes(fm, many))
    hit_off = np.concatenate([hit_off, np.full(many - n, hit_off[-1])])
    rc, got = dev_hits(fm, hit_off, locs, np.concatenate([lens, np.ones(many - n, np.int32)]), np.resize(np.array(desc, np.uint8), many), 1, 0, 0)
    assert rc == 0, last_error()
    one = judge_where_top(o, w, T, desc, 1, 0, 0)
    for name in NAMES:
        g = got[name]
        assert (g[n:] == 0).all(), name + " of a pattern without a hit"
        assert (g[:n].reshape(reps, -1) == getattr(one, name).reshape(1, -1)).all(), name


# ---- an index without extraction, a missing line table, refusals ----
def test_index_without_extraction(hd):
    o, fm0, T = hd
    w = Where("hd16 top plain", o, T, ["size ", "blk_", "zzqq#"], [dict(all=["addStoredBlock"])], [0, -1, -1])
    fm = ia.FmIndex(HD, 16, False, device=0)
    try:
        fm.build_line_table("\n")
        got = host_top(fm, w, [1, 0, 1], 4)
        assert (got["status"] == ST_NOT_ENABLED).all() and (got["kept"] == w.kept).all() and (got["occurrences"] == w.occurrences).all()
        assert w.kept[0] == 314 and all((got[k] == 0).all() for k in NAMES)
        raw = Where("hd16 top plain", o, T, ["size ", "blk_", "zzqq#"], [], [-1] * 3)
        f = Filled(fm, raw.ch, raw.off)
        rc, dev = dev_block(f, 0, 3, raw.lens, [1, 0, 1], 4)
        assert rc == 0 and all((v == 0).all() for v in dev.values()), last_error()
        assert (f.d.st.cpu().numpy()[:3] == ST_NOT_ENABLED).all()
        with pytest.raises(RuntimeError):
            fm.top_lines_by_number("size ")
    finally:
        fm.close()


def test_refusals_leave_the_outputs_untouched(hd):
    """a workspace one byte short, the shape and argument refusals, an index without a line table (always refused: the answer is
    lines), a SuffixArray handle: each returns before a launch"""
    o, fm, T = hd
    w = Where("hd16", o, T, ["size "], [], [-1])
    f = Filled(fm, w.ch, w.off)
    E_ARG = ia._lib.E_ARG
    need = ia.lib.fmx_top_lines_of_hits_scratch_bytes(1, f.total, 10)
    assert need > 200 * f.total and need % 256 == 0 and need < 400 * f.total + (1 << 20)
    rc, got = dev_block(f, 0, 1, w.lens, [1], ws_bytes=need - 1)
    assert rc == E_ARG and "fmx_top_lines_of_hits_scratch_bytes" in last_error() and untouched(got)
    for bad in (dict(frac_digits=-1), dict(frac_digits=10), dict(first=-1), dict(top=0), dict(lens=[-1]), dict(n_hits=-1)):
        args = dict(lens=w.lens)
        args.update(bad)
        rc, got = dev_block(f, 0, 1, descending=[1], **args)
        assert rc == E_ARG and untouched(got), bad
    assert ia.lib.fmx_top_lines_of_hits_scratch_bytes(1, f.total, (1 << 27) + 1) == 0
    torch = _torch()
    p = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    one, d1 = np.array([5], np.int32), np.array([1], np.uint8)
    dv = ia.lib.fmx_top_lines_of_hits_dev

    def call(h=fm.handle, n=1, tl=one, d=d1, n_hits=5, hoff=p.data_ptr(), rows=p.data_ptr(), top=3):
        return dv(h, n, tl.ctypes.data, None if d is None else d.ctypes.data, hoff, p.data_ptr(), n_hits, 0, 0, top, rows, None, None, None, None, None,
                  None, None, None, p.data_ptr(), 256, stream())

    for bad in (dict(h=None), dict(n=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(rows=None), dict(d=None), dict(top=(1 << 27) + 1),
                dict(n=1 << 11, tl=np.zeros(1 << 11, np.int32), d=np.zeros(1 << 11, np.uint8), top=(1 << 16) + 1)):
        assert call(**bad) == E_ARG, bad
    assert call() == E_ARG and "fmx_top_lines_of_hits_scratch_bytes" in last_error()  # (256 bytes of workspace)
    bare = ia.FmIndex(HD[:5000], 16, True, device=0)
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    try:
        sa.construct()
        assert call(h=bare.handle) == E_ARG and "fmx_line_table_build" in last_error()
        assert call(h=sa._h) == E_ARG
        for run in (lambda: bare.top_lines_by_number("size "), lambda: bare.top_lines_by_number("size ", where=dict(all="INFO"))):
            with pytest.raises(ia.FmxError) as err:
                run()
            assert err.value.code == E_ARG and "fmx_line_table_build" in str(err.value)
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == SENT).all()  # nothing launched, nothing written
    # ... and the exact workspace serves
    rc, got = dev_block(f, 0, 1, w.lens, [1], ws_bytes=need)
    assert rc == 0, last_error()
    check_top(got, judge_where_top(o, w, T, [1]), "the exact workspace")
    for kw in (dict(top=0), dict(first=-1), dict(frac_digits=10), dict(lines=(5, 4))):
        with pytest.raises(ia.FmxError) as err:
            fm.top_lines_by_number("size ", **kw)
        assert err.value.code == E_ARG


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_top_lines_mirror.cpp prints what topLinesByNumberBatch / topLinesByNumber return: the batch form against the
    judge, topLinesByNumber against the batch form's row"""
    o, fm, T = hd
    exe = str(tmp_path / "test_top_lines_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_top_lines_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    w = Where("hd16 top mirror", o, T, ["size ", "size ", "zzqq#", "blk_"], [dict(all=["addStoredBlock"])], [-1, 0, 0, -1])
    want = judge_where_top(o, w, T, [1, 0, 1, 0], 5, 1, 0)
    assert out["batch_rows"] == want.rows.tolist() and out["batch_line"] == want.row_line.ravel().tolist()
    assert out["batch_value"] == want.row_value.ravel().tolist() and out["batch_loc"] == want.row_loc.ravel().tolist()
    assert out["batch_lines"] == want.lines.tolist() and out["batch_numbers"] == want.numbers.tolist()
    assert out["batch_not_number"] == want.not_number.tolist() and out["batch_overflow"] == want.overflow.tolist()
    assert out["batch_occurrences"] == [608, 608, 0, 2468] and out["batch_kept"] == w.kept.tolist() and out["batch_status"] == [0] * 4
    assert out["batch_term_status"] == [0]
    # topLinesByNumber(size, 5, smallest, first 1, where addStoredBlock) is pattern 1 of the batch
    r1 = int(want.rows[1])
    assert out["one_line"] == want.row_line[1, :r1].tolist() and out["one_value"] == want.row_value[1, :r1].tolist()
    assert out["one_loc"] == want.row_loc[1, :r1].tolist()
    assert out["one_counts"] == [r1, int(want.lines[1]), int(want.numbers[1]), int(want.not_number[1]), int(want.overflow[1]), int(w.kept[1])]
    assert out["src_line"] == [940, 980, 1334, 1416] and out["src_value"] == [251910] * 4
    assert out["win_line"] == [1015, 1094] and out["win_value"] == [107727140948970996, 157913239647511296] and out["win_counts"] == [2, 53, 60]

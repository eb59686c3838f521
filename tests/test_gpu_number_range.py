"""Query terms on the number behind a pattern on the GPU (latency_ms >= 500): packed hits -> the packed hits whose number lies in a
range (fmx_hits_in_number_range_dev: the kernels of fmx_hit_range.hip around the packed extract, rocPRIM's scans and
fmx_hit_filter.hip's stable store) and the host forms fmx_match_query_number_batch / fmx_match_query_number_class_batch with their
Python and C++ mirrors.

The judge is Ranged (tests/test_number_range_cpu.py): the oracle's hits and windows, parse_number and Python's integers, then
TermBatch.judge's set algebra over the hits that pass, computed once per batch.  Every output is prefilled with a sentinel and
padded, and what lies behind the answer must keep it.  The kept hits are compared IN ORDER: the compaction is stable.  Options are
set inside the tests and put back in `finally`.  Every refused call returns before a launch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_where_cpu import Where
from test_gpu_field_values import SENT64, ST_NOT_ENABLED, last_error
from test_gpu_field_values_where import Filled
from test_gpu_locate_rows import _torch, options
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_range_cpu import MIX_RANGED, MiB64, Ranged, as_list_of, assert_fixture_figures, check_range, range_cases, term_of, trimmed, whole
from test_number_stats_cpu import FRACS, INT64_MAX, MIX_PATTERNS, NAN, OVER, parser_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
PAD = 64  # entries behind the answer that must keep the sentinel
MIX = MIX_RANGED + [dict(all=[("size ", 3, 2)]), dict(all=["addStoredBlock"], none=[("size ", MiB64, None)]), dict(all=[("size ", 0, None)]),
                    dict(all=["INFO", ("size ", 0, 100), "WARN"])]


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def dev_range(fm, n, d_hit_off_ptr, d_locs_ptr, n_hits, lens, lo, hi, frac_digits=0, d_status_ptr=None, ws_bytes=None, skip=()):
    """fmx_hits_in_number_range_dev; rc, a dict of the outputs cut to the answer's sizes — what lies behind them has kept the
    sentinel (asserted) — and `raw`: every output as it came back.  skip: counters handed in as NULL"""
    torch = _torch()
    need = ia.lib.fmx_hits_in_number_range_scratch_bytes(n, n_hits)
    use = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(use, 1), dtype=torch.uint8, device="cuda")
    kept_off = torch.full((n + 1 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    kept_locs = torch.full((max(n_hits, 0) + PAD,), SENT, dtype=torch.int32, device="cuda")
    small = {k: torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda") for k in ("kept", "not_number", "overflow")}
    tl, a, b = np.array(lens, np.int32), np.array(lo, np.int64), np.array(hi, np.int64)  # the call's own copies: scribbled over once it is back
    rc = ia.lib.fmx_hits_in_number_range_dev(fm.handle, n, tl.ctypes.data, a.ctypes.data, b.ctypes.data, frac_digits, d_hit_off_ptr, d_locs_ptr, n_hits,
                                             kept_off.data_ptr(), kept_locs.data_ptr(), *(None if k in skip else small[k].data_ptr() for k in small),
                                             d_status_ptr, ws.data_ptr(), use, stream())
    tl[:] = -9  # (the call has copied what it needs before it returns)
    a[:] = -9
    b[:] = -9
    torch.cuda.synchronize()
    raw = dict(kept_off=kept_off.cpu().numpy(), kept_locs=kept_locs.cpu().numpy(), **{k: v.cpu().numpy() for k, v in small.items()})
    got = dict(raw=raw)
    if rc == 0 and n > 0:
        assert (raw["kept_off"][n + 1:] == SENT64).all(), "stored beyond kept_off"
        got["kept_off"] = raw["kept_off"][:n + 1]
        total = int(got["kept_off"][n])
        assert 0 <= total <= max(n_hits, 0) and (raw["kept_locs"][total:] == SENT).all(), "stored beyond kept_off[n]"
        got["kept_locs"] = raw["kept_locs"][:total]
        for k in small:
            assert (raw[k][n:] == SENT).all() and (k not in skip or (raw[k] == SENT).all()), "stored beyond the answer: " + k
            got[k] = raw[k][:n]
    return rc, got


def untouched(got):
    return all((v == (SENT64 if v.dtype == np.int64 else SENT)).all() for v in got["raw"].values())


def dev_terms(f, r, a=0, b=None, n_hits=None, **kw):
    """... over the terms [a, b) of a Filled block of a Ranged's batch (hit_off + a: it does not start at 0 when a term in front has
    a hit).  n_hits: the slots of the block the call may look at (default: all hits; up to 64 more: slots without a hit)"""
    b = r.n if b is None else b
    n_hits = f.total if n_hits is None else n_hits
    assert n_hits <= f.total + 64  # (d.locs has that many slots behind the hits)
    return dev_range(f.fm, b - a, f.d.hit_off.data_ptr() + 8 * a, f.d.locs.data_ptr(), n_hits, r.lens[a:b], r.lo[a:b], r.hi[a:b], r.F,
                     d_status_ptr=f.d.st.data_ptr() + 4 * a, **kw)


def part(r, a, b):
    """the judge's answer for the terms [a, b) alone"""
    return dict(kept_off=r.kept_off[a:b + 1] - r.kept_off[a], kept_locs=r.kept_locs[r.kept_off[a]:r.kept_off[b]], kept=r.kept[a:b],
                not_number=r.not_number[a:b], overflow=r.overflow[a:b])


def is_subsequence(kept, locs):
    """kept occurs in locs in order (a greedy walk: the first place every kept hit can take)"""
    at = 0
    for h in kept.tolist():
        where = np.flatnonzero(locs[at:] == h)
        if len(where) == 0:
            return False
        at += int(where[0]) + 1
    return True


def host_query(fm, r, max_lines=0, ignore_case=False, lo=True):
    """the host form over a Ranged's arrays; (lines, line_off, status, line_count, occurrences, kept, not_number, overflow)"""
    lo_hi = (r.lo, r.hi) if lo else (None, None)
    if ignore_case:
        packed = ia.pack_class_patterns([ia.ignore_case(ia.chars_to_str(t)) for t in r.terms])
        return fm.match_query_number_class_batch(*packed, r.query_off, r.kinds, *lo_hi, r.F, max_lines, True)
    return fm.match_query_number_batch(r.ch, r.off, r.query_off, r.kinds, *lo_hi, r.F, max_lines, True)


def check_host(fm, r, T, max_lines=0, what="", **kw):
    lines, line_off, status, line_count, occurrences, kept, not_number, overflow = host_query(fm, r, max_lines, **kw)
    want_lines, want_off, want_count = r.judge(T, max_lines)
    assert (line_off == want_off).all() and (line_count == want_count).all(), "%s: line_off %r, expected %r" % (what, line_off[:8], want_off[:8])
    assert lines.shape == want_lines.shape and (lines == want_lines).all(), what + ": lines"
    assert (status == r.status).all() and (occurrences == r.counts).all(), what + ": status, occurrences"
    assert (kept == r.kept).all() and (not_number == r.not_number).all() and (overflow == r.overflow).all(), "%s: kept %r, expected %r" % (what, kept, r.kept)
    return lines, line_off


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


@pytest.fixture(scope="module")
def mix(hd):
    o, fm, T = hd
    return Ranged("hd16 mix", o, MIX)


# ---- 1. the parser at the ranges' edges ----
def test_parser_at_the_ranges_edges():
    """the parser table in one synthetic text, one hit per case, through the device stage and the host form at F = 0, 3, 9: every
    value v against [v, v], [v + 1, max], [0, v - 1], [0, max] and [3, 2] — 2^63 - 1, the two overflow forms, "not a number", a digit
    run cut by the end of the text, a window clipped to zero length at textLength"""
    text, patterns, expected = parser_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    fm = ia.FmIndex(text, 4, True, device=0)
    try:
        fm.build_line_table("\n")
        f = None
        for k, F in enumerate(FRACS):
            for c in range(5):
                cases = [range_cases(e[k])[c] for e in expected]
                r = Ranged("parser table %d" % c, o, [dict(any=[(p, lo, hi) for p, ((lo, hi), _) in zip(patterns, cases)])], F)
                f = f or Filled(fm, r.ch, r.off)  # (the same patterns every time)
                rc, got = dev_terms(f, r, n_hits=f.total + c)
                assert rc == 0, last_error()
                check_range(got, whole(r), "parser table, device, F %d, range %d" % (F, c))
                assert got["kept"].tolist() == [int(ok) for _, ok in cases], (F, c)
                assert got["not_number"].tolist() == [int(e[k] is NAN) for e in expected] and got["overflow"].tolist() == [int(e[k] is OVER) for e in expected]
                check_host(fm, r, T, what="parser table, host, F %d, range %d" % (F, c))
        assert expected[10][0] == INT64_MAX
    finally:
        fm.close()


# ---- 2. the packed form's edges ----
def test_device_stage_on_the_tile_edges(hd, mix):
    """the mix (ranged terms between unranged ones, a ranged term without hits, " " with 30,094 hits across tiles): every slot; the
    slots trimmed to 1, 1,023, 1,024, 1,025 and to whole tiles, up to 64 slots behind the hits; parts of the block (hit_off[0] != 0);
    n = 1; every term unranged: kept_locs is locs byte for byte; counters handed in as NULL; a workspace one byte short"""
    o, fm, T = hd
    r = mix
    f = Filled(fm, r.ch, r.off)
    total = int(r.all_off[-1])
    locs = f.d.locs.cpu().numpy()[:total]
    sp = [ia.chars_to_str(t) for t in r.terms].index(" ")
    assert f.total == total and (locs == r.all_packed).all() and r.counts[sp] == 30094 and r.lo[sp] == 0
    for n_hits in (total, total + 37, total + 64, 1, 1023, 1024, 1025, 3 * 1024 + 1, total - 1):
        rc, got = dev_terms(f, r, n_hits=n_hits)
        assert rc == 0, last_error()
        check_range(got, trimmed(r, 0, n_hits), "n_hits %d of %d" % (n_hits, total))
    assert is_subsequence(got["kept_locs"][:3000], locs)
    # parts of the block: hit_off[0] != 0; a ranged pattern between two unranged ones; n = 1 (" " alone, across tiles)
    for a, b in ((1, 4), (2, r.n), (sp, sp + 1), (3, 4), (sp - 1, sp + 2), (r.n - 3, r.n)):
        assert r.all_off[a] > 0
        rc, got = dev_terms(f, r, a, b, n_hits=int(r.all_off[b]) + (a % 3) * 32)
        assert rc == 0, last_error()
        check_range(got, part(r, a, b), "terms [%d, %d)" % (a, b))
    assert r.lo[r.n - 3] < 0 <= r.lo[r.n - 2] and r.lo[r.n - 1] < 0 and r.lo[3] >= 0 and r.counts[3] == 0 and 0 < r.kept[sp] < r.counts[sp]
    # every term unranged: the hits come back as they are
    plain = Ranged("hd16 plain", o, [dict(all=["size ", "blk_"], none=["zzzq#", ":"])])
    fp = Filled(fm, plain.ch, plain.off)
    rc, got = dev_terms(fp, plain)
    assert rc == 0 and got["kept_locs"].tobytes() == fp.d.locs.cpu().numpy()[:fp.total].tobytes(), last_error()
    assert (got["kept"] == plain.counts).all() and got["not_number"].sum() == 0 and got["overflow"].sum() == 0
    # counters handed in as NULL: the others are still stored
    rc, got = dev_terms(f, r, skip=("kept", "overflow"))
    assert rc == 0 and (got["not_number"] == r.not_number).all() and (got["kept_off"] == r.kept_off).all(), last_error()
    # n_hits == 0: offsets and counters are zeroed; n == 0: only kept_off[0]
    rc, got = dev_terms(f, r, n_hits=0)
    assert rc == 0 and all((got["raw"][k][:r.n] == 0).all() for k in ("kept_off", "kept", "not_number", "overflow")), last_error()
    assert (got["raw"]["kept_locs"] == SENT).all()
    rc, got = dev_terms(f, r, 0, 0)
    assert rc == 0 and got["raw"]["kept_off"][0] == 0 and (got["raw"]["kept_off"][1:] == SENT64).all(), last_error()
    # a workspace one byte short: nothing is launched, nothing is stored; the exact workspace serves
    need = ia.lib.fmx_hits_in_number_range_scratch_bytes(r.n, total)
    assert need > 120 * total and need % 256 == 0
    rc, got = dev_terms(f, r, ws_bytes=need - 1)
    assert rc == ia._lib.E_ARG and "fmx_hits_in_number_range_scratch_bytes" in last_error() and untouched(got)
    rc, got = dev_terms(f, r, ws_bytes=need)
    assert rc == 0, last_error()
    check_range(got, whole(r), "the exact workspace")


# ---- 3. launch shapes ----
@pytest.mark.parametrize("opts", [dict(block=1024, groups_per_cu=1), dict(block=512, groups_per_cu=64)])
def test_launch_shapes(hd, mix, opts):
    """the mix under `block` = 1024 and a small groups_per_cu (looping grids in the extract and in the locate stages in front):
    the answers of the default"""
    o, fm, T = hd
    with options(**opts):
        f = Filled(fm, mix.ch, mix.off)
        rc, got = dev_terms(f, mix, n_hits=f.total + 5)
        assert rc == 0, last_error()
        check_range(got, whole(mix), repr(opts))
        check_host(fm, mix, T, what="mix under %r" % opts)


def test_grid_stride_loops_run_more_than_once(hd):
    """(" " ranged, "1" unranged, "0" ranged) repeated until the slots are more than the key grid covers in one pass, under
    groups_per_cu=1: the same answers as with the default"""
    o, fm, T = hd
    r = Ranged("hd16 heavy", o, [dict(all=[(" ", 0, 5), "1", ("0", 1, None)])])
    per = int(r.all_off[-1])
    key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
    assert ia.lib.fmx_hit_lines_geometry(fm.handle, 10 ** 9, C.byref(key_grid), C.byref(flat_grid)) == 0  # (the caps)
    reps = key_grid.value * 1024 // per + 2
    ch, off = ia.pack_patterns(r.terms * reps)
    lens, lo, hi = np.tile(r.lens, reps), np.tile(r.lo, reps), np.tile(r.hi, reps)
    answers = []
    for opts in (dict(groups_per_cu=1), {}):
        with options(**opts):
            f = Filled(fm, ch, off.astype(np.int32))
            assert f.total == reps * per and key_grid.value * 1024 < f.total
            rc, got = dev_range(fm, 3 * reps, f.d.hit_off.data_ptr(), f.d.locs.data_ptr(), f.total, lens, lo, hi)
        assert rc == 0, last_error()
        assert (got["kept"].reshape(reps, 3) == r.kept).all() and (got["not_number"].reshape(reps, 3) == r.not_number).all()
        assert (got["overflow"].reshape(reps, 3) == r.overflow).all() and (np.diff(got["kept_off"]).reshape(reps, 3) == r.kept).all()
        assert (got["kept_locs"].reshape(reps, -1) == r.kept_locs).all()
        answers.append(got)
    assert all((answers[0][k] == answers[1][k]).all() for k in ("kept_off", "kept_locs", "kept", "not_number", "overflow"))
    assert 0 < r.kept[0] < r.counts[0] and r.kept[1] == r.counts[1]


# ---- 4. the host forms against the judge ----
def test_host_forms(hd, mix):
    """the mix, literal and class (ignore_case: every term of the mix has ONE spelling on the fixture, so the judge's answer holds),
    with and without a limit; NONE with a ranged term; a query whose only ALL term is ranged and keeps nothing; NULL ranges; an
    index without extraction; n == 0"""
    o, fm, T = hd
    r = mix
    for max_lines in (0, 3):
        check_host(fm, r, T, max_lines, "mix, max_lines %d" % max_lines)
        check_host(fm, r, T, max_lines, "mix, class, max_lines %d" % max_lines, ignore_case=True)
    per = r.per_query(T)
    stored = Ranged("hd16 stored", o, [dict(all=["addStoredBlock"])]).per_query(T)[0]
    assert len(per[3]) == 0 and len(per[8]) == 0 and len(per[9]) == 74 and len(stored) == 314 and len(per[10]) == 485 and len(per[6]) == 14
    # a NONE term on a number: the lines whose "size " is no number stay
    text = HD.split("\n")
    no_number = [int(L) for L in stored if re.search("size (?![0-9])", text[L]) and not re.search("size [0-9]", text[L])]
    assert len(no_number) > 0 and set(no_number) <= set(per[9].tolist())
    # NULL num_lo and num_hi: match_query_batch's answer, array for array
    want = fm.match_query_batch(r.ch, r.off, r.query_off, r.kinds, 3, True)
    got = host_query(fm, r, 3, lo=False)
    assert all((a == b).all() and a.dtype == b.dtype for a, b in zip(got[:5], want)) and (got[5] == r.counts).all() and got[6].sum() == 0 and got[7].sum() == 0
    want = fm.match_query_class_batch(*ia.pack_class_patterns([ia.ignore_case(ia.chars_to_str(t)) for t in r.terms]), r.query_off, r.kinds, 0, True)
    got = host_query(fm, r, 0, ignore_case=True, lo=False)
    assert all((a == b).all() for a, b in zip(got[:5], want)) and (got[5] == r.counts).all()
    # every num_lo negative: the same lines
    lines = fm.match_query_number_batch(r.ch, r.off, r.query_off, r.kinds, [-1] * r.n, [-5] * r.n, 0, 0, True)
    plain = fm.match_query_batch(r.ch, r.off, r.query_off, r.kinds, 0, True)
    assert all((a == b).all() for a, b in zip(lines[:5], plain)) and (lines[5] == r.counts).all() and lines[6].sum() == 0
    for lo, hi in ((r.lo, None), (None, r.hi)):
        with pytest.raises(ia.FmxError) as err:
            fm.match_query_number_batch(r.ch, r.off, r.query_off, r.kinds, lo, hi)
        assert err.value.code == ia._lib.E_ARG
    # n == 0: queries without terms have no lines
    out = fm.match_query_number_batch(np.zeros(0, np.uint16), [0], [0, 0, 0], [], [], [], 0, 0, True)
    assert out[0].shape == (0,) and out[1].tolist() == [0, 0, 0] and out[3].tolist() == [0, 0] and out[5].shape == (0,)
    # an index built without extraction: ranged terms FMX_ST_NOT_ENABLED and no hits, unranged terms unaffected
    bare = ia.FmIndex(HD, 16, False, device=0)
    try:
        bare.build_line_table("\n")
        none_kept = Ranged("hd16 mix", o, [{w: [(term_of(t)[0], 3, 2) if isinstance(t, tuple) else t for t in as_list_of(g)] for w, g in qu.items()}
                                           for qu in MIX])
        assert (none_kept.lo == np.where(r.lo >= 0, 3, -1)).all() and (none_kept.counts == r.counts).all()
        lines, line_off, status, line_count, occurrences, kept, not_number, overflow = host_query(bare, r, 0)
        want_lines, want_off, want_count = none_kept.judge(T, 0)
        assert (line_off == want_off).all() and (lines == want_lines).all() and (line_count == want_count).all()
        assert (status == np.where(r.lo >= 0, ST_NOT_ENABLED, r.status)).all() and (occurrences == r.counts).all()
        assert (kept == np.where(r.lo >= 0, 0, r.counts)).all() and not_number.sum() == 0 and overflow.sum() == 0
        got = host_query(bare, r, 0, lo=False)  # (without ranges it still answers)
        assert all((a == b).all() for a, b in zip(got[:5], plain))
        f = Filled(bare, r.ch, r.off)
        rc, dev = dev_terms(f, r)
        assert rc == 0 and (dev["kept"] == np.where(r.lo >= 0, 0, r.counts)).all() and dev["not_number"].sum() == 0, last_error()
        assert (dev["kept_locs"] == r.all_packed[np.repeat(r.lo < 0, np.diff(r.all_off))]).all()
        assert (f.d.st.cpu().numpy()[:r.n] == np.where(r.lo >= 0, ST_NOT_ENABLED, r.status)).all()
    finally:
        bare.close()


# ---- 5. the invariant ----
def test_invariant_against_number_stats(hd):
    """with [0, 2^63 - 1] kept, not_number and overflow are count, not_number and overflow of number_stats_where_batch without edges
    and without a filter, for the number stats' mix of patterns (an empty pattern among them)"""
    o, fm, T = hd
    w = Where("hd16 mix", o, T, MIX_PATTERNS, [], [-1] * len(MIX_PATTERNS))
    n = len(MIX_PATTERNS)
    for F in (0, 3):
        stats = fm.number_stats_where_batch(*w.pattern_arrays(), *w.term_arrays(), w.query_off, w.kinds, w.where_of, None, (500,), F)
        out = fm.match_query_number_batch(*w.pattern_arrays(), list(range(n + 1)), [0] * n, [0] * n, [INT64_MAX] * n, F, 0, True)
        assert (out[5] == stats["count"][:, 0]).all() and (out[6] == stats["not_number"]).all() and (out[7] == stats["overflow"]).all(), F
        assert (out[4] == stats["occurrences"]).all() and (out[2] == stats["status"]).all() and out[5].sum() > 0 and out[6].sum() > 0


# ---- 6. the fixture's figures ----
def test_fixture_figures(hd):
    """the issue's figures through the host form, each call also against the judge"""
    o, fm, T = hd

    class Got:
        pass

    def get(queries, F):
        r = Ranged("hd16", o, queries, F)
        lines, line_off = check_host(fm, r, T, what=repr(queries))
        g = Got()
        out = host_query(fm, r)
        g.kept, g.not_number, g.overflow, g.per_query = out[5], out[6], out[7], [lines[a:b] for a, b in zip(line_off[:-1], line_off[1:])]
        return g

    assert_fixture_figures(get)


# ---- 7. the mirrors ----
def test_python_sugar(hd, mix):
    o, fm, T = hd
    per = mix.per_query(T)
    assert (fm.match_query(all=["addStoredBlock", ("size ", None, MiB64 - 1)]) == per[6]).all() and len(per[6]) == 14
    assert (fm.match_query(all=["addStoredBlock"], none=[("size ", MiB64, None)]) == per[9]).all()
    assert (fm.match_query(all=("size ", 0, None)) == per[10]).all() and (fm.match_query(all=[("SIZE ", 0, None)], ignore_case=True) == per[10]).all()
    assert (fm.match_query(all=[("size ", 0, None)], max_lines=7) == per[10][:7]).all() and len(fm.match_query(all=[("SIZE ", 0, None)])) == 0
    src = Ranged("hd16", o, [dict(all=[("src: /10.", 251000, 251500)])], 3)
    assert (fm.match_query(all=[("src: /10.", 251000, 251500)], frac_digits=3) == src.per_query(T)[0]).all() and src.kept[0] == 156
    rows = fm.grep(all=["addStoredBlock", ("size ", None, MiB64 - 1)], max_lines=3)
    assert [i for i, _ in rows] == per[6][:3].tolist() and all("addStoredBlock" in t and " size " in t for _, t in rows)
    assert (fm.match_query(all=["addStoredBlock"]) == Ranged("hd16 stored", o, [dict(all=["addStoredBlock"])]).per_query(T)[0]).all()  # (the existing path)
    assert fm.number_range_count("size ") == (485, 123, 0, 608) and fm.number_range_count("size ", MiB64) == (457, 123, 0, 608)
    assert fm.number_range_count("size ", None, MiB64 - 1) == (28, 123, 0, 608) and fm.number_range_count("size ", 3, 2) == (0, 123, 0, 608)
    assert fm.number_range_count("SRC: /10.", 251000, None, frac_digits=3, ignore_case=True)[0] == 184
    assert fm.number_range_count("blk_", 5 * 10 ** 18)[0] == 576 and fm.number_range_count("zzqq#") == (0, 0, 0, 0)
    for bad in (lambda: fm.match_query(all=[("size ", -1, 5)]), lambda: fm.match_query(all=[("size ", 0, 2 ** 63)]), lambda: fm.number_range_count("size ", -2)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(IndexError):
        fm.match_query(all=[("", 0, 5)])
    with pytest.raises(ia.FmxError):
        fm.match_query(all=[("size ", 0, 5)], frac_digits=10)


def test_cpp_mirror(hd, tmp_path):
    """tests/cpp/test_number_range_mirror.cpp prints what matchQueryNumberBatch / matchQueryNumber return"""
    o, fm, T = hd
    exe = str(tmp_path / "test_number_range_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_number_range_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    w = Ranged("hd16 mirror", o, [dict(all=["addStoredBlock", ("size ", 0, MiB64 - 1)]), dict(all=["addStoredBlock"], none=[("size ", MiB64, None)]),
                                  dict(all=[("size ", 3, 2)], any=[("zzqq#", 0, None)])])
    lines, line_off, line_count = w.judge(T, 0)
    assert out["batch_offsets"] == line_off.tolist() == [0, 14, 88, 88] and out["batch_lines"] == lines.tolist() and out["batch_line_count"] == line_count.tolist()
    assert out["batch_occurrences"] == w.counts.tolist() and out["batch_kept"] == w.kept.tolist() == [314, 28, 314, 457, 0, 0]
    assert out["batch_not_number"] == w.not_number.tolist() and out["batch_overflow"] == w.overflow.tolist()
    cut = Ranged("hd16 mirror cut", o, w.queries[:2])
    lines, line_off, line_count = cut.judge(T, 5)
    assert out["cut_offsets"] == line_off.tolist() == [0, 5, 10] and out["cut_lines"] == lines.tolist() and out["cut_line_count"] == [14, 74]
    src = Ranged("hd16", o, [dict(all=[("src: /10.", 251000, 251500)])], 3)
    assert out["one_lines"] == src.per_query(T)[0].tolist() and src.kept[0] == 156


# ---- 8. refusals: every one returns before a launch ----
def test_refusals_leave_the_outputs_untouched(hd, mix):
    o, fm, T = hd
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    r = Ranged("hd16", o, [dict(all=[("size ", 0, None)])])
    f = Filled(fm, r.ch, r.off)
    for bad in (dict(frac_digits=-1), dict(frac_digits=10), dict(lens=[-1]), dict(n_hits=-1)):
        args = dict(n=1, d_hit_off_ptr=f.d.hit_off.data_ptr(), d_locs_ptr=f.d.locs.data_ptr(), n_hits=f.total, lens=r.lens, lo=r.lo, hi=r.hi)
        args.update(bad)
        rc, got = dev_range(fm, **args)
        assert rc == E_ARG and untouched(got), bad
    torch = _torch()
    p = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    one, lo, hi = np.array([5], np.int32), np.array([0], np.int64), np.array([9], np.int64)
    dv = ia.lib.fmx_hits_in_number_range_dev

    def call(h=fm.handle, n=1, tl=one, lo_=lo, hi_=hi, F=0, hoff=p.data_ptr(), n_hits=5, koff=p.data_ptr(), klocs=p.data_ptr()):
        a = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return dv(h, n, a(tl), a(lo_), a(hi_), F, hoff, p.data_ptr(), n_hits, koff, klocs, None, None, None, None, p.data_ptr(), 256, stream())

    for bad in (dict(h=None), dict(n=-1), dict(tl=None), dict(lo_=None), dict(hi_=None), dict(F=10), dict(hoff=None), dict(koff=None), dict(klocs=None),
                dict(n_hits=1 << 31)):
        assert call(**bad) == E_ARG, bad
    assert call() == E_ARG and "fmx_hits_in_number_range_scratch_bytes" in last_error()  # (256 bytes of workspace)
    host = fm.match_query_number_batch
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    away = ia.FmIndex(HD[:5000], 16, True, device=None)
    bare = ia.FmIndex(HD[:5000], 16, True, device=0)
    try:
        sa.construct()
        for h in (sa._h, rrr._h, wt._h):
            assert call(h=h) == E_ARG, last_error()
        assert call(h=away.handle) == E_NO_DEVICE
        assert call(h=bare.handle) == E_ARG and "fmx_hits_in_number_range_scratch_bytes" in last_error()  # (no line table is needed)
        for index, code in ((away, E_NO_DEVICE), (bare, E_ARG)):  # the host form: not resident; no line table
            with pytest.raises(ia.FmxError) as err:
                index.match_query_number_batch(r.ch, r.off, r.query_off, r.kinds, r.lo, r.hi)
            assert err.value.code == code and (code != E_ARG or "fmx_line_table_build" in str(err.value))
    finally:
        away.close()
        bare.close()
    for kw in (dict(frac_digits=-1), dict(frac_digits=10)):
        with pytest.raises(ia.FmxError) as err:
            host(r.ch, r.off, r.query_off, r.kinds, r.lo, r.hi, **kw)
        assert err.value.code == E_ARG
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == SENT).all()  # nothing launched, nothing written

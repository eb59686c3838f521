"""Query terms on the number behind a pattern (fmx_hits_in_number_range_dev, fmx_match_query_number_batch; latency_ms >= 500) on the
CPU: the functions the kernels of index4j_amd/csrc/fmx_hit_range.hip run — fm_range_ranged, fm_range_code, fm_range_tail,
fm_range_not_number, fm_range_overflow (index4j_amd/csrc/fmx_hit_range.hpp), with fm_val_window, fm_hit_tile / fm_hit_pattern and
fm_filter_slot / fm_filter_kept_off — compiled for the host and driven by a mirror of the stages (tests/range_hostsim.cpp, a
stand-alone program: its `self` mode checks the functions at their edges, its `range` mode runs the stages lane by lane), built once
plain and once with -fsanitize=address,undefined and run directly, as a program.

The judge is Python over the oracle (Ranged): the hits are expected_packed's, the windows judge_values' (the oracle's extract over
[s, e) at max_len = 32), the number parse_number's (tests/test_number_stats_cpu.py) compared as Python ints, the lines of the queries
TermBatch.judge's set algebra (tests/test_match_query_cpu.py) over the hits that pass.  The GPU suite runs the kernels and the host
forms themselves (tests/test_gpu_number_range.py, which shares the helpers below)."""
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import judge_values
from test_field_values_where_cpu import as_list
from test_locate_all_cpu import SENT, expected_packed
from test_match_lines_cpu import judge_n_lines, judge_table
from test_match_query_cpu import TermBatch
from test_number_stats_cpu import FRACS, INT64_MAX, NAN, OVER, WINDOW, parse_number, parser_text

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SIM_SENT = -77  # range_hostsim.cpp's kSentinel
OUTSIDE, KEEP, NOT_NUMBER, OVERFLOW = 0, 1, 2, 3  # fmx_hit_range.hpp's codes
MiB64 = 67108864


def term_of(t):
    """(pattern, lo, hi) of a term of a query: a str is a plain string term (lo = hi = -1), None is an open bound"""
    if isinstance(t, tuple):
        return t[0], 0 if t[1] is None else t[1], INT64_MAX if t[2] is None else t[2]
    return t, -1, -1


class Ranged(TermBatch):
    """the judge's answer for a batch of TERMS cut into queries = [dict(all=, any=, none=)], a term a str or (str, lo, hi): the
    oracle's packed hits, the code of every hit, the hits that pass in the order they had, the three counters, and — through
    TermBatch.judge over the passing hits — the lines of the queries"""

    def __init__(self, key, o, queries, frac_digits=0):
        triples = [(term_of(t), k) for qu in queries for k, word in enumerate(("all", "any", "none")) for t in as_list_of(qu.get(word, ()))]
        self.queries, self.F = queries, frac_digits
        self.terms = [ia.as_chars(t[0]) for t, _ in triples]
        self.kinds = np.array([k for _, k in triples], np.uint8)
        self.lo, self.hi = np.array([t[1] for t, _ in triples], np.int64), np.array([t[2] for t, _ in triples], np.int64)
        per_query = [sum(len(as_list_of(qu.get(w, ()))) for w in ("all", "any", "none")) for qu in queries]
        self.query_off = np.concatenate([[0], np.cumsum(per_query)]).astype(np.int32)
        ch, off = ia.pack_patterns(self.terms)
        self.ch, self.off = np.ascontiguousarray(ch), off.astype(np.int32)
        self.lens = np.diff(self.off).astype(np.int32)
        self.n, self.q = len(self.terms), len(queries)
        batch_key = "%s ranged %r" % (key, [ia.chars_to_str(t) for t in self.terms])
        self.all_packed, self.all_off, self.status, _, self.counts = expected_packed(batch_key, o, self.ch, self.off, -1)
        j = judge_range(o, self.all_packed, self.all_off, self.lens, self.lo, self.hi, frac_digits)
        self.codes, self.kept_off, self.kept_locs, self.kept, self.not_number, self.overflow, self.windows = j
        # what TermBatch.judge reads: the hits a term HOLDS with
        self.packed, self.hit_off, self.total = self.kept_locs, self.kept_off, int(self.kept_off[-1])
        self._judged = {}


def as_list_of(group):
    """the terms of a group: a lone str and a lone (str, lo, hi) are one term"""
    if isinstance(group, tuple) and len(group) == 3 and isinstance(group[0], str) and not isinstance(group[1], str):
        return [group]
    return as_list(group)


def judge_range(o, locs, hit_off, lens, lo, hi, frac_digits):
    """by the definition, over packed hits: the window of every hit of a RANGED pattern from the oracle, its value, the comparison
    in Python ints.  (codes per hit, kept_off, kept_locs, kept, not_number, overflow, windows: (starts, stops, lengths, rows) per
    hit, an unranged pattern's empty)"""
    n = len(hit_off) - 1
    locs, hit_off = np.asarray(locs, np.int32), np.asarray(hit_off, np.int64)
    total = int(hit_off[-1]) - int(hit_off[0])
    base = int(hit_off[0])
    codes = np.full(total, KEEP, np.int32)
    starts, stops, lengths = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(total, np.int64)
    rows = np.zeros((total, WINDOW), np.uint16)
    ranged = [i for i in range(n) if lo[i] >= 0]
    if ranged:
        sub_locs = np.concatenate([locs[hit_off[i]:hit_off[i + 1]] for i in ranged] + [np.zeros(0, np.int32)]).astype(np.int32)
        sub_off = np.concatenate([[0], np.cumsum([hit_off[i + 1] - hit_off[i] for i in ranged])]).astype(np.int64)
        w = judge_values(o, sub_locs, sub_off, np.asarray(lens)[ranged], "", WINDOW)
        cache = {}
        for k, i in enumerate(ranged):
            for j in range(int(sub_off[k]), int(sub_off[k + 1])):
                ln = int(w.lengths[j])
                key = (w.rows[j, :ln].tobytes(), i)
                if key not in cache:
                    v = parse_number(w.rows[j, :ln].tolist(), frac_digits)
                    cache[key] = NOT_NUMBER if v is NAN else OVERFLOW if v is OVER else KEEP if int(lo[i]) <= v <= int(hi[i]) else OUTSIDE
                at = int(hit_off[i]) - base + j - int(sub_off[k])
                codes[at] = cache[key]
                starts[at], stops[at], lengths[at], rows[at] = w.starts[j], w.stops[j], ln, w.rows[j]
    per = [codes[hit_off[i] - base:hit_off[i + 1] - base] for i in range(n)]
    kept = np.array([(c == KEEP).sum() for c in per], np.int32)
    nn = np.array([(c == NOT_NUMBER).sum() for c in per], np.int32)
    ov = np.array([(c == OVERFLOW).sum() for c in per], np.int32)
    kept_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    kept_locs = locs[base:base + total][codes == KEEP].astype(np.int32)
    return codes, kept_off, kept_locs, kept, nn, ov, (starts, stops, lengths, rows)


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "range_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "range_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("range_hostsim")


def run_range_sim(simdir, text_len, lens, lo, hi, frac_digits, hit_off, locs, windows, n_hits=None, extra_hits=0, extract=True, sanitize=False):
    """the stages' mirror over a packed block (hit_off[0] may be non-zero; extra_hits slots behind hit_off[n] hold no hit; n_hits:
    fewer slots than hits) and the JUDGE's windows of the hits inside the slots (windows: judge_range's, per hit from hit_off[0]
    on).  Returns a dict: kept_off, kept_locs (cut to kept_off[n]; what lies behind has kept the sentinel), kept, not_number,
    overflow, not_enabled"""
    n = len(hit_off) - 1
    first, total = int(hit_off[0]), int(hit_off[-1])
    n_hits = total + extra_hits if n_hits is None else n_hits
    locs = np.concatenate([locs, np.full(extra_hits, SENT, np.int32)]).astype(np.int32)[:n_hits]
    inside = max(min(total, n_hits) - first, 0)
    starts, stops, lengths, rows = windows
    per_slot = np.zeros(n_hits, np.int64)
    per_slot[first:first + inside] = lengths[:inside]
    win_off = np.concatenate([[0], np.cumsum(per_slot)]).astype(np.int64)
    keep = np.arange(WINDOW)[None, :] < lengths[:inside, None]
    win = rows[:inside][keep] if inside else np.zeros(0, np.uint16)
    head = np.array([n, n_hits, frac_digits, text_len, int(extract)], np.int64)
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (head, np.asarray(lens, np.int32), np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(hit_off, np.int64), locs, win_off,
                  win.astype(np.uint16)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), "range", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.uint8)
    at = 0

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += count * np.dtype(dtype).itemsize
        return out

    kept_off, kept_locs = take(np.int64, n + 1), take(np.int32, n_hits)
    got = dict(kept_off=kept_off, kept=take(np.int32, n), not_number=take(np.int32, n), overflow=take(np.int32, n))
    start, stop, pattern, got["not_enabled"] = take(np.int32, n_hits), take(np.int32, n_hits), take(np.int32, n_hits), take(np.int32, n)
    assert at == len(raw)
    assert (kept_locs[kept_off[-1]:] == SIM_SENT).all(), "stored beyond kept_off[n]"
    got["kept_locs"] = kept_locs[:kept_off[-1]]
    # the windows of the stage are the judge's; a slot that is no hit has the pattern n and an empty window
    assert (start[first:first + inside] == starts[:inside]).all() and (stop[first:first + inside] == stops[:inside]).all()
    assert (start[:first] == 0).all() and (stop[first + inside:] == 0).all()
    assert (pattern[:first] == n).all() and (pattern[first + inside:] == n).all() and (pattern[first:first + inside] < n).all()
    return got


def trimmed(r, first, n_hits):
    """a Ranged's answer through the slots [.., n_hits) of a block whose ranged hits begin at slot `first`"""
    codes = r.codes[:max(n_hits - first, 0)]
    ends = np.clip(np.minimum(r.all_off, max(n_hits - first, 0)), 0, None)
    keep = np.concatenate([[0], np.cumsum(codes == KEEP)])
    nn, ov = np.concatenate([[0], np.cumsum(codes == NOT_NUMBER)]), np.concatenate([[0], np.cumsum(codes == OVERFLOW)])
    return dict(kept_off=keep[ends] - keep[ends[0]], kept_locs=r.all_packed[:len(codes)][codes == KEEP], kept=np.diff(keep[ends]),
                not_number=np.diff(nn[ends]), overflow=np.diff(ov[ends]))


def check_range(got, want, what):
    for k in ("kept_off", "kept", "not_number", "overflow"):
        assert (np.asarray(got[k]) == np.asarray(want[k])).all(), "%s: %s %r, expected %r" % (what, k, np.asarray(got[k])[:8], np.asarray(want[k])[:8])
    bad = np.flatnonzero(np.asarray(got["kept_locs"]) != np.asarray(want["kept_locs"]))
    assert len(bad) == 0, "%s: %d kept hits differ (or are out of order), first at %r" % (what, len(bad), bad[:5])


def whole(r):
    return dict(kept_off=r.kept_off, kept_locs=r.kept_locs, kept=r.kept, not_number=r.not_number, overflow=r.overflow)


def sim_ranged(simdir, o, r, what, **kw):
    got = run_range_sim(simdir, o.getInputLength() - 1, r.lens, r.lo, r.hi, r.F, r.all_off, r.all_packed, r.windows, **kw)
    check_range(got, whole(r), what)
    assert (r.kept + r.not_number + r.overflow <= r.counts).all() and (got["not_enabled"] == 0).all()
    return got


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


def range_cases(v):
    """the ranges every value v of the parser table is put against, and whether v passes: [v, v], [v + 1, max], [0, v - 1], [0, max],
    [3, 2]; a value that is NAN or OVER passes none of them"""
    if not isinstance(v, int):
        return [((0, 0), False), ((1, INT64_MAX), False), ((0, INT64_MAX - 1), False), ((0, INT64_MAX), False), ((3, 2), False)]
    return [((v, v), True), ((min(v + 1, INT64_MAX), INT64_MAX), v == INT64_MAX), ((0, max(v - 1, 0)), v == 0), ((0, INT64_MAX), True), ((3, 2), False)]


def test_per_item_functions(simdir):
    """fm_range_code at the ranges' edges for F = 0, 3, 9, what does not parse against every range, the word of the two reasons up
    to 2^31 - 1 of each, the refused arguments: range_hostsim.cpp's self_checks, plain and under AddressSanitizer and UBSan"""
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_parser_table_at_the_ranges_edges(simdir):
    """ONE text with one hit per case of the parser table; for F = 0, 3, 9 and every case with value v the five ranges of
    range_cases: 2^63 - 1, the overflow forms, "not a number", the digit run and the window clipped by the end of the text"""
    text, patterns, expected = parser_text()
    o = orc.OracleFmIndex(text, 4, True)
    for k, F in enumerate(FRACS):
        for c in range(5):
            cases = [range_cases(e[k])[c] for e in expected]
            r = Ranged("parser table %d" % c, o, [dict(any=[(p, lo, hi) for p, ((lo, hi), _) in zip(patterns, cases)])], F)
            assert (r.counts == 1).all()
            sim_ranged(simdir, o, r, "F %d, range %d" % (F, c), sanitize=c == k, extra_hits=c)
            assert r.kept.tolist() == [int(ok) for _, ok in cases], (F, c)
            assert r.not_number.tolist() == [int(e[k] is NAN) for e in expected] and r.overflow.tolist() == [int(e[k] is OVER) for e in expected]
    assert expected[10][0] == INT64_MAX and r.windows[2][-1] == 0 and r.windows[2][-2] == 3


# the fixture's figures (HDFS_2k_multichar.log, 2,000 lines): a Python regular expression over the decoded text gives them
FIGURES = [  # (pattern, F, lo, hi, hits that pass, lines they lie on)
    ("size ", 0, 0, None, 485, 485), ("size ", 0, MiB64, None, 457, 457), ("size ", 0, 0, MiB64 - 1, 28, 28), ("size ", 0, 2, 2, 1, 1),
    ("size ", 0, 3, 2, 0, 0), ("src: /10.", 3, 251000, 251500, 156, None), ("src: /10.", 3, 251000, None, 184, None),
    ("blk_", 0, 5 * 10 ** 18, None, 576, 461), ("blk_", 0, 0, None, 1237, 1004),
]
QUERY_FIGURES = [(dict(all=["addStoredBlock", ("size ", 0, MiB64 - 1)]), 14), (dict(all=["addStoredBlock"], none=[("size ", MiB64, None)]), 74),
                 (dict(all=["addStoredBlock"]), 314)]


def regex_figure(pattern, F, lo, hi):
    """(hits that pass, lines they lie on, hits followed by no number) straight off the text: no oracle, no window"""
    hi = INT64_MAX if hi is None else hi
    passing, lines, nn = 0, set(), 0
    for i, line in enumerate(HD.split("\n")):
        for m in re.finditer(re.escape(pattern), line):
            num = re.match(r"[0-9]+(\.[0-9]*)?" if F else r"[0-9]+", line[m.end():])
            if not num:
                nn += 1
                continue
            run, _, frac = num.group().partition(".")
            v = int(run) * 10 ** F + (int(frac[:F]) * 10 ** (F - len(frac[:F])) if frac[:F] else 0)
            if lo <= v <= hi:
                passing += 1
                lines.add(i)
    return passing, len(lines), nn


def assert_fixture_figures(get):
    """get(queries, F) -> an object with kept, not_number, overflow (per term) and per_query line lists: the figures of the fixture,
    whoever computed them"""
    for pattern, F, lo, hi, hits, lines in FIGURES:
        r = get([dict(all=[(pattern, lo, hi)])], F)
        assert int(r.kept[0]) == hits and (lines is None or len(r.per_query[0]) == lines), (pattern, lo, hi)
        assert int(r.overflow[0]) == 0 and (pattern != "size " or int(r.not_number[0]) == 123)
    for query, lines in QUERY_FIGURES:
        assert len(get([query], 0).per_query[0]) == lines, query


class JudgedFigures:
    def __init__(self, r, T):
        self.kept, self.not_number, self.overflow, self.per_query = r.kept, r.not_number, r.overflow, r.per_query(T)


def test_fixture_figures(simdir, hd):
    """the issue's figures: a regular expression over the text gives them, the judge over the oracle confirms them, and the stages'
    mirror gives the judge's answer"""
    o, T = hd
    assert judge_n_lines(T, len(HD)) == 2000
    for pattern, F, lo, hi, hits, lines in FIGURES:
        got = regex_figure(pattern, F, lo, hi)
        assert got[0] == hits and (lines is None or got[1] == lines) and (pattern != "size " or got[2] == 123), (pattern, lo, hi, got)
    calls = []

    def get(queries, F):
        r = Ranged("hd16", o, queries, F)
        sim_ranged(simdir, o, r, repr(queries), sanitize=len(calls) % 4 == 0, extra_hits=len(calls) % 3)
        calls.append(queries)
        return JudgedFigures(r, T)

    assert_fixture_figures(get)


MIX_RANGED = [dict(all=["terminating"]), dict(all=["blk_"], none=[("size ", MiB64, None)]), dict(all=[("zzzq#", 0, None)]),
              dict(none=[("size ", 0, None)]), dict(), dict(any=[("src: /10.", 251, 251), "Receiving"], none="src:"),
              dict(all=["addStoredBlock", ("size ", None, MiB64 - 1)]), dict(all=[("blk_", 5 * 10 ** 18, None), (" ", 0, 5)], any=["INFO", ("size ", 3, 2)])]


def test_mix_and_tile_edges(simdir, hd):
    """MIX_RANGED: ranged terms between unranged ones, a ranged term without hits, a range that keeps nothing, " " with 30,094 hits
    across tiles; the block trimmed to the tile edges and shifted (hit_off[0] != 0, slots behind the hits); every term unranged: the
    hits come back as they are; an index without extraction: a ranged term keeps nothing"""
    o, T = hd
    r = Ranged("hd16 mix", o, MIX_RANGED)
    sim_ranged(simdir, o, r, "mix", extra_hits=37)
    total = int(r.all_off[-1])
    assert total > 30 * 1024 and r.counts[r.n - 3] == 30094 and r.kept[3] == 0 and r.counts[3] == 0 and r.kept[r.n - 1] == 0
    for n_hits in (1, 1023, 1024, 1025, 3 * 1024 + 1, total - 1):
        got = run_range_sim(simdir, len(HD), r.lens, r.lo, r.hi, 0, r.all_off, r.all_packed, r.windows, n_hits=n_hits, sanitize=n_hits == 1025)
        check_range(got, trimmed(r, 0, n_hits), "n_hits %d" % n_hits)
    # the same block behind 1,500 slots of other patterns: hit_off[0] != 0
    shift = 1500
    locs = np.concatenate([np.full(shift, SENT, np.int32), r.all_packed])
    got = run_range_sim(simdir, len(HD), r.lens, r.lo, r.hi, 0, r.all_off + shift, locs, r.windows, extra_hits=64, sanitize=True)
    check_range(got, whole(r), "hit_off[0] = %d" % shift)
    # every term unranged: kept_locs is locs
    plain = Ranged("hd16 plain", o, [dict(all=["size ", "blk_"], none=["zzzq#", ":"])])
    got = sim_ranged(simdir, o, plain, "unranged")
    assert (got["kept_locs"] == plain.all_packed).all() and (plain.kept == plain.counts).all() and plain.not_number.sum() == 0
    # no extraction: ranged terms keep nothing and are told so, unranged ones are copied through
    got = run_range_sim(simdir, len(HD), r.lens, r.lo, r.hi, 0, r.all_off, r.all_packed, r.windows, extract=False)
    assert (got["not_enabled"] == (r.lo >= 0)).all() and (got["kept"] == np.where(r.lo >= 0, 0, r.counts)).all()
    assert got["not_number"].sum() == 0 and got["overflow"].sum() == 0
    assert (got["kept_locs"] == r.all_packed[np.repeat(r.lo < 0, np.diff(r.all_off))]).all()
    # the queries: a NONE term on a number leaves the lines whose "size " is no number; an ALL term that keeps nothing empties its query
    per = r.per_query(T)
    assert len(per[2]) == 0 and len(per[3]) == 0 and len(per[4]) == 0 and len(per[6]) == 14 and len(per[1]) > 0


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    names = ("fmx_hits_in_number_range_scratch_bytes", "fmx_hits_in_number_range_dev", "fmx_match_query_number_batch",
             "fmx_match_query_number_class_batch")
    for name in names:
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("size 12 is long\nsize 7 and one more line\n", 4, True, device=None)
    lens, hit_off, ids = np.array([5, 2, 1], np.int32), np.zeros(4, np.int64), np.zeros(8, np.int32)
    lo, hi = np.array([0, -1, 5], np.int64), np.array([9, -1, 2], np.int64)
    out = np.full(64, SENT, np.int64)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def dcall(h=fm._h, n=3, tl=lens, lo_=lo, hi_=hi, F=0, hoff=hit_off, locs=ids, n_hits=2, koff=out, klocs=out):
        return ia.lib.fmx_hits_in_number_range_dev(h, n, p(tl), p(lo_), p(hi_), F, p(hoff), p(locs), n_hits, p(koff), p(klocs), p(out), p(out), p(out),
                                                   None, None, 0, None)

    assert dcall() == E_NO_DEVICE and dcall(n_hits=0) == E_NO_DEVICE
    for bad in (dict(h=None), dict(n=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(locs=None), dict(koff=None), dict(klocs=None),
                dict(tl=None), dict(lo_=None), dict(hi_=None), dict(tl=np.array([5, -1, 1], np.int32)), dict(F=-1), dict(F=10)):
        assert dcall(**bad) == E_ARG, bad
    assert (out == SENT).all()
    sb = ia.lib.fmx_hits_in_number_range_scratch_bytes
    assert sb(0, 5) == 0 and sb(5, 0) == 0 and sb(5, 1 << 31) == 0 and sb(-1, 5) == 0
    # per slot: the window's 64 bytes, pattern and range 12, offsets 16, the extract's status 4, flags and scans 24
    assert sb(3, 1000) >= (64 + 12 + 16 + 4 + 24) * 1000 and sb(3, 1000) % 256 == 0 and sb(3, 1000) < 400 * 1000
    # the host forms
    ch, off = ia.pack_patterns(["size ", "is", "line"])
    off = off.astype(np.int32)
    qoff, kinds = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.uint8)
    small = np.full(3, SENT, np.int32)
    buf = np.zeros(1, np.int64)

    def host(h=fm._h, off_=off, n=3, lo_=lo, hi_=hi, F=0, qoff_=qoff, kinds_=kinds, q=2, loff=out, lines=buf):
        return ia.lib.fmx_match_query_number_batch(h, ch.ctypes.data, p(off_), n, p(lo_), p(hi_), F, p(qoff_), p(kinds_), q, 0, p(loff),
                                                   None if lines is None else lines.ctypes.data_as(ia._lib.C.POINTER(ia._lib.C.c_void_p)), p(small),
                                                   p(small), p(small), p(small), p(small), p(small))

    assert host() == E_NO_DEVICE and host(lo_=None, hi_=None) == E_NO_DEVICE
    for bad in (dict(h=None), dict(n=-1), dict(q=-1), dict(lo_=None), dict(hi_=None), dict(F=-1), dict(F=10), dict(qoff_=None), dict(kinds_=None),
                dict(loff=None), dict(lines=None), dict(qoff_=np.array([1, 2, 3], np.int32)), dict(kinds_=np.array([0, 3, 1], np.uint8)),
                dict(off_=np.array([0, 5, 4, 11], np.int32))):
        assert host(**bad) == E_ARG, bad
    assert (small == SENT).all() and (out == SENT).all() and buf[0] == 0
    alt, pos, pat = ia.pack_class_patterns([ia.ignore_case("size "), ia.ignore_case("is"), ia.ignore_case("line")])
    alt, pos, pat = np.ascontiguousarray(alt, np.uint16), np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(pat, np.int32)

    def chost(h=fm._h, max_ranges=16, lo_=lo, hi_=hi, F=0):
        return ia.lib.fmx_match_query_number_class_batch(h, p(alt), p(pos), len(pos) - 1, p(pat), 3, max_ranges, p(lo_), p(hi_), F, p(qoff), p(kinds), 2,
                                                         0, p(out), buf.ctypes.data_as(ia._lib.C.POINTER(ia._lib.C.c_void_p)), p(small), p(small),
                                                         p(small), p(small), p(small), p(small))

    assert chost() == E_NO_DEVICE and chost(lo_=None, hi_=None) == E_NO_DEVICE
    for bad in (dict(h=None), dict(max_ranges=0), dict(max_ranges=1025), dict(lo_=None), dict(hi_=None), dict(F=10)):
        assert chost(**bad) == E_ARG, bad
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    assert dcall(h=sa._h) == E_ARG and host(h=sa._h) == E_ARG and chost(h=sa._h) == E_ARG
    assert (small == SENT).all() and (out == SENT).all() and buf[0] == 0
    fm.close()

"""Statistics of the number behind a pattern, by the value of a field of the same line, per bucket of lines
(fmx_numbers_by_key_buckets_dev, fmx_number_stats_by_histogram_batch; timechart p95(latency_ms=) by status=) on the CPU: the
per-item functions of index4j_amd/csrc/fmx_by_hist.hpp — with those of fmx_value_hist.hpp, fmx_hit_by.hpp and fmx_hit_numbers.hpp —
compiled for the host and driven by a mirror of the stage (tests/by_hist_hostsim.cpp, a stand-alone program that also checks every
cell hit by hit in 128-bit arithmetic), which is additionally built with -fsanitize=address,undefined and run as such, as a program.

The judge is Python over the oracle (judge_by_hist): Where's kept hits with the span of the edges as window, judge_by's stages a
and b and its rows (tests/test_number_stats_by_cpu.py), parse_number over the oracle's windows and pct_of
(tests/test_number_stats_cpu.py), then plain Python per cell; it asserts the five invariants of the call on itself.  On the edge
text a second, independent judge reads the text with regular expressions.  The GPU suite runs the kernels and the host forms
themselves (tests/test_gpu_number_stats_by_histogram.py, which shares the helpers below)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import judge_values
from test_field_values_where_cpu import EVERY_LINE, Where
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN
from test_match_lines_cpu import judge_table
from test_number_stats_by_cpu import EDGE_KEYS, EDGE_LINES, EDGE_NUMBERS, edge_text, judge_by
from test_number_stats_cpu import NAN, OVER, WINDOW, parse_number, pct_of

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
EDGES_EMPTY = np.array([500, 750, 750, 1000], np.int32)  # the middle bucket is empty
EDGES_HALVES = np.array([0, 1000, 2000], np.int32)


def span(edges):
    """the window of the filter: the span of the edges, or every line"""
    return EVERY_LINE if edges is None else (int(edges[0]), int(edges[-1]))


class ByHist:
    """the judge's answer: base (judge_by's, for the same window), n_groups (m), key_row_off (m + 1), key_row_group, key_row_lines,
    row_text (R strings), cell_off (n + 1), count, sums (Python ints), min, max, pct (the packed cells), no_key, not_number, overflow,
    kept (n), hits (n, B: the kept hits per bucket), B, P"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def rows(self, i=0):
        """[(value, lines, counts per bucket, sums per bucket)] of number pattern i, then the same for "other" as (None, None, ...)"""
        k, B = int(self.by_of[i]), self.B
        out = []
        for r in range(int(self.key_row_off[k + 1] - self.key_row_off[k]) + 1):
            a = int(self.cell_off[i]) + r * B
            named = r < self.key_row_off[k + 1] - self.key_row_off[k]
            kr = int(self.key_row_off[k]) + r
            out.append((self.row_text[kr] if named else None, int(self.key_row_lines[kr]) if named else None, self.count[a:a + B].tolist(),
                        self.sums[a:a + B]))
        return out

    def cell(self, i, r, b):
        return int(self.cell_off[i]) + r * self.B + b


def judge_by_hist(o, w, T, m, by_of, stop, max_len, edges=None, top=10, permille=(500, 950), frac_digits=0):
    """by the definition, over the KEPT hits of a Where whose patterns are m key patterns followed by n number patterns and whose
    window is the span of the edges"""
    assert tuple(w.window) == span(edges)
    base = judge_by(o, w, T, m, by_of, stop, max_len, permille, frac_digits)
    n, P = base.n, len(permille)
    T = np.asarray(T)
    by_of = np.asarray(by_of, np.int32)
    B = 1 if edges is None else len(edges) - 1
    groups = np.diff(base.val_off)
    # the key rows: the groups by descending lines, a stable sort
    key_row_off, key_row_group, key_row_lines, row_text, rank = [0], [], [], [], []
    for k in range(m):
        lines = base.lines[int(base.val_off[k]):int(base.val_off[k + 1])].tolist()
        order = sorted(range(len(lines)), key=lambda g: -lines[g])
        rows = order[:top]
        texts = base.strings(k)
        key_row_group += rows
        key_row_lines += [lines[g] for g in rows]
        row_text += [texts[g] for g in rows]
        key_row_off.append(key_row_off[-1] + len(rows))
        rk = [len(rows)] * len(lines)  # (every group that is no row: the pattern's own "other")
        for r, g in enumerate(rows):
            rk[g] = r
        rank.append(rk)
        assert key_row_lines[key_row_off[k]:] == sorted(lines, reverse=True)[:len(rows)]  # invariant 5
    key_row_off = np.array(key_row_off, np.int64)
    R_of = np.diff(key_row_off)
    cell_off = np.concatenate([[0], np.cumsum((R_of[by_of] + 1) * B)]).astype(np.int64) if n else np.zeros(1, np.int64)
    cells = int(cell_off[-1])
    # the numbers, hit by hit
    n_off = (w.kept_off[m:] - w.kept_off[m]).astype(np.int64)
    n_locs = w.kept_locs[int(w.kept_off[m]):]
    windows = judge_values(o, np.asarray(n_locs, np.int32), n_off, w.lens[m:], "", WINDOW)
    numbers = [parse_number(row[:ln].tolist(), frac_digits) for row, ln in zip(windows.rows, windows.lengths)]
    per = [[] for _ in range(cells)]
    no_key, nn, ov = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    hits, tails = np.zeros((n, B), np.int64), np.zeros((n, B), np.int64)
    for i in range(n):
        k = int(by_of[i])
        mine = base.first_lines[int(base.first_off[k]):int(base.first_off[k + 1])]
        for t in range(int(n_off[i]), int(n_off[i + 1])):
            L = int(np.searchsorted(T, n_locs[t], side="left"))
            b = 0 if edges is None else int(np.searchsorted(edges, L, side="right")) - 1
            assert 0 <= b < B and (edges is None or edges[b] <= L < edges[b + 1])  # (the filter's window: every kept hit has a bucket)
            hits[i, b] += 1
            at = int(np.searchsorted(mine, L))
            if at == len(mine) or mine[at] != L:
                no_key[i] += 1  # decided before the parse
                tails[i, b] += 1
            elif numbers[t] is NAN:
                nn[i] += 1
                tails[i, b] += 1
            elif numbers[t] is OVER:
                ov[i] += 1
                tails[i, b] += 1
            else:
                g = int(base.group_of_first[int(base.first_off[k]) + at])
                per[int(cell_off[i]) + rank[k][g] * B + b].append(numbers[t])
    count = np.array([len(p) for p in per], np.int32)
    sums = [sum(p) for p in per]
    vmin = np.array([min(p) if p else 0 for p in per], np.int64)
    vmax = np.array([max(p) if p else 0 for p in per], np.int64)
    pct = np.array([[pct_of(sorted(p), pm) for pm in permille] for p in per], np.int64).reshape(cells, P)
    kept = w.kept[m:]
    for i in range(n):
        k, c0 = int(by_of[i]), int(cell_off[i])
        R = int(R_of[k])
        mine = count[c0:int(cell_off[i + 1])].reshape(R + 1, B)
        assert mine.sum() + no_key[i] + nn[i] + ov[i] == kept[i]  # invariant 1
        assert (mine.sum(axis=0) + tails[i] == hits[i]).all()  # invariant 4 (the hits histogram of the same call)
        assert (no_key[i], nn[i], ov[i]) == (base.no_key[i], base.not_number[i], base.overflow[i])
        # invariants 2 and 3: a row's cells over b are number_stats_by's row of that group for the same window; the rest is "other"
        r0 = int(base.row_off[i])
        named = set()
        for r in range(R):
            g = key_row_group[int(key_row_off[k]) + r]
            named.add(g)
            cs = range(c0 + r * B, c0 + (r + 1) * B)
            assert sum(int(count[c]) for c in cs) == base.count[r0 + g] and sum(sums[c] for c in cs) == base.sums[r0 + g]
            full = [c for c in cs if count[c]]
            assert min((int(vmin[c]) for c in full), default=0) == base.min[r0 + g] and max((int(vmax[c]) for c in full), default=0) == base.max[r0 + g]
            if B == 1:
                assert (pct[c0 + r] == base.pct[r0 + g]).all()
        rest = [g for g in range(int(groups[k])) if g not in named]
        cs = range(c0 + R * B, c0 + (R + 1) * B)
        assert sum(int(count[c]) for c in cs) == sum(int(base.count[r0 + g]) for g in rest)
        assert sum(sums[c] for c in cs) == sum(base.sums[r0 + g] for g in rest)
        assert rest or not any(count[c] for c in cs)  # top >= G_k: "other" is zero
    return ByHist(base=base, m=m, n=n, B=B, P=P, by_of=by_of, n_groups=groups.astype(np.int32), key_row_off=key_row_off,
                  key_row_group=np.array(key_row_group, np.int32), key_row_lines=np.array(key_row_lines, np.int32), row_text=row_text,
                  cell_off=cell_off, count=count, sums=sums, min=vmin, max=vmax, pct=pct, no_key=no_key, not_number=nn, overflow=ov, kept=kept,
                  key_kept=w.kept[:m], hits=hits)


def check_by_hist(got, want, what):
    """got: a dict of arrays under the judge's names, each of the answer's size (sum_lo / sum_hi for sums)"""
    for name in ("key_row_off", "key_row_group", "key_row_lines", "cell_off", "count", "min", "max", "no_key", "not_number", "overflow"):
        g, e = np.asarray(got[name]), np.asarray(getattr(want, name))
        assert g.shape == e.shape and (g == e).all(), "%s: %s %r, expected %r" % (what, name, g[:8], e[:8])
    sums = [(int(hi) << 64) | int(lo) for lo, hi in zip(np.asarray(got["sum_lo"], np.uint64), np.asarray(got["sum_hi"], np.uint64))]
    assert sums == want.sums, what + ": sums"
    assert (np.asarray(got["pct"]).reshape(len(want.count), want.P) == want.pct).all(), what + ": percentiles"


_JUDGED = {}


def judged(tag, o, T, keys, numbers, by_of, stop, max_len, edges=None, top=10, queries=(), key_where=None, where=None, permille=(500, 950),
           frac_digits=0):
    """(Where, ByHist) of a case, judged once per session and shared by the tests that need it (left unchanged)"""
    key = (tag, tuple(keys), tuple(numbers), tuple(by_of), stop, max_len, None if edges is None else tuple(int(e) for e in edges), top, repr(queries),
           repr(key_where), repr(where), tuple(permille), frac_digits)
    if key not in _JUDGED:
        m = len(keys)
        where_of = list(key_where or [-1] * m) + list(where or [-1] * len(numbers))
        w = Where(tag, o, T, list(keys) + list(numbers), list(queries), where_of, span(edges))
        _JUDGED[key] = (w, judge_by_hist(o, w, T, m, by_of, stop, max_len, edges, top, permille, frac_digits))
    return _JUDGED[key]


# ---- the mirror ----
_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "by_hist_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "by_hist_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("by_hist_hostsim")


def run_hostsim(simdir, text, w, want, T, edges, top, permille=(500, 950), frac_digits=0, lead=0, extra_hits=0, max_fences=4096, sanitize=False):
    """the stage's mirror over the KEPT number hits of a Where, the judge's stages a and b and the text itself.  lead: slots in
    front of the block that hold no hit (hit_off[0] = lead); extra_hits: slots behind it"""
    m, n, base = want.m, want.n, want.base
    chars = ia.as_chars(text)
    hit_off = (w.kept_off[m:] - w.kept_off[m] + lead).astype(np.int64)
    locs = np.concatenate([np.full(lead, -5, np.int32), w.kept_locs[int(w.kept_off[m]):], np.full(extra_hits, -5, np.int32)]).astype(np.int32)
    pm = np.asarray(permille, np.int32)
    e = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32)
    head = np.array([m, n, len(locs), len(T), max_fences, len(e), top, len(pm), frac_digits, len(chars), len(base.first_lines), len(base.lines)], np.int64)
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (head, np.asarray(T, np.int32), np.asarray(w.lens[m:], np.int32), np.asarray(want.by_of, np.int32), hit_off, locs, e, pm,
                  base.first_off.astype(np.int64), base.first_lines.astype(np.int32), base.group_of_first.astype(np.int32),
                  base.val_off.astype(np.int64), np.asarray(base.lines, np.int32), chars.astype(np.uint16)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), "run", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.uint8)
    at = 0

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += count * np.dtype(dtype).itemsize
        return out

    got = dict(key_row_off=take(np.int64, m + 1))
    R = int(got["key_row_off"][m])
    got.update(key_row_group=take(np.int32, R), key_row_lines=take(np.int32, R), cell_off=take(np.int64, n + 1))
    cells, P = int(got["cell_off"][n]), len(pm)
    got.update(count=take(np.int32, cells), sum_lo=take(np.uint64, cells), sum_hi=take(np.uint64, cells), min=take(np.int64, cells),
               max=take(np.int64, cells), pct=take(np.int64, cells * P), no_key=take(np.int32, n), not_number=take(np.int32, n),
               overflow=take(np.int32, n))
    assert at == len(raw)
    return got


def sim_case(simdir, text, tag, o, T, keys, numbers, by_of, stop, max_len, edges=None, top=10, queries=(), key_where=None, where=None,
             permille=(500, 950), frac_digits=0, **kw):
    w, want = judged(tag, o, T, keys, numbers, by_of, stop, max_len, edges, top, queries, key_where, where, permille, frac_digits)
    got = run_hostsim(simdir, text, w, want, T, edges, top, permille, frac_digits, **kw)
    check_by_hist(got, want, "%s %r by %r top %d" % (tag, numbers, keys, top))
    return want


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


@pytest.fixture(scope="module")
def edge():
    text = edge_text()
    o = orc.OracleFmIndex(text, 8, True)
    return text, o, judge_table(o, "\n")


def test_per_item_functions(simdir):
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]


# the issue's figures (plain Python over the fixture's text gave them); the JUDGE decides
FSN, PKT, XCV = "dfs.FSNamesystem", "dfs.DataNode$PacketResponder", "dfs.DataNode$DataXceiver"
FSN_COUNTS, PKT_COUNTS, REST_COUNTS = [27, 10, 32, 19, 32, 28, 24, 32], [33, 6, 29, 14, 22, 24, 31, 23], [21, 7, 16, 7, 10, 18, 9, 11]


def assert_fixture_figures(get):
    """get(number pattern, key pattern, stop, edges, top, where) -> something with rows(0) = [(value, lines, counts, sums)] + other,
    n_groups, kept, no_key, not_number, and min / pct by cell(i, r, b)"""
    a = get("size ", "INFO ", " :", EDGES_250, 2, None)
    assert (int(a.n_groups[0]), int(a.kept[0]), int(a.no_key[0]), int(a.not_number[0])) == (356, 608, 0, 123)
    rows = a.rows(0)
    assert [(v, ln, c, sum(c), sum(s)) for v, ln, c, s in rows] == [
        (FSN, 525, FSN_COUNTS, 204, 13_074_465_816), (PKT, 480, PKT_COUNTS, 182, 11_681_158_219), (None, None, REST_COUNTS, 99, 6_337_250_623)]
    assert int(a.min[a.cell(0, 0, 6)]) == 2 and rows[0][3][0] == 1_811_939_328
    assert all(int(a.pct[c][0]) == 67_108_864 for c in range(len(a.count)) if a.count[c])  # every p50 of a non-empty cell
    b = get("size ", "INFO ", " :", None, 3, None)
    rows = b.rows(0)
    assert [(v, ln, c) for v, ln, c, _ in rows] == [(FSN, 525, [204]), (PKT, 480, [182]), (XCV, 283, [0]), (None, None, [99])]
    c = get("size ", " from /10.", ".", EDGES_250, 1, None)
    assert (int(c.no_key[0]), int(c.not_number[0])) == (386, 47)
    assert [(v, ln, cn, sum(cn), sum(s)) for v, ln, cn, s in c.rows(0)] == [
        ("251", 181, [30, 5, 27, 10, 15, 19, 19, 14], 139, 9_066_835_001), (None, None, [6, 1, 4, 4, 5, 7, 5, 4], 36, 2_250_162_971)]
    c5 = get("size ", " from /10.", ".", EDGES_250, 5, None).rows(0)
    assert len(c5) == 3 and (c5[1][0], c5[1][1]) == ("250", 41) and sum(c5[2][2]) == 0
    d = get("blk_", "INFO ", " :", EDGES_HALVES, 2, None)
    assert (int(d.no_key[0]), int(d.not_number[0])) == (80, 1195)
    rows = d.rows(0)
    assert [(v, cn) for v, _, cn, _ in rows] == [(FSN, [125, 236]), (PKT, [111, 137]), (None, [281, 303])]
    assert rows[0][3] == [564_741_097_690_755_251_057, 1_120_940_049_190_542_864_522] and min(rows[0][3]) > 2 ** 64
    e = get("size ", "INFO ", " :", EDGES_250, 2, dict(all=["addStoredBlock"]))
    assert (int(e.n_groups[0]), int(e.kept[0]), int(e.not_number[0])) == (60, 314, 60)
    rows = e.rows(0)
    assert [(v, ln, cn, sum(cn)) for v, ln, cn, _ in rows[:2]] == [(FSN, 247, FSN_COUNTS, 204), ("", 9, [0, 0, 0, 0, 2, 2, 2, 1], 7)]
    assert sum(rows[2][2]) == 43
    g = get("size ", "INFO ", " :", EDGES_EMPTY, 2, None)
    assert (int(g.n_groups[0]), int(g.kept[0]), int(g.not_number[0])) == (90, 154, 37)
    assert [(v, cn) for v, _, cn, _ in g.rows(0)] == [(FSN, [32, 0, 19]), (PKT, [29, 0, 14]), (None, [16, 0, 7])]


def test_fixture_figures(simdir, hd):
    """the issue's figures on the judge's answer, each case also through the mirror of the stage"""
    o, T = hd

    def get(number, key, stop, edges, top, where):
        return sim_case(simdir, HD, "hd16 byhist", o, T, [key], [number], [0], stop, 32, edges, top, queries=[where] if where else (),
                        key_where=[0] if where else None, where=[0] if where else None)

    assert_fixture_figures(get)


def test_tops_shared_keys_and_packed_blocks(simdir, hd):
    """top below, at and above G_k, a top that cuts through a run of equal lines; two key patterns with different G_k and three number
    patterns of which two share a key; every edge shape; slots in front of and behind the block; few fences; 0 and 16 percentiles"""
    o, T = hd
    cut = sim_case(simdir, HD, "hd16 byhist", o, T, ["INFO "], ["size "], [0], " :", 32, EDGES_250, 300)
    tail = cut.key_row_lines[-120:]
    assert len(cut.key_row_lines) == 300 and tail[0] == tail[-1] == 1  # the cut runs through the groups with one line
    assert (np.diff(cut.key_row_group[-120:]) > 0).all()  # ... which stay in value order
    for top in (1, 355, 356, 357, 65536):
        want = sim_case(simdir, HD, "hd16 byhist", o, T, ["INFO "], ["size "], [0], " :", 32, None, top)
        assert len(want.key_row_lines) == min(top, 356)
    for edges, kw in ((None, dict(lead=3, extra_hits=70)), (EDGES_250, dict(max_fences=16)), (EDGES_UNEVEN, dict(lead=3, extra_hits=70, max_fences=8)),
                      (EDGES_EMPTY, {}), (EDGES_BEYOND, dict(lead=1030, extra_hits=1))):
        want = sim_case(simdir, HD, "hd16 byhist", o, T, ["INFO ", " from /10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, edges, 5,
                        permille=(0, 500, 1000), **kw)
        assert want.key_row_off.tolist()[1] == 5 and want.key_row_off[2] - 5 == min(5, int(want.n_groups[1]))
        assert (want.count[int(want.cell_off[0]):int(want.cell_off[1])] == sim_case(
            simdir, HD, "hd16 byhist", o, T, ["INFO "], ["size "], [0], " :.", 16, edges, 5, permille=(0, 500, 1000)).count).all()
    sim_case(simdir, HD, "hd16 byhist", o, T, [" from /10.", "INFO "], ["blk_", "size "], [1, 0], " :.", 16, EDGES_250, 3, permille=())
    sim_case(simdir, HD, "hd16 byhist", o, T, ["INFO "], ["src: /10."], [0], " :", 32, EDGES_250, 4, permille=tuple(range(0, 1000, 63)), frac_digits=3)


def regex_line(text, at, line, key, number, stop, max_len, frac_digits):
    """one line by `re`: (the key's value or None, the numbers that parse, no_key, not_number, overflow); at: where the line starts
    in the text (a window may run past the line's end)"""
    k = line.find(key)
    value = None
    if k >= 0:
        window = text[at + k + len(key):at + k + len(key) + max_len]
        value = re.match("[^%s]*" % re.escape(stop), window, re.S).group() if stop else window
    numbers, no_key, nn, ov = [], 0, 0, 0
    for hit in re.finditer("(?=%s)" % re.escape(number), line):
        v = parse_number([ord(c) for c in text[at + hit.start() + len(number):at + hit.start() + len(number) + WINDOW]], frac_digits)
        if value is None:
            no_key += 1
        elif v is NAN:
            nn += 1
        elif v is OVER:
            ov += 1
        else:
            numbers.append(v)
    return value, numbers, no_key, nn, ov


def regex_by_hist(text, key, number, stop, max_len, edges, top, frac_digits=0):
    """the independent judge: [(value, lines, [numbers per bucket])] of the key rows, other's numbers per bucket, (no_key,
    not_number, overflow) and the number of groups — every line and every hit by `re`, only the lines inside the edges' span"""
    B = 1 if edges is None else len(edges) - 1
    lo, hi = span(edges)
    groups, per_line, at = {}, [], 0
    for L, line in enumerate(text.split("\n")):
        if lo <= L < hi:
            value, numbers, no_key, nn, ov = regex_line(text, at, line, key, number, stop, max_len, frac_digits)
            b = 0 if edges is None else int(np.searchsorted(edges, L, side="right")) - 1
            per_line.append((value, numbers, b))
            if value is not None:
                groups[value] = groups.get(value, 0) + 1
            per_line[-1] += (no_key, nn, ov)
        at += len(line) + 1
    values = sorted(groups, key=lambda v: [ord(c) for c in v])
    order = sorted(values, key=lambda v: -groups[v])[:top]  # (a stable sort of the values in value order)
    rows = {v: [[] for _ in range(B)] for v in order}
    other = [[] for _ in range(B)]
    tails = [0, 0, 0]
    for value, numbers, b, no_key, nn, ov in per_line:
        tails = [tails[0] + no_key, tails[1] + nn, tails[2] + ov]
        if value is not None:
            (rows[value] if value in rows else other)[b].extend(numbers)
    return [(v, groups[v], rows[v]) for v in order], other, tuple(tails), len(values)


def assert_regex(want, i, k, text, key, number, stop, max_len, edges, top, frac_digits=0):
    """the judge's answer for number pattern i by key pattern k equals the regular expressions'"""
    rows, other, tails, G = regex_by_hist(text, key, number, stop, max_len, edges, top, frac_digits)
    mine = want.rows(i)
    assert int(want.n_groups[k]) == G and len(mine) == len(rows) + 1
    for (value, lines, counts, sums), (v, ln, per) in zip(mine, rows):
        assert (value, lines, counts, sums) == (v, ln, [len(p) for p in per], [sum(p) for p in per]), v
    assert (mine[-1][2], mine[-1][3]) == ([len(p) for p in other], [sum(p) for p in other])
    assert (int(want.no_key[i]), int(want.not_number[i]), int(want.overflow[i])) == tails


def test_edge_text(simdir, edge):
    """the edge text against both judges, through the mirror: tops, edges that cut groups, number patterns without a hit, a key
    pattern without a hit, fractions"""
    text, o, T = edge
    assert len(T) == EDGE_LINES - 1
    thirds = np.array([0, 1000, 2000, 3000], np.int32)
    odd = np.array([5, 6, 6, 13, 150, 2101, 2999], np.int32)
    for edges, top, stop in ((None, 3, " \n"), (thirds, 7, " \n"), (odd, 8, " \n"), (thirds, 100, " "), (odd, 1, " \n")):
        want = sim_case(simdir, text, "edge byhist", o, T, EDGE_KEYS, EDGE_NUMBERS, [0, 0, 0], stop, 32, edges, top, permille=(0, 500, 950, 1000))
        assert_regex(want, 0, 0, text, "k=", "n=", stop, 32, edges, top)
        assert_regex(want, 2, 0, text, "k=", "m=", stop, 32, edges, top)
        assert want.kept[1] == 0 and want.cell_off[2] - want.cell_off[1] == want.cell_off[1]  # the pattern without a hit still has its cells
    for F in (0, 3, 9):
        want = sim_case(simdir, text, "edge byhist", o, T, EDGE_KEYS, EDGE_NUMBERS, [3, 1, 2], " \n", 32, thirds, 4, permille=(500,), frac_digits=F)
        assert_regex(want, 2, 2, text, "c=", "m=", " \n", 32, thirds, 4, F)
        assert_regex(want, 1, 1, text, "id=", "zzq#", " \n", 32, thirds, 4, F)
        assert want.no_key[0] == want.kept[0] > EDGE_LINES and want.cell_off[1] == 3  # "zq#" has no hit: one row, "other", of zeros
        assert want.n_groups.tolist() == [want.n_groups[0], EDGE_LINES, 1, 0] and want.key_row_off.tolist()[1:] == [4, 8, 9, 9]
    frac = sim_case(simdir, text, "edge byhist", o, T, ["k="], ["n="], [0], " \n", 32, odd, 6, frac_digits=3)
    assert_regex(frac, 0, 0, text, "k=", "n=", " \n", 32, odd, 6, 3)


def test_edge_text_filters(simdir, edge):
    """a filter that keeps no number hit (the key rows with zero cells), key_where_of different from where_of"""
    text, o, T = edge
    thirds = np.array([0, 1000, 2000, 3000], np.int32)
    q = [dict(all=["nokey"]), dict(all=["k=far"]), dict(all=["only"])]
    empty = sim_case(simdir, text, "edge byhist", o, T, ["k="], ["n="], [0], " \n", 32, thirds, 5, queries=q, key_where=[-1], where=[2])
    assert empty.kept[0] == 0 and len(empty.key_row_lines) == 5 and sum(empty.count) == 0
    mixed = sim_case(simdir, text, "edge byhist", o, T, ["k="], ["n="], [0], " \n", 32, thirds, 5, queries=q, key_where=[1], where=[-1])
    assert mixed.row_text == ["far"] and mixed.rows(0)[0][2:] == ([1, 0, 1], [100, 0, 2100]) and mixed.no_key[0] == mixed.kept[0] - 2


def test_sanitized_build(simdir, hd, edge):
    """the mirror under AddressSanitizer and UndefinedBehaviorSanitizer, as a program"""
    o, T = hd
    sim_case(simdir, HD, "hd16 byhist", o, T, ["INFO ", " from /10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, EDGES_UNEVEN, 5,
             permille=(0, 500, 1000), lead=5, extra_hits=1030, max_fences=8, sanitize=True)
    sim_case(simdir, HD, "hd16 byhist", o, T, ["INFO "], ["size "], [0], " :", 32, None, 300, sanitize=True)
    text, eo, eT = edge
    sim_case(simdir, text, "edge byhist", eo, eT, EDGE_KEYS, EDGE_NUMBERS, [3, 1, 2], " \n", 32, np.array([0, 1000, 2000, 3000], np.int32), 4,
             permille=(500,), frac_digits=9, sanitize=True)


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols and methods); every refusal of a HOST array comes before the handle
    is asked for its device, and a refused call stores nothing"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_numbers_by_key_buckets_scratch_bytes", "fmx_numbers_by_key_buckets_dev", "fmx_number_stats_by_histogram_batch",
                 "fmx_number_stats_by_histogram_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    assert hasattr(ia.FmIndex, "number_stats_by_histogram")
    fm = ia.FmIndex("k=a n=1\nk=b n=2\n", 4, True, device=None)
    keys, numbers, none = ia.pack_patterns([ia.as_chars("k=")]), ia.pack_patterns([ia.as_chars("n=")]), ia.pack_patterns([])

    def call(by_of=(0,), stop=" \n", max_len=8, permille=(500,), frac_digits=0, keys=keys, where_of=(-1,), edges=None, top=3):
        try:
            fm.number_stats_by_histogram_batch(*keys, *numbers, by_of, *none, [0], [], [-1] * (len(keys[1]) - 1), where_of, stop, max_len, edges, top,
                                               permille, frac_digits)
        except ia.FmxError as e:
            return e.code, str(e)
        return 0, ""

    assert call()[0] == E_NO_DEVICE
    for kw, word in ((dict(by_of=(1,)), "by_of[0]"), (dict(by_of=(-1,)), "by_of[0]"), (dict(keys=none), "m == 0"), (dict(max_len=0), "max_len"),
                     (dict(max_len=65), "max_len"), (dict(stop="x" * 65), "stop set"), (dict(frac_digits=10), "frac_digits"),
                     (dict(frac_digits=-1), "frac_digits"), (dict(permille=(1001,)), "permille"), (dict(permille=tuple(range(17))), "n_permille"),
                     (dict(where_of=(0,)), "where_of"), (dict(top=0), "top"), (dict(top=65537), "top"),
                     (dict(edges=np.arange(2 ** 27 // 4 + 2, dtype=np.int32)), "2^27 cells"),
                     (dict(edges=np.arange(2 ** 27 // 8 + 1, dtype=np.int32), permille=(1, 2, 3)), "2^27 percentiles")):
        code, msg = call(**kw)
        assert code == E_ARG and word in msg, (kw, code, msg)
    # bad edges: handed to the library as they are (the Python layer would refuse them first)
    i32, i64 = np.int32, np.int64
    SENT = -0x3C3C3C3D
    for edges in ([0], [3, 2], [-1, 4]):
        e = np.array(edges, i32)
        kch, koff = keys
        nch, noff = numbers
        koff, noff = koff.astype(i32), noff.astype(i32)
        zero_off, by_of, wo, pm, stop = np.zeros(1, i32), np.zeros(1, i32), np.full(1, -1, i32), np.array([500], i32), ia.as_chars(" \n")
        outs = [np.full(k, SENT, t) for k, t in ((1, i32), (2, i64), (2, i64))] + [np.full(1, SENT, i32) for _ in range(9)]
        n_groups, key_row_off, cell_off = outs[:3]
        ptr = [C.c_void_p(0x1234) for _ in range(10)]
        rc = ia.lib.fmx_number_stats_by_histogram_batch(fm._h, kch.ctypes.data, koff.ctypes.data, 1, nch.ctypes.data, noff.ctypes.data, 1, by_of.ctypes.data,
                                                        None, zero_off.ctypes.data, 0, zero_off.ctypes.data, None, 0, wo.ctypes.data, wo.ctypes.data,
                                                        e.ctypes.data, len(e), 3, stop.ctypes.data, len(stop), 8, 0, pm.ctypes.data, 1,
                                                        n_groups.ctypes.data, key_row_off.ctypes.data, *(C.byref(x) for x in ptr[:4]),
                                                        cell_off.ctypes.data, *(C.byref(x) for x in ptr[4:]), *(a.ctypes.data for a in outs[3:]), None)
        assert rc == E_ARG, edges
        assert all((a == SENT).all() for a in outs) and all(x.value == 0x1234 for x in ptr)  # a refused call stores nothing
    size = ia.lib.fmx_numbers_by_key_buckets_scratch_bytes
    assert size(0, 1, 10, 1000, 0, 2) == 0 and size(1, 0, 10, 1000, 0, 2) == 0 and size(1, 1, 10, 1000, 1, 2) == 0 and size(1, 1, 10, 1000, 0, 17) == 0
    assert size(1, 1, 10, 2 ** 31, 0, 2) == 0 and size(1, 1, 2 ** 31, 1000, 0, 2) == 0
    assert size(3, 2, 10, 1000, 9, 2) > ia.lib.fmx_numbers_by_key_scratch_bytes(3, 1000, 2) and size(3, 2, 10, 0, 9, 2) > 0  # (no number hit: the ranks)
    fm.close()

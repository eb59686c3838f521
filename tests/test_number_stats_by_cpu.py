"""Statistics of the number behind a pattern, grouped by the value of a field of the same line (fmx_first_hits_of_lines_dev,
fmx_values_of_hits_groups_dev, fmx_numbers_by_key_dev, fmx_number_stats_by_batch; stats count, sum(bytes=), p95(latency_ms=) by
status=) on the CPU: the per-item functions of index4j_amd/csrc/fmx_hit_by.hpp — with those of fmx_hit_values.hpp and
fmx_hit_numbers.hpp — compiled for the host and driven by a mirror of the three stages (tests/by_key_hostsim.cpp, a stand-alone
program), which is additionally built with -fsanitize=address,undefined and run as such, as a program.

The judge is Python over the oracle (judge_by): Where's kept hits (tests/test_field_values_where_cpu.py) of the key patterns and the
number patterns in ONE block; per key pattern the first kept hit of every line by numpy over the line table; judge_values'
windows and values over those hits (tests/test_field_values_cpu.py); parse_number over the oracle's windows of the number hits
(tests/test_number_stats_cpu.py); then plain Python per (pattern, group).  On the edge text a second, independent judge reads the
text with regular expressions.  The GPU suite runs the kernels and the host forms themselves (tests/test_gpu_number_stats_by.py,
which shares the helpers below)."""
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
from test_match_lines_cpu import judge_table
from test_number_stats_cpu import NAN, OVER, WINDOW, parse_number, pct_of

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
WS = " \t\r\n"


class By:
    """the judge's answer: first_off / first_lines / first_locs / group_of_first (stages a and b), val_off, lines, text_off, chars
    (the groups), row_off, count, sums (Python ints), min, max, pct (the packed rows), no_key, not_number, overflow, kept (n)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def strings(self, k=0):
        return [self.chars[self.text_off[g]:self.text_off[g + 1]].tobytes().decode("utf-16-le", "surrogatepass")
                for g in range(int(self.val_off[k]), int(self.val_off[k + 1]))]

    def row(self, i, value, k=None):
        """(count, sum, min, max) of number pattern i in the group of that value of its key pattern"""
        k = int(self.by_of[i]) if k is None else k
        r = int(self.row_off[i]) + self.strings(k).index(value)
        return int(self.count[r]), self.sums[r], int(self.min[r]), int(self.max[r])

    def lines_of(self, value, k=0):
        return int(self.lines[int(self.val_off[k]) + self.strings(k).index(value)])


def judge_by(o, w, T, m, by_of, stop, max_len, permille=(500, 950), frac_digits=0):
    """by the definition, over the KEPT hits of a Where whose patterns are m key patterns followed by n number patterns"""
    n, P = w.n - m, len(permille)
    by_of = np.asarray(by_of, np.int32)
    T = np.asarray(T)
    first_lines, first_locs, first_off = [], [], [0]
    for k in range(m):  # the hit with the smallest position on every line, the lines ascending
        h = np.sort(w.kept_locs[w.kept_off[k]:w.kept_off[k + 1]])
        u, idx = np.unique(np.searchsorted(T, h, side="left"), return_index=True)
        first_lines.append(u.astype(np.int32))
        first_locs.append(h[idx].astype(np.int32))
        first_off.append(first_off[-1] + len(u))
    first_off = np.array(first_off, np.int64)
    all_lines = np.concatenate(first_lines + [np.zeros(0, np.int32)]).astype(np.int32)
    all_locs = np.concatenate(first_locs + [np.zeros(0, np.int32)]).astype(np.int32)
    vals = judge_values(o, all_locs, first_off, w.lens[:m], stop, max_len)
    # the group of every first hit: its value among the sorted values of its pattern
    stop_units = set(ia.as_chars(stop).tolist())
    group_of_first = np.zeros(len(all_locs), np.int32)
    for k in range(m):
        index = {v: g for g, (v, _) in enumerate(vals.per[k])}
        for t in range(int(first_off[k]), int(first_off[k + 1])):
            units = vals.rows[t][:int(vals.lengths[t])].tolist()
            cut = next((j for j, u in enumerate(units) if u in stop_units), len(units))
            group_of_first[t] = index[tuple(units[:cut])]
    # the numbers
    n_off = (w.kept_off[m:] - w.kept_off[m]).astype(np.int64)
    n_locs = w.kept_locs[int(w.kept_off[m]):]
    windows = judge_values(o, np.asarray(n_locs, np.int32), n_off, w.lens[m:], "", WINDOW)
    numbers = [parse_number(row[:ln].tolist(), frac_digits) for row, ln in zip(windows.rows, windows.lengths)]
    groups = np.diff(vals.val_off)
    row_off = np.concatenate([[0], np.cumsum(groups[by_of])]).astype(np.int64) if n else np.zeros(1, np.int64)
    R = int(row_off[-1])
    per = [[] for _ in range(R)]
    no_key, nn, ov = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        k = int(by_of[i])
        mine = first_lines[k]
        for t in range(int(n_off[i]), int(n_off[i + 1])):
            L = int(np.searchsorted(T, n_locs[t], side="left"))
            at = int(np.searchsorted(mine, L))
            if at == len(mine) or mine[at] != L:
                no_key[i] += 1  # decided before the parse
            elif numbers[t] is NAN:
                nn[i] += 1
            elif numbers[t] is OVER:
                ov[i] += 1
            else:
                per[int(row_off[i]) + int(group_of_first[int(first_off[k]) + at])].append(numbers[t])
    count = np.array([len(p) for p in per], np.int32)
    sums = [sum(p) for p in per]
    vmin = np.array([min(p) if p else 0 for p in per], np.int64)
    vmax = np.array([max(p) if p else 0 for p in per], np.int64)
    pct = np.array([[pct_of(sorted(p), pm) for pm in permille] for p in per], np.int64).reshape(R, P)
    kept = w.kept[m:]
    for i in range(n):  # the invariant, on the judge itself
        assert count[row_off[i]:row_off[i + 1]].sum() + no_key[i] + nn[i] + ov[i] == kept[i]
    return By(m=m, n=n, P=P, by_of=by_of, first_off=first_off, first_lines=all_lines, first_locs=all_locs, group_of_first=group_of_first,
              val_off=vals.val_off, lines=vals.counts, text_off=vals.text_off, chars=vals.chars, row_off=row_off, count=count, sums=sums, min=vmin,
              max=vmax, pct=pct, no_key=no_key, not_number=nn, overflow=ov, kept=kept, key_kept=w.kept[:m])


def check_by(got, want, what, stages=False):
    """got: a dict of arrays under the judge's names, each of the answer's size (sum_lo / sum_hi for sums)"""
    for name in ("val_off", "lines", "text_off", "chars", "row_off", "count", "min", "max", "no_key", "not_number", "overflow") + (
            ("first_off", "first_lines", "first_locs", "group_of_first") if stages else ()):
        g, e = np.asarray(got[name]), np.asarray(getattr(want, name))
        assert g.shape == e.shape and (g == e).all(), "%s: %s %r, expected %r" % (what, name, g[:8], e[:8])
    sums = [(int(hi) << 64) | int(lo) for lo, hi in zip(np.asarray(got["sum_lo"], np.uint64), np.asarray(got["sum_hi"], np.uint64))]
    assert sums == want.sums, what + ": sums"
    assert (np.asarray(got["pct"]).reshape(len(want.count), want.P) == want.pct).all(), what + ": percentiles"


# ---- the edge text: about 3,000 lines, every case of the issue in one text ----
EDGE_LINES = 3000
EDGE_KEYS = ["k=", "id=", "c=", "zq#"]        # values of few groups; as many groups as lines; one group only; no hit at all
EDGE_NUMBERS = ["n=", "zzq#", "m="]           # a number pattern with no hit between two that have hits


def edge_text():
    special = {
        5: "id=5 c=x k=b mid k=a n=5 m=1",                 # two key hits: SA-row order a, b; by position b is first
        6: "id=6 c=x n=7 n=8 n=9 k=v1 m=2",                # three hits of one number pattern on one line
        10: "id=10 c=x n=77 nokey",                        # a number and no key of "k="
        11: "id=11 c=x n=abc n=12",                        # no key: the number that does not parse is no_key too, and only that
        12: "id=12 c=x k=v2 nothing",                      # a key and no number
        13: "id=13 c=x k=zz9 only",                        # a group of its own without a number: count 0
        14: "id=14 c=x k= n=4",                            # the empty key
        20: "id=20 c=x n=3 k=",                            # the key pattern ends the line: the window starts at the line feed
        21: "tail21 id=21 c=x n=21",                       # (what follows line 20's pattern without a line feed in the stop set)
        30: "id=30 c=x k=abcdX n=30", 31: "id=31 c=x k=abcdY n=31", 32: "id=32 c=x k=abcd n=32", 33: "id=33 c=x k=abcdefghX n=33",
        34: "id=34 c=x k=abcdefghY n=34",                  # keys that differ only behind a multiple of four code units
        40: "id=40 c=x k=v3 n=9223372036854775807 m=7",    # 2^63 - 1
        41: "id=41 c=x k=v3 n=9223372036854775808",        # overflow
        42: "id=42 c=x k=v3 n=1.5 n=0.123456789",          # fractions
        43: "id=43 c=x k=v3 n=x n=",                       # not numbers, on a line with a key
        50: "id=50 c=x k=ab n=50", 51: "id=51 c=x k=ab\0 n=51", 52: "id=52 c=x k=ab\0\0 n=52",  # a key against the same key and U+0000:
        53: "id=53 c=x k=ab n=53",                         # the padded chunk keys are equal, the length pass tells them apart
        100: "id=100 c=x k=far n=100", 2100: "id=2100 c=x k=far n=2100",   # one key 2,000 lines apart
        200: "id=200 c=x k=nb n=1", 201: "id=201 c=x k=nb n=2", 202: "id=202 c=x k=nb n=3",  # neighbouring lines with one key
    }
    lines = [special.get(i, "id=%d c=x k=v%d n=%d m=%d" % (i, i % 7, (i * 7919) % 100003, i % 11)) for i in range(EDGE_LINES - 1)]
    lines.append("id=%d c=x k=last n=42" % (EDGE_LINES - 1))  # the last line has no line feed behind it
    return "\n".join(lines)


def regex_judge(text, key, number, stop, max_len, frac_digits=0):
    """the independent judge: {value: [lines, [numbers]]}, no_key, not_number, overflow — every line and every hit by `re`"""
    groups, no_key, nn, ov = {}, 0, 0, 0
    at = 0
    for line in text.split("\n"):
        k = line.find(key)
        value = None
        if k >= 0:
            window = text[at + k + len(key):at + k + len(key) + max_len]
            value = re.match("[^%s]*" % re.escape(stop), window, re.S).group() if stop else window
            groups.setdefault(value, [0, []])[0] += 1
        for hit in re.finditer("(?=%s)" % re.escape(number), line):
            v = parse_number([ord(c) for c in text[at + hit.start() + len(number):at + hit.start() + len(number) + WINDOW]], frac_digits)
            if value is None:
                no_key += 1
            elif v is NAN:
                nn += 1
            elif v is OVER:
                ov += 1
            else:
                groups[value][1].append(v)
        at += len(line) + 1
    return groups, no_key, nn, ov


def assert_regex(want, i, k, text, key, number, stop, max_len, frac_digits=0):
    """the judge's answer for number pattern i by key pattern k equals the regular expressions'"""
    groups, no_key, nn, ov = regex_judge(text, key, number, stop, max_len, frac_digits)
    values = sorted(groups, key=lambda v: [ord(c) for c in v])
    assert want.strings(k) == values
    assert [want.lines_of(v, k) for v in values] == [groups[v][0] for v in values]
    for v in values:
        s = groups[v][1]
        assert want.row(i, v, k) == (len(s), sum(s), min(s, default=0), max(s, default=0)), v
    assert (int(want.no_key[i]), int(want.not_number[i]), int(want.overflow[i])) == (no_key, nn, ov)


# ---- the mirror ----
_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "by_key_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "by_key_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("by_key_hostsim")


def run_hostsim(simdir, text, w, T, m, by_of, stop, max_len, permille=(500, 950), frac_digits=0, lead=0, extra_hits=0, max_fences=4096, sanitize=False):
    """the three stages' mirror over the KEPT hits of a Where (m key patterns, then the number patterns) and the text itself.  lead:
    slots in front of the block that hold no hit (hit_off[0] = lead); extra_hits: slots behind it"""
    n = w.n - m
    chars = ia.as_chars(text)
    hit_off = (w.kept_off + lead).astype(np.int64)
    locs = np.concatenate([np.full(lead, -5, np.int32), w.kept_locs, np.full(extra_hits, -5, np.int32)]).astype(np.int32)
    stop_units, pm = ia.as_chars(stop), np.asarray(permille, np.int32)
    head = np.array([m, n, len(locs), len(T), max_fences, len(stop_units), max_len, len(pm), frac_digits, len(chars)], np.int64)
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (head, np.asarray(T, np.int32), np.asarray(w.lens, np.int32), np.asarray(by_of, np.int32), hit_off, locs, stop_units.astype(np.uint16), pm,
                  chars.astype(np.uint16)):
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

    got = dict(first_off=take(np.int64, m + 1))
    F = int(take(np.int64, 1)[0])
    got.update(first_lines=take(np.int32, F), first_locs=take(np.int32, F), group_of_first=take(np.int32, F), val_off=take(np.int64, m + 1))
    G = int(got["val_off"][m])
    got.update(lines=take(np.int32, G), text_off=take(np.int64, G + 1))
    got.update(chars=take(np.uint16, int(got["text_off"][G])), row_off=take(np.int64, n + 1))
    R, P = int(got["row_off"][n]), len(pm)
    got.update(count=take(np.int32, R), sum_lo=take(np.uint64, R), sum_hi=take(np.uint64, R), min=take(np.int64, R), max=take(np.int64, R),
               pct=take(np.int64, R * P), no_key=take(np.int32, n), not_number=take(np.int32, n), overflow=take(np.int32, n))
    assert at == len(raw)
    return got


def sim_case(simdir, text, key, o, T, keys, numbers, by_of, stop, max_len, queries=(), key_where=None, where=None, window=EVERY_LINE,
             permille=(500, 950), frac_digits=0, **kw):
    m = len(keys)
    where_of = list(key_where or [-1] * m) + list(where or [-1] * len(numbers))
    w = Where(key, o, T, list(keys) + list(numbers), list(queries), where_of, window)
    want = judge_by(o, w, T, m, by_of, stop, max_len, permille, frac_digits)
    got = run_hostsim(simdir, text, w, T, m, by_of, stop, max_len, permille, frac_digits, **kw)
    check_by(got, want, "%s %r by %r" % (key, numbers, keys), stages=True)
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


# the issue's figures (brute force over the fixture's text gave them); the JUDGE decides
def assert_fixture_figures(get):
    """get(number pattern, key pattern, stop, where) -> something with row(0, value), lines_of(value), strings(), no_key, not_number, kept"""
    a = get("size ", "updated: 10.", ".:", None)
    assert a.strings() == ["250", "251"]
    assert (a.lines_of("250"), a.row(0, "250")) == (37, (27, 1_582_626_150, 3_541_872, 67_108_864))
    assert (a.lines_of("251"), a.row(0, "251")) == (210, (176, 11_326_104_278, 3_530_010, 67_108_864))
    assert (int(a.no_key[0]), int(a.not_number[0]), int(a.kept[0])) == (361, 44, 608)
    b = get("size ", " from /10.", ".", None)
    assert (b.lines_of("250"), b.row(0, "250")[:2]) == (41, (36, 2_250_162_971))
    assert (b.lines_of("251"), b.row(0, "251")[:2]) == (181, (139, 9_066_835_001))
    assert int(b.no_key[0]) == 386
    c = get("size ", "INFO ", " :", dict(all=["addStoredBlock"]))
    assert len(c.strings()) == 60
    count, total, vmin, _ = c.row(0, "dfs.FSNamesystem")
    assert (count, total, vmin) == (204, 13_074_465_816, 2)
    d = get("blk_", "INFO ", " :", None)
    assert d.row(0, "")[:2] == (18, 76_684_844_924_695_405_528) and int(d.no_key[0]) == 80


def test_fixture_figures(simdir, hd):
    """the issue's figures on the judge's answer, each case also through the mirror of the stages"""
    o, T = hd

    def get(number, key, stop, where):
        return sim_case(simdir, HD, "hd16 by", o, T, [key], [number], [0], stop, 32, queries=[where] if where else (), key_where=[0] if where else None,
                        where=[0] if where else None)

    assert_fixture_figures(get)


def test_fixture_cross_checks(simdir, hd):
    """one key hit per line: the groups and their lines are field_values' values and counts; two number patterns on one key, two
    keys in one call, a permuting by_of, slots in front of and behind the block, few fences"""
    o, T = hd
    w = Where("hd16 by info", o, T, ["INFO "], [], [-1], EVERY_LINE, " :", 32)
    one = sim_case(simdir, HD, "hd16 by", o, T, ["INFO "], ["size "], [0], " :", 32)
    assert (one.val_off == w.values.val_off).all() and (one.lines == w.values.counts).all() and (one.chars == w.values.chars).all()
    both = sim_case(simdir, HD, "hd16 by", o, T, ["INFO ", "updated: 10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, permille=(0, 500, 1000),
                    lead=3, extra_hits=70, max_fences=16)
    alone = sim_case(simdir, HD, "hd16 by", o, T, ["updated: 10.", "INFO "], ["size ", "size ", "blk_"], [0, 1, 1], " :.", 16, permille=(0, 500, 1000))
    g0, g1 = int(both.val_off[1]), int(both.val_off[2]) - int(both.val_off[1])
    assert (both.count[:g0] == alone.count[g1:g1 + g0]).all() and (both.count[2 * g0:] == alone.count[:g1]).all()
    assert both.sums[g0:2 * g0] == alone.sums[g1 + g0:]


def test_edge_text(simdir, edge):
    """every case of the edge text against both judges, through the mirror"""
    text, o, T = edge
    assert len(T) == EDGE_LINES - 1 and not text.endswith("\n")
    for stop, max_len in ((" \n", 32), (" ", 32), (" \n", 1), (" \n", 64)):
        want = sim_case(simdir, text, "edge", o, T, EDGE_KEYS, EDGE_NUMBERS, [0, 0, 0], stop, max_len, permille=(0, 500, 950, 1000))
        assert_regex(want, 0, 0, text, "k=", "n=", stop, max_len)
        assert_regex(want, 2, 0, text, "k=", "m=", stop, max_len)
        assert want.kept[1] == 0 and want.row_off[2] - want.row_off[1] == want.val_off[1]  # the pattern without a hit still has its rows
    vals = want.strings(0)  # (max_len 64)
    assert "" in vals and "b" in vals and "a" not in vals  # the empty key; of k=b ... k=a the first by position
    assert want.lines_of("far") == 2 and want.lines_of("nb") == 3 and want.lines_of("last") == 1 and want.row(0, "last")[:2] == (1, 42)
    assert want.row(0, "zz9") == (0, 0, 0, 0) and want.lines_of("zz9") == 1
    assert vals[vals.index("ab"):vals.index("ab") + 3] == ["ab", "ab\0", "ab\0\0"]  # a value in front of its extensions
    assert (want.row(0, "ab")[:2], want.row(0, "ab\0")[:2], want.row(0, "ab\0\0")[:2]) == ((2, 103), (1, 51), (1, 52)) and want.lines_of("ab") == 2
    assert want.row(0, "v1")[0] >= 3 and {"abcd", "abcdX", "abcdY", "abcdefghX", "abcdefghY"} <= set(vals)
    # no key of "k=": n=77 (line 10), n=abc and n=12 (line 11: the one that does not parse is no_key and nothing else), n=21 (line 21)
    assert int(want.no_key[0]) == 4 and int(want.overflow[0]) == 1 and int(want.not_number[0]) == 2
    assert want.row(0, "v3")[3] == 2 ** 63 - 1
    # the key pattern that ends its line: with the line feed in the stop set the empty key, without it text of the next line
    nl = sim_case(simdir, text, "edge", o, T, ["k="], ["n="], [0], " ", 32)
    assert "\ntail21" in nl.strings(0) and nl.row(0, "\ntail21")[:2] == (1, 3)
    # fractions; by_of that permutes the keys; a key pattern without a hit; one group only; as many groups as lines
    for F in (0, 3, 9):
        want = sim_case(simdir, text, "edge", o, T, EDGE_KEYS, EDGE_NUMBERS, [3, 1, 2], " \n", 32, permille=(500,), frac_digits=F)
        assert_regex(want, 2, 2, text, "c=", "m=", " \n", 32, F)
        assert want.no_key[0] == want.kept[0] > EDGE_LINES and want.row_off[1] == 0  # every hit of "n=" is no_key: "zq#" has no hit
        assert want.val_off[2] - want.val_off[1] == EDGE_LINES and want.val_off[3] - want.val_off[2] == 1
    frac = sim_case(simdir, text, "edge", o, T, ["k="], ["n="], [0], " \n", 32, frac_digits=3)
    assert_regex(frac, 0, 0, text, "k=", "n=", " \n", 32, 3)
    assert frac.row(0, "v3")[2] == 123 and int(frac.overflow[0]) == 2  # 0.123456789 truncated; 2^63 - 1 scaled by 1000 overflows


def test_edge_text_filters(simdir, edge):
    """a window of lines that cuts a group in two, a filter that keeps no key hit, one that keeps no number hit, key_where_of
    different from where_of"""
    text, o, T = edge
    cut = sim_case(simdir, text, "edge", o, T, ["k="], ["n="], [0], " \n", 32, window=(150, 2101))
    assert cut.lines_of("far") == 1 and cut.lines_of("nb") == 3 and "last" not in cut.strings(0)
    q = [dict(all=["nokey"]), dict(all=["k=far"]), dict(all=["only"])]
    none = sim_case(simdir, text, "edge", o, T, ["k="], ["n="], [0], " \n", 32, queries=q, key_where=[0], where=[-1])
    assert none.val_off[1] == 0 and none.no_key[0] == none.kept[0] > EDGE_LINES and none.key_kept[0] == 0
    empty = sim_case(simdir, text, "edge", o, T, ["k="], ["n="], [0], " \n", 32, queries=q, key_where=[-1], where=[2])
    assert empty.kept[0] == 0 and empty.val_off[1] > 10 and sum(empty.count) == 0
    mixed = sim_case(simdir, text, "edge", o, T, ["k="], ["n="], [0], " \n", 32, queries=q, key_where=[1], where=[-1])
    assert mixed.strings(0) == ["far"] and mixed.row(0, "far")[:2] == (2, 2200) and mixed.no_key[0] == mixed.kept[0] - 2


def test_sanitized_build(simdir, hd, edge):
    """the mirror under AddressSanitizer and UndefinedBehaviorSanitizer, as a program"""
    o, T = hd
    sim_case(simdir, HD, "hd16 by", o, T, ["INFO ", "updated: 10."], ["size ", "blk_"], [1, 0], " :.", 16, lead=5, extra_hits=1030, max_fences=8,
             sanitize=True)
    text, eo, eT = edge
    sim_case(simdir, text, "edge", eo, eT, EDGE_KEYS, EDGE_NUMBERS, [0, 3, 1], " \n", 64, permille=tuple(range(0, 1000, 63)), frac_digits=9, sanitize=True)


def test_host_checks_are_sanitizer_clean(tmp_path):
    """tests/cpp/san_by_of.cpp: check_by_of (index4j_amd/csrc/fmx_host_batch.cpp, the file the library is linked from) and
    fm_by_rows_bad as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, every array exactly as large as
    the contract makes it"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "index4j_amd", "csrc")
    exe = str(tmp_path / "san_by_of")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + csrc, os.path.join(root, "tests", "cpp", "san_by_of.cpp"),
                           os.path.join(csrc, "fmx_host_batch.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert "by_of: all cases ok" in r.stdout, r.stdout[-3000:]


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols); every refusal of a HOST array comes before the handle is asked
    for its device"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_first_hits_of_lines_scratch_bytes", "fmx_first_hits_of_lines_dev", "fmx_values_of_hits_groups_scratch_bytes",
                 "fmx_values_of_hits_groups_dev", "fmx_numbers_by_key_scratch_bytes", "fmx_numbers_by_key_dev", "fmx_number_stats_by_batch",
                 "fmx_number_stats_by_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("k=a n=1\nk=b n=2\n", 4, True, device=None)
    keys, numbers, none = ia.pack_patterns([ia.as_chars("k=")]), ia.pack_patterns([ia.as_chars("n=")]), ia.pack_patterns([])

    def call(by_of=(0,), stop=" \n", max_len=8, permille=(500,), frac_digits=0, keys=keys, where_of=(-1,), lines=None):
        try:
            fm.number_stats_by_batch(*keys, *numbers, by_of, *none, [0], [], [-1] * (len(keys[1]) - 1), where_of, stop, max_len, lines, permille, frac_digits)
        except ia.FmxError as e:
            return e.code, str(e)
        return 0, ""

    assert call()[0] == E_NO_DEVICE
    for kw, word in ((dict(by_of=(1,)), "by_of[0]"), (dict(by_of=(-1,)), "by_of[0]"), (dict(keys=none), "m == 0"), (dict(max_len=0), "max_len"),
                     (dict(max_len=65), "max_len"), (dict(stop="x" * 65), "stop set"), (dict(frac_digits=10), "frac_digits"),
                     (dict(frac_digits=-1), "frac_digits"), (dict(permille=(1001,)), "permille"), (dict(permille=tuple(range(17))), "n_permille"),
                     (dict(where_of=(0,)), "where_of"), (dict(lines=(5, 4)), "window")):
        code, msg = call(**kw)
        assert code == E_ARG and word in msg, (kw, code, msg)
    # the class form: its own batches are judged in front of everything else
    single = lambda ps: ia.pack_class_patterns([list(p) for p in ps])  # noqa: E731

    def ccall(by_of=(0,), max_ranges=16, max_len=8, keys=("k=",)):
        try:
            fm.number_stats_by_class_batch(*single(keys), *single(["n="]), by_of, *single([]), [0], [], [-1] * len(keys), [-1], " \n", max_len, None, (500,), 0,
                                           max_ranges)
        except ia.FmxError as e:
            return e.code, str(e)
        return 0, ""

    assert ccall()[0] == E_NO_DEVICE
    for kw, word in ((dict(by_of=(1,)), "by_of[0]"), (dict(keys=()), "m == 0"), (dict(max_ranges=0), "bad arguments"), (dict(max_ranges=1025), "bad arguments"),
                     (dict(max_len=65), "max_len")):
        code, msg = ccall(**kw)
        assert code == E_ARG and word in msg, (kw, code, msg)
    sizes = ia.lib.fmx_first_hits_of_lines_scratch_bytes, ia.lib.fmx_values_of_hits_groups_scratch_bytes, ia.lib.fmx_numbers_by_key_scratch_bytes
    assert sizes[0](0, 5) == 0 and sizes[0](1, 0) == 0 and sizes[0](1, 2 ** 31) == 0 and sizes[0](1, 1000) > 1000 * 28
    assert sizes[1](1, 1000, 0) == 0 and sizes[1](1, 1000, 65) == 0
    assert sizes[1](2, 1000, 32) >= ia.lib.fmx_values_of_hits_scratch_bytes(2, 1000, 32) + 4000  # the twin's own: a group per run more
    assert sizes[2](1, 1000, 17) == 0 and sizes[2](0, 1000, 2) == 0 and sizes[2](3, 1000, 2) > ia.lib.fmx_numbers_of_hits_scratch_bytes(3, 1000, 0, 2)
    fm.close()

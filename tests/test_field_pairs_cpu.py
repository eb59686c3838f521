"""Statistics and line counts by the values of two fields of the same line (fmx_pairs_of_first_hits_dev,
fmx_number_stats_by_pair_batch; stats p95(latency_ms=) by host=, status= and the pivot table count by host=, status=) on the CPU: the
per-item functions of index4j_amd/csrc/fmx_hit_pairs.hpp and its host checks, compiled for the host and driven by a mirror of the
join stage (tests/pairs_hostsim.cpp, a stand-alone program), which is additionally built with -fsanitize=address,undefined and run
as such, as a program.

The judge is judge_pairs: built over judge_by's first_lines / group_of_first (tests/test_number_stats_by_cpu.py, held to the
README's figures there) by the definition — a line has a pair key where it has a key of both patterns — then plain Python per (number
pattern, pair).  On the edge text a second, independent judge reads the text with regular expressions.  The GPU suite runs the
kernels and the host forms themselves (tests/test_gpu_field_pairs.py, which shares the helpers below)."""
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
from test_match_lines_cpu import judge_table
from test_number_stats_by_cpu import EDGE_LINES, edge_text, judge_by
from test_number_stats_cpu import NAN, OVER, WINDOW, parse_number, pct_of

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
PAIR_KEYS = ["k=", "id=", "c=", "zq#", "m="]
PAIR_NUMBERS = ["n=", "zzq#", "m="]
# what each pair of the edge call covers (indexes into PAIR_KEYS)
EDGE_PAIRS = [(0, 2),   # (k=, c=): b has one group
              (0, 1),   # (k=, id=): as many pairs as lines
              (2, 2),   # (c=, c=): one pair only, a == b
              (0, 3),   # (k=, zq#): b has no hit — no pair, an empty entry between two that are not
              (3, 0),   # (zq#, k=): a is empty
              (0, 4),   # (k=, m=) and
              (4, 0)]   # (m=, k=): lines with a and not b and the reverse, keys 2,000 lines apart, neighbours with one pair, the last line


class Pairs:
    """the judge's answer: base (judge_by's By: the single keys' stages and groups), pair_a, pair_b, pair_off, pair_group_a,
    pair_group_b, pair_lines, joined_off, joined_lines, joined_group (the join), row_off, count, sums (Python ints), min, max, pct
    (the packed rows), no_key, not_number, overflow, kept (n)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def values(self, j=0):
        """[((a, b), lines)] of pair j, in pair order"""
        a, b = self.base.strings(int(self.pair_a[j])), self.base.strings(int(self.pair_b[j]))
        return [((a[int(self.pair_group_a[r])], b[int(self.pair_group_b[r])]), int(self.pair_lines[r]))
                for r in range(int(self.pair_off[j]), int(self.pair_off[j + 1]))]

    def table(self, j=0):
        return dict(self.values(j))

    def rows(self, i=0):
        """{(a, b): (count, sum, min, max)} of number pattern i"""
        r0 = int(self.row_off[i])
        return {v: (int(self.count[r0 + g]), self.sums[r0 + g], int(self.min[r0 + g]), int(self.max[r0 + g]))
                for g, (v, _) in enumerate(self.values(int(self.by_of[i])))} if self.row_off[i + 1] > r0 else {}


def join_lists(first_off, first_lines, group_of_first, pairs):
    """the join by the definition, over any first-hit lists: per pair the lines both sides have, their (ga, gb), the distinct pairs
    ascending with their lines, and the index of every joined line's pair"""
    pair_off, joined_off, ga_all, gb_all, cnt_all, jl_all, jg_all = [0], [0], [], [], [], [], []
    for a, b in pairs:
        la, lb = (first_lines[int(first_off[k]):int(first_off[k + 1])] for k in (a, b))
        fa, fb = (group_of_first[int(first_off[k]):int(first_off[k + 1])] for k in (a, b))
        common, ia_, ib_ = np.intersect1d(la, lb, assume_unique=True, return_indices=True)
        has_groups = (fa[ia_] >= 0) & (fb[ib_] >= 0)  # (a negative group is no group: such a line has no key)
        common, ia_, ib_ = common[has_groups], ia_[has_groups], ib_[has_groups]
        keyed = list(zip(fa[ia_].tolist(), fb[ib_].tolist()))
        distinct = sorted(set(keyed))
        index = {k: r for r, k in enumerate(distinct)}
        counts = np.bincount([index[k] for k in keyed], minlength=len(distinct))
        ga_all += [k[0] for k in distinct]
        gb_all += [k[1] for k in distinct]
        cnt_all += counts.tolist()
        jl_all += common.tolist()
        jg_all += [index[k] for k in keyed]
        pair_off.append(pair_off[-1] + len(distinct))
        joined_off.append(joined_off[-1] + len(common))
    i32 = lambda x: np.array(x, np.int32)  # noqa: E731
    return dict(pair_off=np.array(pair_off, np.int64), pair_group_a=i32(ga_all), pair_group_b=i32(gb_all), pair_lines=i32(cnt_all),
                joined_off=np.array(joined_off, np.int64), joined_lines=i32(jl_all), joined_group=i32(jg_all))


def np_join(first_off, first_lines, group_of_first, val_off, pairs):
    """join_lists in whole-array numpy, for lists of millions of entries and calls of millions of pairs (held to join_lists in
    test_np_join_is_the_definition); a group outside its key pattern's groups is no group, as in the stage"""
    first_off, val_off = np.asarray(first_off, np.int64), np.asarray(val_off, np.int64)
    pa, pb = np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)
    c, m = len(pairs), len(first_off) - 1
    lens = first_off[pa + 1] - first_off[pa]
    slot_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(slot_off[-1])
    slot_pair = np.repeat(np.arange(c, dtype=np.int64), lens)
    at = first_off[pa[slot_pair]] + (np.arange(S, dtype=np.int64) - slot_off[slot_pair])
    lines = np.asarray(first_lines, np.int64)
    groups = np.asarray(group_of_first, np.int64)
    lo, hi = int(first_off[0]), int(first_off[m])
    big = int(lines[lo:hi].max(initial=0)) + 2
    entry_key = np.repeat(np.arange(m, dtype=np.int64), np.diff(first_off)) * big + lines[lo:hi]  # ascending: pattern, then line
    want = pb[slot_pair] * big + lines[at]
    found = np.searchsorted(entry_key, want)
    ok = found < len(entry_key)
    ok[ok] = entry_key[found[ok]] == want[ok]
    ga, gb = groups[at], np.full(S, -1, np.int64)
    gb[ok] = groups[lo + found[ok]]
    n_groups = np.diff(val_off)
    ok &= (ga >= 0) & (ga < n_groups[pa[slot_pair]]) & (gb >= 0) & (gb < n_groups[pb[slot_pair]])
    jp, ja, jb, jl = slot_pair[ok], ga[ok], gb[ok], lines[at][ok]  # the joined entries, in slot order
    order = np.lexsort((jb, ja, jp))
    sp, sa, sb = jp[order], ja[order], jb[order]
    head = np.ones(len(order), bool)
    head[1:] = (sp[1:] != sp[:-1]) | (sa[1:] != sa[:-1]) | (sb[1:] != sb[:-1])
    starts = np.flatnonzero(head)
    pair_off = np.searchsorted(sp[starts], np.arange(c + 1)).astype(np.int64)
    number = np.cumsum(head) - 1  # the packed pair of every sorted entry
    joined_group = np.zeros(len(order), np.int64)
    joined_group[order] = number - pair_off[sp]
    return dict(pair_off=pair_off, pair_group_a=sa[starts].astype(np.int32), pair_group_b=sb[starts].astype(np.int32),
                pair_lines=np.diff(np.concatenate([starts, [len(order)]])).astype(np.int32),
                joined_off=np.searchsorted(jp, np.arange(c + 1)).astype(np.int64), joined_lines=jl.astype(np.int32), joined_group=joined_group.astype(np.int32))


def judge_pairs(o, w, T, m, pairs, by_of, stop, max_len, permille=(500, 950), frac_digits=0):
    """by the definition, over the KEPT hits of a Where whose patterns are m key patterns followed by n number patterns; pairs: (a, b)
    key patterns each; by_of[i]: the pair of number pattern i"""
    n, P = w.n - m, len(permille)
    by_of = np.asarray(by_of, np.int32)
    T = np.asarray(T)
    base = judge_by(o, w, T, m, [pairs[int(j)][0] for j in by_of], stop, max_len, permille, frac_digits)  # (its rows are not looked at)
    j = join_lists(base.first_off, base.first_lines, base.group_of_first, pairs)
    for k, (a, b) in enumerate(pairs):  # the invariants, on the judge itself
        r0, r1 = int(j["pair_off"][k]), int(j["pair_off"][k + 1])
        assert j["pair_lines"][r0:r1].sum() == j["joined_off"][k + 1] - j["joined_off"][k] and (j["pair_lines"][r0:r1] >= 1).all()
        per_a = np.bincount(j["pair_group_a"][r0:r1], weights=j["pair_lines"][r0:r1], minlength=int(base.val_off[a + 1] - base.val_off[a]))
        assert (per_a <= base.lines[int(base.val_off[a]):int(base.val_off[a + 1])]).all()
    # the numbers
    n_off = (w.kept_off[m:] - w.kept_off[m]).astype(np.int64)
    n_locs = w.kept_locs[int(w.kept_off[m]):]
    windows = judge_values(o, np.asarray(n_locs, np.int32), n_off, w.lens[m:], "", WINDOW)
    numbers = [parse_number(row[:ln].tolist(), frac_digits) for row, ln in zip(windows.rows, windows.lengths)]
    per_pair = np.diff(j["pair_off"])
    row_off = np.concatenate([[0], np.cumsum(per_pair[by_of])]).astype(np.int64) if n and j["pair_off"][-1] > 0 else np.zeros(n + 1, np.int64)
    R = int(row_off[-1])
    per = [[] for _ in range(R)]
    no_key, nn, ov = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        k = int(by_of[i])
        mine = j["joined_lines"][int(j["joined_off"][k]):int(j["joined_off"][k + 1])]
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
                per[int(row_off[i]) + int(j["joined_group"][int(j["joined_off"][k]) + at])].append(numbers[t])
    count = np.array([len(p) for p in per], np.int32)
    sums = [sum(p) for p in per]
    vmin = np.array([min(p) if p else 0 for p in per], np.int64)
    vmax = np.array([max(p) if p else 0 for p in per], np.int64)
    pct = np.array([[pct_of(sorted(p), pm) for pm in permille] for p in per], np.int64).reshape(R, P)
    kept = w.kept[m:]
    for i in range(n):  # the invariant, on the judge itself
        assert count[row_off[i]:row_off[i + 1]].sum() + no_key[i] + nn[i] + ov[i] == kept[i]
    return Pairs(base=base, m=m, n=n, P=P, c=len(pairs), by_of=by_of, pair_a=np.array([p[0] for p in pairs], np.int32),
                 pair_b=np.array([p[1] for p in pairs], np.int32), row_off=row_off, count=count, sums=sums, min=vmin, max=vmax, pct=pct, no_key=no_key,
                 not_number=nn, overflow=ov, kept=kept, key_kept=w.kept[:m], **j)


JOIN_NAMES = ("pair_off", "pair_group_a", "pair_group_b", "pair_lines", "joined_off", "joined_lines", "joined_group")


def check_join(got, want, what):
    for name in JOIN_NAMES:
        g, e = np.asarray(got[name]), np.asarray(want[name] if isinstance(want, dict) else getattr(want, name))
        assert g.shape == e.shape and (g == e).all(), "%s: %s %r, expected %r" % (what, name, g[:8], e[:8])


def check_pairs(got, want, what):
    """got: a dict of arrays under the judge's names (the host form's answer)"""
    for name in ("val_off", "lines", "text_off", "chars"):
        g, e = np.asarray(got[name]), np.asarray(getattr(want.base, name))
        assert g.shape == e.shape and (g == e).all(), "%s: %s %r, expected %r" % (what, name, g[:8], e[:8])
    for name in ("pair_off", "pair_group_a", "pair_group_b", "pair_lines", "row_off", "count", "min", "max", "no_key", "not_number", "overflow"):
        g, e = np.asarray(got[name]), np.asarray(getattr(want, name))
        assert g.shape == e.shape and (g == e).all(), "%s: %s %r, expected %r" % (what, name, g[:8], e[:8])
    sums = [(int(hi) << 64) | int(lo) for lo, hi in zip(np.asarray(got["sum_lo"], np.uint64), np.asarray(got["sum_hi"], np.uint64))]
    assert sums == want.sums, what + ": sums"
    assert (np.asarray(got["pct"]).reshape(len(want.count), want.P) == want.pct).all(), what + ": percentiles"


# ---- the independent judge ----
def regex_pairs(text, key_a, key_b, number, stop, max_len, frac_digits=0):
    """{(a, b): [lines, [numbers]]}, the lines with a key of a, of b, and no_key, not_number, overflow — every line and hit by `re`"""
    pairs, no_key, nn, ov, with_a, with_b = {}, 0, 0, 0, 0, 0
    at = 0

    def value_of(line, key):
        k = line.find(key)
        if k < 0:
            return None
        window = text[at + k + len(key):at + k + len(key) + max_len]
        return re.match("[^%s]*" % re.escape(stop), window, re.S).group() if stop else window

    for line in text.split("\n"):
        va, vb = value_of(line, key_a), value_of(line, key_b)
        with_a += va is not None
        with_b += vb is not None
        both = va is not None and vb is not None
        if both:
            pairs.setdefault((va, vb), [0, []])[0] += 1
        for hit in (re.finditer("(?=%s)" % re.escape(number), line) if number else ()):
            v = parse_number([ord(ch) for ch in text[at + hit.start() + len(number):at + hit.start() + len(number) + WINDOW]], frac_digits)
            if not both:
                no_key += 1
            elif v is NAN:
                nn += 1
            elif v is OVER:
                ov += 1
            else:
                pairs[(va, vb)][1].append(v)
        at += len(line) + 1
    return pairs, no_key, nn, ov, with_a, with_b


def units(s):
    return [ord(ch) for ch in s]


def assert_regex_pairs(want, j, i, text, key_a, key_b, number, stop, max_len, frac_digits=0):
    """the judge's pair j (and number pattern i, or None) equals the regular expressions'"""
    pairs, no_key, nn, ov, _, _ = regex_pairs(text, key_a, key_b, number if i is not None else None, stop, max_len, frac_digits)
    order = sorted(pairs, key=lambda v: (units(v[0]), units(v[1])))
    assert want.values(j) == [(v, pairs[v][0]) for v in order]
    if i is not None:
        assert int(want.by_of[i]) == j
        rows = want.rows(i)
        for v in order:
            s = pairs[v][1]
            assert rows[v] == (len(s), sum(s), min(s, default=0), max(s, default=0)), v
        assert (int(want.no_key[i]), int(want.not_number[i]), int(want.overflow[i])) == (no_key, nn, ov)


# ---- the mirror ----
_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "pairs_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "pairs_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("pairs_hostsim")


def run_hostsim(simdir, first_off, first_lines, group_of_first, val_off, pairs, lead=0, extra=0, sanitize=False, expect=0):
    """the join's mirror over first-hit lists; lead: entries in front of first_off[0] that are no first hits; extra: slots beyond the
    real ones (n_slots = the a-sides' first hits + extra)"""
    m, c = len(first_off) - 1, len(pairs)
    fo = np.asarray(first_off, np.int64) + lead
    fl = np.concatenate([np.full(lead, -5, np.int32), np.asarray(first_lines, np.int32)])
    fg = np.concatenate([np.full(lead, -5, np.int32), np.asarray(group_of_first, np.int32)])
    n_slots = int(sum(first_off[a + 1] - first_off[a] for a, _ in pairs)) + extra
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (np.array([m, c, n_slots, len(fl)], np.int64), fo, fl, fg, np.asarray(val_off, np.int64), np.array([p[0] for p in pairs], np.int32),
                  np.array([p[1] for p in pairs], np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), "run", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == expect, (r.returncode, r.stderr[-3000:])
    if expect:
        return None
    raw = np.fromfile(dst, np.uint8)
    at = 0

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += count * np.dtype(dtype).itemsize
        return out

    got = dict(pair_off=take(np.int64, c + 1))
    R = int(got["pair_off"][c])
    got.update(pair_group_a=take(np.int32, R), pair_group_b=take(np.int32, R), pair_lines=take(np.int32, R), joined_off=take(np.int64, c + 1))
    J = int(got["joined_off"][c])
    got.update(joined_lines=take(np.int32, J), joined_group=take(np.int32, J))
    assert at == len(raw)
    return got


def sim_case(simdir, want, what, **kw):
    pairs = list(zip(want.pair_a.tolist(), want.pair_b.tolist()))
    got = run_hostsim(simdir, want.base.first_off, want.base.first_lines, want.base.group_of_first, want.base.val_off, pairs, **kw)
    check_join(got, want, what)
    return got


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


# ---- the fixture's figures: what the README states for "0811" by "INFO dfs.", held against judge_pairs ----
FIX_KEYS, FIX_STOP, FIX_MAX_LEN = ["0811", "INFO dfs."], " :.$\n", 32
DAYS, CLASSES = ("09", "10", "11"), ("DataBlockScanner", "DataNode", "FSDataset", "FSNamesystem")
FIX_TABLE = {("09", "DataBlockScanner"): 2, ("09", "DataNode"): 65, ("09", "FSNamesystem"): 25,
             ("10", "DataBlockScanner"): 13, ("10", "DataNode"): 354, ("10", "FSDataset"): 114, ("10", "FSNamesystem"): 249,
             ("11", "DataBlockScanner"): 3, ("11", "DataNode"): 344, ("11", "FSDataset"): 107, ("11", "FSNamesystem"): 251}
FIX_FILTER = dict(all=["blk_"], none=["PacketResponder"])
FIX_SIZE_ROWS = {("09", "DataNode"): (20, 1_342_177_280, None), ("09", "FSNamesystem"): (14, 939_524_096, None),
                 ("10", "DataNode"): (75, 4_724_082_131, 3_540_106), ("10", "FSNamesystem"): (89, 5_870_511_269, None),
                 ("11", "DataNode"): (87, 5_614_898_808, 3_538_321), ("11", "FSNamesystem"): (101, 6_264_430_451, 2)}


def assert_pair_figures(get):
    """get(number pattern or None, where or None, window or None) -> (table {(a, b): lines}, rows {(a, b): (count, sum, min, max)},
    dict(no_key, not_number, kept, key_lines=(lines with a key of a, of b)))"""
    table, _, info = get(None, None, None)
    assert info["key_lines"] == (2000, 1527) and sum(table.values()) == 1527 and len(table) == 11
    assert table == FIX_TABLE
    table, _, _ = get(None, FIX_FILTER, None)
    filtered = dict(FIX_TABLE)
    filtered.update({("09", "DataNode"): 24, ("10", "DataNode"): 145, ("11", "DataNode"): 114})
    assert sum(table.values()) == 1047 and len(table) == 11 and table == filtered
    table, _, _ = get(None, None, (500, 1000))
    assert table == {("10", "DataBlockScanner"): 7, ("10", "DataNode"): 200, ("10", "FSDataset"): 48, ("10", "FSNamesystem"): 128}
    table, rows, info = get("size ", None, None)
    assert table == FIX_TABLE and (info["kept"], info["no_key"], info["not_number"]) == (608, 133, 89)
    with_numbers = {v: r for v, r in rows.items() if r[0]}
    assert len(with_numbers) == 6 and sum(r[0] for r in rows.values()) == 386 and len(rows) == 11
    for v, (count, total, vmin) in FIX_SIZE_ROWS.items():
        assert with_numbers[v][:2] == (count, total) and with_numbers[v][3] == 67_108_864, v
        assert vmin is None or with_numbers[v][2] == vmin, v


def fixture_case(o, T, number, where, window):
    numbers = [number] if number else []
    q = dict(queries=[where], where_of=[0] * (2 + len(numbers))) if where else dict(queries=[], where_of=[-1] * (2 + len(numbers)))
    w = Where("hd16 pairs", o, T, FIX_KEYS + numbers, q["queries"], q["where_of"], window or EVERY_LINE)
    return w, judge_pairs(o, w, T, 2, [(0, 1)], [0] * len(numbers), FIX_STOP, FIX_MAX_LEN)


def test_fixture_figures(simdir, hd):
    """the issue's figures on the judge's answer, each case also through the mirror of the join"""
    o, T = hd

    def get(number, where, window):
        w, want = fixture_case(o, T, number, where, window)
        sim_case(simdir, want, "hd16 pairs %r %r %r" % (number, where, window), extra=5)
        n = want.n
        info = dict(no_key=int(want.no_key[0]) if n else 0, not_number=int(want.not_number[0]) if n else 0, kept=int(want.kept[0]) if n else 0,
                    key_lines=(int(want.base.first_off[1]), int(want.base.first_off[2] - want.base.first_off[1])))
        return want.table(), want.rows() if n else {}, info

    assert_pair_figures(get)


def edge_case(o, T, stop=" \n", max_len=32, by_of=(0, 1, 5), queries=(), where_of=None, window=EVERY_LINE, permille=(0, 500, 950, 1000), frac_digits=0,
              pairs=EDGE_PAIRS, numbers=PAIR_NUMBERS):
    where_of = list(where_of) if where_of is not None else [-1] * (len(PAIR_KEYS) + len(numbers))
    w = Where("edge pairs", o, T, PAIR_KEYS + list(numbers), list(queries), where_of, window)
    return w, judge_pairs(o, w, T, len(PAIR_KEYS), list(pairs), list(by_of), stop, max_len, permille, frac_digits)


def test_edge_text(simdir, edge):
    """every pair of the edge call against both judges, the join through the mirror with slots in front and behind"""
    text, o, T = edge
    for stop, max_len in ((" \n", 32), (" \n", 1)):
        w, want = edge_case(o, T, stop, max_len)
        sim_case(simdir, want, "edge %r %d" % (stop, max_len), lead=3, extra=70)
        sim_case(simdir, want, "edge %r %d, exactly the slots" % (stop, max_len))
        for j, (a, b) in enumerate(EDGE_PAIRS):
            i = {0: 0, 1: 1, 5: 2}.get(j)
            assert_regex_pairs(want, j, i, text, PAIR_KEYS[a], PAIR_KEYS[b], PAIR_NUMBERS[i] if i is not None else None, stop, max_len)
    w, want = edge_case(o, T)
    base = want.base
    groups = np.diff(base.val_off)
    # (k=, c=): b has one group and a key on every line that has one of a — the pairs are a's groups, pair_lines = lines
    assert groups[2] == 1 and want.pair_off[1] == groups[0] and (want.pair_group_a[:groups[0]] == np.arange(groups[0])).all()
    assert (want.pair_lines[:groups[0]] == base.lines[:groups[0]]).all() and (want.pair_group_b[:groups[0]] == 0).all()
    # (k=, id=): as many pairs as lines with both keys
    assert want.pair_off[2] - want.pair_off[1] == want.joined_off[2] - want.joined_off[1] > EDGE_LINES - 10
    # (c=, c=): one pair, every line
    assert want.values(2) == [(("x", "x"), EDGE_LINES)]
    # (k=, zq#) and (zq#, k=): no pair, empty entries between two that are not
    assert want.pair_off[3] == want.pair_off[4] == want.pair_off[5] and want.joined_off[3] == want.joined_off[5] and want.pair_off[5] < want.pair_off[6]
    # (k=, m=) and (m=, k=): the same pairs with the sides swapped; lines with k= and no m= are a-side slots without a partner in the
    # one and b-side lines that no slot asks for in the other
    km, mk = want.table(5), want.table(6)
    assert km == {(a, b): c for (b, a), c in mk.items()} and sum(km.values()) == base.first_off[5] - base.first_off[4] < base.first_off[1]
    assert km[("b", "1")] == 1  # line 5: of k=b ... k=a the first by position
    assert not {"far", "nb", "last", "zz9"} & {a for a, _ in km}  # keys of lines without m=
    kc = want.table(0)  # one key 2,000 lines apart, neighbouring lines with one pair, the last line
    assert (kc[("far", "x")], kc[("nb", "x")], kc[("last", "x")]) == (2, 3, 1) and want.joined_lines[int(want.joined_off[1]) - 1] == EDGE_LINES - 1
    # Σ_gb pair_lines(ga, ·) <= lines[ga], with equality where every line with a key of a has one of b
    r0, r1 = int(want.pair_off[5]), int(want.pair_off[6])
    per_a = np.bincount(want.pair_group_a[r0:r1], weights=want.pair_lines[r0:r1], minlength=int(groups[0]))
    assert (per_a <= base.lines[:groups[0]]).all() and (per_a < base.lines[:groups[0]]).any()
    # the numbers: n= by (k=, c=) is n= by k= alone, array for array; zzq# has no hit and still its rows; m= by (k=, m=)
    one = judge_by(o, w, T, len(PAIR_KEYS), [0, 0, 0], " \n", 32, (0, 500, 950, 1000), 0)
    a0, a1 = int(want.row_off[0]), int(want.row_off[1])
    assert (want.count[a0:a1] == one.count[:groups[0]]).all() and want.sums[a0:a1] == one.sums[:groups[0]] and (want.pct[a0:a1] == one.pct[:groups[0]]).all()
    assert want.no_key[0] == one.no_key[0] and want.not_number[0] == one.not_number[0] and want.overflow[0] == one.overflow[0]
    assert want.kept[1] == 0 and want.row_off[2] - want.row_off[1] == want.pair_off[2] - want.pair_off[1]
    assert want.no_key[2] == 0 and want.count[int(want.row_off[2]):].sum() == want.kept[2]  # every m= hit lies on a line with k=


def test_np_join_is_the_definition(simdir, edge):
    """np_join (the judge of the GPU suite's made-up lists) against join_lists on the edge call's lists, against the mirror on made-up
    lists with groups that are no groups, and with entries in front of first_off[0]"""
    text, o, T = edge
    w, want = edge_case(o, T)
    base = want.base
    check_join(np_join(base.first_off, base.first_lines, base.group_of_first, base.val_off, EDGE_PAIRS), want, "np_join, edge lists")
    rng = np.random.default_rng(20241021)
    per = [400, 0, 250, 1, 300]
    first_off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    first_lines = np.concatenate([np.sort(rng.choice(600, p, replace=False)) for p in per]).astype(np.int32)
    val_off = np.array([0, 9, 9, 12, 13, 300], np.int64)
    group = np.concatenate([rng.integers(-1, 10, 400), rng.integers(0, 3, 250), [0], rng.integers(0, 301, 300)]).astype(np.int32)  # (-1, 9 and 287: no groups)
    pairs = [(0, 2), (1, 0), (4, 0), (3, 3), (0, 1), (2, 4), (0, 0), (4, 4)]
    made = np_join(first_off, first_lines, group, val_off, pairs)
    assert (group[:400] == 9).any() and (group[:400] == -1).any() and made["pair_off"][2] == made["pair_off"][1] and made["pair_off"][-1] > 100
    valid = np.where((group >= 0) & (group < np.repeat(np.diff(val_off), per)), group, -9)
    check_join(made, join_lists(first_off, first_lines, valid, pairs), "np_join, made-up lists")
    check_join(run_hostsim(simdir, first_off, first_lines, group, val_off, pairs, lead=4, extra=33), made, "the mirror, made-up lists")


def test_pair_of_one_key_is_stats_by(simdir, hd, edge):
    """a pair (k, k) has the pairs (g, g) for every group of k with pair_lines = lines, and its rows are judge_by's rows by k"""
    o, T = hd
    w = Where("hd16 pairs kk", o, T, ["INFO ", "size ", "blk_"], [], [-1, -1, -1])
    want = judge_pairs(o, w, T, 1, [(0, 0)], [0, 0], " :", 32)
    one = judge_by(o, w, T, 1, [0, 0], " :", 32)
    G = int(one.val_off[1])
    assert (want.pair_group_a == np.arange(G)).all() and (want.pair_group_b == np.arange(G)).all() and (want.pair_lines == one.lines).all()
    for name in ("row_off", "count", "min", "max", "pct", "no_key", "not_number", "overflow"):
        assert (getattr(want, name) == getattr(one, name)).all(), name
    assert want.sums == one.sums
    sim_case(simdir, want, "(k, k)", extra=1)


def test_edge_text_filters(simdir, edge):
    """a window of lines, a filter that keeps no key hit of one side, one that keeps nothing at all, the pivot alone (n == 0)"""
    text, o, T = edge
    nk = len(PAIR_KEYS)
    w, cut = edge_case(o, T, window=(150, 2101))
    sim_case(simdir, cut, "edge, window", lead=1, extra=9)
    assert cut.table(0)[("far", "x")] == 1 and cut.table(0)[("nb", "x")] == 3 and ("last", "x") not in cut.table(0)
    q = [dict(all=["nokey"]), dict(all=["k=far"]), dict(all=["zzqq%"])]
    w, none_b = edge_case(o, T, queries=q, where_of=[-1, -1, -1, -1, 0] + [-1] * 3)  # m= only on lines that hold "nokey": none has k=
    assert none_b.pair_off[5] == none_b.pair_off[7] and none_b.no_key[2] == none_b.kept[2] > 0 and none_b.pair_off[1] > 0
    sim_case(simdir, none_b, "edge, no kept hit of one side", extra=3)
    w, nothing = edge_case(o, T, queries=q, where_of=[2] * (nk + 3))
    assert nothing.pair_off[-1] == 0 and nothing.kept.sum() == 0 and nothing.key_kept.sum() == 0
    w, far = edge_case(o, T, queries=q, where_of=[1] * nk + [-1] * 3)
    assert far.values(0) == [(("far", "x"), 2)] and far.values(5) == [] and far.no_key[0] == far.kept[0] - 2
    w, pivot = edge_case(o, T, by_of=(), numbers=())
    assert pivot.n == 0 and len(pivot.row_off) == 1
    check_join({k: getattr(pivot, k) for k in JOIN_NAMES}, edge_case(o, T)[1], "the pivot alone")


def test_sanitized_build(simdir, hd, edge):
    """the mirror under AddressSanitizer and UndefinedBehaviorSanitizer, as a program; made-up lists at the widest key"""
    o, T = hd
    w, want = fixture_case(o, T, None, None, None)
    sim_case(simdir, want, "hd16 pairs", lead=5, extra=1030, sanitize=True)
    text, eo, eT = edge
    w, want = edge_case(eo, eT)
    sim_case(simdir, want, "edge", lead=2, extra=0, sanitize=True)
    sim_case(simdir, want, "edge", lead=0, extra=77, sanitize=True)
    # groups near 2^31 on both sides: 31 + 31 bits and 2 for three pairs; a fourth pair is refused
    first_off = np.array([0, 3, 6], np.int64)
    first_lines = np.array([1, 4, 9, 1, 5, 9], np.int32)
    group = np.array([2 ** 31 - 2, 0, 7, 2 ** 31 - 2, 3, 2 ** 31 - 3], np.int32)
    val_off = np.array([0, 2 ** 31 - 1, 2 ** 32 - 2], np.int64)
    want = join_lists(first_off, first_lines, group, [(0, 1), (1, 0), (1, 1)])
    assert want["pair_lines"].tolist() == [1, 1, 1, 1, 1, 1, 1] and want["pair_group_a"][:2].tolist() == [7, 2 ** 31 - 2]
    check_join(run_hostsim(simdir, first_off, first_lines, group, val_off, [(0, 1), (1, 0), (1, 1)], extra=2, sanitize=True), want, "31 + 31 + 2 bits")
    run_hostsim(simdir, first_off, first_lines, group, val_off, [(0, 1), (1, 0), (1, 1), (0, 0)], sanitize=True, expect=5)


# ---- error returns without a device ----
def raw_pair_call(h, class_form=False, **kw):
    """fmx_number_stats_by_pair_batch / _class_batch through ctypes with every array of the contract's size; kw replaces arguments by
    name (None: a NULL pointer).  Returns rc, whether the caller's arrays are untouched, the twelve pointers"""
    SENT = -0x5A5A5A5B
    lib = ia.lib
    keys, numbers = ["k=", "c="], ["n="]
    ints = {k: np.full(4, SENT, np.int32) for k in ("no_key", "not_number", "overflow", "occurrences", "kept", "status", "key_occurrences", "key_kept",
                                                    "key_status")}
    offs = {k: np.full(4, SENT, np.int64) for k in ("val_off", "pair_off", "row_off")}
    ptrs = {k: C.c_void_p(0x5A5A) for k in ("lines", "text_off", "chars", "pair_group_a", "pair_group_b", "pair_lines", "count", "sum_lo", "sum_hi", "min",
                                            "max", "pct")}
    a = dict(m=2, n=1, n_pairs=1, n_terms=0, q=0, line_lo=0, line_hi=2 ** 31 - 1, n_stop=2, max_len=8, frac_digits=0, n_permille=1, max_ranges=16,
             by_of=np.array([0], np.int32), pair_a=np.array([0], np.int32), pair_b=np.array([1], np.int32), query_off=np.zeros(1, np.int32),
             term_kind=np.zeros(1, np.uint8), key_where_of=np.array([-1, -1], np.int32), where_of=np.array([-1], np.int32),
             stop=ia.as_chars(" \n").astype(np.uint16), permille=np.array([500], np.int32))
    if class_form:
        single = lambda ps: ia.pack_class_patterns([list(p) for p in ps])  # noqa: E731
        (a["key_alt"], a["key_pos_off"], a["key_off"]), (a["alt"], a["pos_off"], a["pat_off"]) = single(keys), single(numbers)
        a["term_alt"], a["term_pos_off"], a["term_off"] = single([])
        for k in ("key_pos_off", "key_off", "pos_off", "pat_off", "term_pos_off", "term_off"):
            a[k] = np.ascontiguousarray(a[k], np.int32)
        a.update(key_n_pos=len(a["key_pos_off"]) - 1, n_pos=len(a["pos_off"]) - 1, term_n_pos=0)
    else:
        (a["key_pat"], a["key_off"]), (a["pat"], a["pat_off"]) = ia.pack_patterns([ia.as_chars(k) for k in keys]), ia.pack_patterns([ia.as_chars(p) for p in numbers])
        a["term_pat"], a["term_off"] = np.zeros(1, np.uint16), np.zeros(1, np.int32)
        a["key_off"], a["pat_off"] = a["key_off"].astype(np.int32), a["pat_off"].astype(np.int32)
    a.update(ints)
    a.update(offs)
    a.update(ptrs)
    a["term_status"] = None
    a.update(kw)

    def arg(name):
        v = a[name]
        if v is None:
            return None
        if isinstance(v, np.ndarray):
            return v.ctypes.data
        if isinstance(v, C.c_void_p):
            return C.byref(v)
        return v

    tail = ["query_off", "term_kind", "q", "key_where_of", "where_of", "line_lo", "line_hi", "stop", "n_stop", "max_len", "frac_digits", "permille", "n_permille",
            "val_off", "lines", "text_off", "chars", "pair_off", "pair_group_a", "pair_group_b", "pair_lines", "row_off", "count", "sum_lo", "sum_hi", "min", "max",
            "pct", "no_key", "not_number", "overflow", "occurrences", "kept", "status", "key_occurrences", "key_kept", "key_status", "term_status"]
    if class_form:
        names = ["key_alt", "key_pos_off", "key_n_pos", "key_off", "m", "alt", "pos_off", "n_pos", "pat_off", "n", "by_of", "n_pairs", "pair_a", "pair_b",
                 "term_alt", "term_pos_off", "term_n_pos", "term_off", "n_terms", "max_ranges"] + tail
        rc = lib.fmx_number_stats_by_pair_class_batch(h, *(arg(k) for k in names))
    else:
        names = ["key_pat", "key_off", "m", "pat", "pat_off", "n", "by_of", "n_pairs", "pair_a", "pair_b", "term_pat", "term_off", "n_terms"] + tail
        rc = lib.fmx_number_stats_by_pair_batch(h, *(arg(k) for k in names))
    untouched = all((v == SENT).all() for v in list(ints.values()) + list(offs.values()))
    return rc, untouched, [ptrs[k].value for k in ptrs if isinstance(a[k], C.c_void_p)]


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols); every refusal of a HOST array comes before the handle is asked for
    its device, and leaves the caller's arrays as they were with the pointers to the ONE allocation NULL"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_pairs_of_first_hits_scratch_bytes", "fmx_pairs_of_first_hits_dev", "fmx_number_stats_by_pair_batch",
                 "fmx_number_stats_by_pair_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("k=a c=x n=1\nk=b c=x n=2\n", 4, True, device=None)
    h = fm.handle
    try:
        for class_form in (False, True):
            rc, untouched, ptrs = raw_pair_call(h, class_form)
            assert rc == E_NO_DEVICE and all(p is None for p in ptrs), (rc, last_error())
            # every "bad arguments" case
            bad = [dict(m=-1), dict(n=-1), dict(n_pairs=-1), dict(n_terms=-1), dict(q=-1), dict(key_where_of=None), dict(where_of=None), dict(by_of=None),
                   dict(pair_a=None), dict(pair_b=None), dict(n_terms=1, term_off=None)]
            bad += [{k: None} for k in ("val_off", "pair_off", "row_off", "lines", "text_off", "chars", "pair_group_a", "pair_group_b", "pair_lines", "count",
                                        "sum_lo", "sum_hi", "min", "max", "pct")]
            if class_form:
                bad += [dict(max_ranges=0), dict(max_ranges=1025), dict(pos_off=None), dict(pat_off=None), dict(key_pos_off=None), dict(key_off=None),
                        dict(n_pos=-1), dict(key_n_pos=-1), dict(term_n_pos=-1), dict(n_terms=1, term_pos_off=None)]
            else:
                bad += [dict(key_off=None), dict(pat_off=None)]
            for kw in bad:
                rc, untouched, ptrs = raw_pair_call(h, class_form, **kw)
                assert rc == E_ARG and "bad arguments" in last_error() and untouched and all(p is None for p in ptrs), (class_form, kw, rc, last_error())
            assert raw_pair_call(None, class_form)[0] == E_ARG and "bad arguments" in last_error()
            # the refusals of the host arrays, each with its word
            i32 = lambda *x: np.array(x, np.int32)  # noqa: E731
            for kw, word in ((dict(pair_a=i32(2)), "pair_a or pair_b"), (dict(pair_b=i32(-1)), "pair_a or pair_b"), (dict(by_of=i32(1)), "by_of"),
                             (dict(by_of=i32(-1)), "by_of"), (dict(n_pairs=0), "n_pairs == 0"), (dict(max_len=0), "max_len"), (dict(max_len=65), "max_len"),
                             (dict(n_stop=65), "stop set"), (dict(frac_digits=10), "frac_digits"), (dict(frac_digits=-1), "frac_digits"),
                             (dict(permille=i32(1001)), "permille"), (dict(n_permille=17), "n_permille"), (dict(where_of=i32(0)), "where_of"),
                             (dict(key_where_of=i32(-1, 0)), "where_of"), (dict(line_lo=5, line_hi=4), "window"), (dict(line_lo=-1), "window")):
                rc, untouched, ptrs = raw_pair_call(h, class_form, **kw)
                assert rc == E_ARG and word in last_error() and untouched and all(p is None for p in ptrs), (class_form, kw, rc, last_error())
        # m == 0: the handle is still asked for its views (tests/test_gpu_field_pairs.py has the answer of a resident one)
        rc, _, ptrs = raw_pair_call(h, m=0, n=0, n_pairs=0, key_off=None, key_where_of=None)
        assert rc == E_NO_DEVICE and all(p is None for p in ptrs)
        rc, _, _ = raw_pair_call(h, m=0, n=0)
        assert rc == E_ARG and "m == 0" in last_error()
        # the Python forms
        with pytest.raises(ia.FmxError) as err:
            fm.field_value_pairs("k=", "c=")
        assert err.value.code == E_NO_DEVICE
        with pytest.raises(ia.FmxError) as err:
            fm.number_stats_by_pair("n=", "k=", "c=", ignore_case=True)
        assert err.value.code == E_NO_DEVICE
        with pytest.raises(IndexError):
            fm.field_value_pairs("k=", "")
        # the join stage: every refusal before the handle is asked for its device
        size = ia.lib.fmx_pairs_of_first_hits_scratch_bytes
        assert size(0, 1, 10) == 0 and size(1, 0, 10) == 0 and size(1, 1, 0) == 0 and size(1, 1, 2 ** 31) == 0
        assert size(2, 3, 1000) >= 1000 * 40 and size(2, 3, 2000) > size(2, 3, 1000)
        p = 0x1000  # (never read: every call below is refused)
        voff, pa, pb = np.array([0, 2, 3], np.int64), np.array([0], np.int32), np.array([1], np.int32)

        def join(m=2, val_off=voff, c=1, pair_a=pa, pair_b=pb, n_slots=100, ws_bytes=None, first=p, out=p):
            need = size(m, c, n_slots)
            return ia.lib.fmx_pairs_of_first_hits_dev(h, m, None if val_off is None else val_off.ctypes.data, c, None if pair_a is None else pair_a.ctypes.data,
                                                      None if pair_b is None else pair_b.ctypes.data, first, first, first, n_slots, out, out, out, out, out, out,
                                                      out, p, need if ws_bytes is None else ws_bytes, None)

        assert join() == E_NO_DEVICE
        for kw in (dict(m=-1), dict(c=-1), dict(val_off=None), dict(pair_a=None), dict(pair_b=None), dict(first=None), dict(out=None)):
            assert join(**kw) == E_ARG and "bad arguments" in last_error(), kw
        wide = np.array([0, 2 ** 31 - 1, 2 ** 32 - 2], np.int64)
        four = np.zeros(4, np.int32)
        for kw, word in ((dict(pair_a=i32(2)), "pair_a or pair_b"), (dict(pair_b=i32(-1)), "pair_a or pair_b"), (dict(m=0), "m == 0"),
                         (dict(val_off=np.array([0, 3, 2], np.int64)), "val_off"), (dict(val_off=np.array([-1, 3, 3], np.int64)), "val_off"),
                         (dict(n_slots=2 ** 31), "2^31 - 1 slots"), (dict(n_slots=-1), "slots"),
                         (dict(val_off=wide, c=4, pair_a=four, pair_b=four + 1), "64 bits"), (dict(ws_bytes=size(2, 1, 100) - 1), "fmx_pairs_of_first_hits_scratch_bytes")):
            assert join(**kw) == E_ARG and word in last_error(), (kw, last_error())
        assert join(val_off=wide, c=3, pair_a=four[:3], pair_b=four[:3] + 1) == E_NO_DEVICE  # 2 + 31 + 31 bits
    finally:
        fm.close()

"""The lines ranked by the number behind a pattern (fmx_top_lines_of_hits_dev, fmx_top_lines_where_batch; ... | sort -k latency -nr |
head -10) on the CPU: the functions the kernels of index4j_amd/csrc/fmx_hit_top.hip run — fm_top_ordered, fm_top_better,
fm_top_line_key, fm_top_segment, fm_top_rows (index4j_amd/csrc/fmx_hit_top.hpp), with fm_val_window, fm_hit_tile / fm_hit_pattern,
fm_num_parse, fm_line_of over fences and fm_range_tail's word — compiled for the host and driven by a mirror of the stages
(tests/top_lines_hostsim.cpp, a stand-alone program: its `self` mode checks the functions at their edges, its `top` mode runs the
stages lane by lane), built once plain and once with -fsanitize=address,undefined and run directly, as a program.

The judge is Python over the oracle (judge_top_lines), never the code under test: the windows are judge_values' at 32
(tests/test_field_values_cpu.py), the number parse_number's (tests/test_number_stats_cpu.py), the kept hits Where's
(tests/test_field_values_where_cpu.py), the line np.searchsorted(T, loc, "left"), the ranking plain `sorted`.  The GPU suite runs the
kernels and the host forms themselves (tests/test_gpu_top_lines.py, which shares the helpers below)."""
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import judge_values
from test_field_values_where_cpu import SENT, Where
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_stats_cpu import FRACS, INT64_MAX, NAN, OVER, WINDOW, parse_number, parser_text

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()


class Top:
    """the judge's answer for a batch: rows, lines, numbers, not_number, overflow (n), row_line, row_value, row_loc (n, top), zero
    behind rows[i]; ranked[i]: EVERY candidate of pattern i as (line, value, loc), best first; windows: judge_values' answer"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def judge_top_lines(o, locs, hit_off, lens, T, descending, top=10, first=0, frac_digits=0):
    """by the definition, over packed hits (the KEPT hits of a Where): the window of every hit from the oracle, its value, its
    line, the candidate of every line, then plain `sorted`"""
    n = len(hit_off) - 1
    windows = judge_values(o, np.asarray(locs, np.int32), np.asarray(hit_off, np.int64), lens, "", WINDOW)
    cache, vals = {}, []
    for row, ln in zip(windows.rows, windows.lengths):
        key = row[:ln].tobytes()
        if key not in cache:
            cache[key] = parse_number(row[:ln].tolist(), frac_digits)
        vals.append(cache[key])
    rows, lines, numbers, nn, ov = (np.zeros(n, np.int32) for _ in range(5))
    row_line, row_loc, row_value = np.zeros((n, top), np.int32), np.zeros((n, top), np.int32), np.zeros((n, top), np.int64)
    ranked = []
    for i in range(n):
        a, b = int(hit_off[i]), int(hit_off[i + 1])
        L = np.searchsorted(T, np.asarray(locs[a:b]), side="left").tolist()
        sign = -1 if descending[i] else 1
        best = {}  # line -> (the value in the order asked, loc): the smallest wins
        for v, line, loc in zip(vals[a:b], L, np.asarray(locs[a:b]).tolist()):
            if v is NAN:
                nn[i] += 1
            elif v is OVER:
                ov[i] += 1
            else:
                numbers[i] += 1
                best[line] = min(best.get(line, (sign * v, loc)), (sign * v, loc))
        order = sorted(best, key=lambda line: (best[line][0], line))
        ranked.append([(line, sign * best[line][0], best[line][1]) for line in order])
        lines[i] = len(order)
        mine = ranked[i][first:first + top]
        rows[i] = len(mine)
        for j, (line, v, loc) in enumerate(mine):
            row_line[i, j], row_value[i, j], row_loc[i, j] = line, v, loc
        assert numbers[i] + nn[i] + ov[i] == b - a and rows[i] == min(top, max(0, lines[i] - first))  # the invariants, on the judge itself
    return Top(n=n, top=top, rows=rows, lines=lines, numbers=numbers, not_number=nn, overflow=ov, row_line=row_line, row_value=row_value,
               row_loc=row_loc, ranked=ranked, windows=windows, values=vals)


def judge_where_top(o, w, T, descending, top=10, first=0, frac_digits=0):
    """... over the KEPT hits of a Where"""
    return judge_top_lines(o, w.kept_locs, w.kept_off, w.lens, T, descending, top, first, frac_digits)


def check_top(got, want, what):
    """got: a dict of arrays (rows, row_line, row_value, row_loc, lines, numbers, not_number, overflow), each of the answer's shape"""
    n, top = want.n, want.top
    for name in ("rows", "lines", "numbers", "not_number", "overflow"):
        assert (np.asarray(got[name]).reshape(n) == getattr(want, name)).all(), "%s: %s %r" % (what, name, np.asarray(got[name]).tolist()[:8])
    for name in ("row_line", "row_value", "row_loc"):
        g = np.asarray(got[name]).reshape(n, top)
        assert (g == getattr(want, name)).all(), "%s: %s at %r" % (what, name, np.argwhere(g != getattr(want, name))[:4].tolist())


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "top_lines_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "top_lines_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("top_lines_hostsim")


def run_top_sim(simdir, want, T, n, hit_off, locs, lens, text_len, descending, top=10, first=0, frac_digits=0, extra_hits=0, max_fences=4096,
                sanitize=False):
    """the stages' mirror over a packed block (hit_off[0] may be non-zero; extra_hits slots behind hit_off[n] hold no hit) and the
    JUDGE's windows of the hits, in their order; a dict as check_top takes it"""
    begin, total = int(hit_off[0]), int(hit_off[-1])
    n_hits = total + extra_hits
    locs = np.concatenate([locs, np.full(extra_hits, SENT, np.int32)]).astype(np.int32)[:n_hits]
    inside = total - begin
    w = want.windows
    assert inside == len(w.lengths)
    per_slot = np.zeros(n_hits, np.int64)
    per_slot[begin:begin + inside] = w.lengths
    win_off = np.concatenate([[0], np.cumsum(per_slot)]).astype(np.int64)
    keep = np.arange(WINDOW)[None, :] < w.lengths[:, None]
    win = w.rows[keep] if inside else np.zeros(0, np.uint16)
    head = np.array([n, n_hits, len(T), max_fences, frac_digits, text_len, first, top], np.int64)
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (head, np.asarray(T, np.int32), np.asarray(lens, np.int32), np.asarray(descending, np.uint8), np.asarray(hit_off, np.int64), locs,
                  win_off, win.astype(np.uint16)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), "top", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.uint8)
    at = 0

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += count * np.dtype(dtype).itemsize
        return out

    got = dict(rows=take(np.int32, n), row_line=take(np.int32, n * top), row_value=take(np.int64, n * top), row_loc=take(np.int32, n * top),
               lines=take(np.int32, n), numbers=take(np.int32, n), not_number=take(np.int32, n), overflow=take(np.int32, n))
    start, stop = take(np.int32, n_hits), take(np.int32, n_hits)
    assert at == len(raw)
    assert (start[begin:begin + inside] == w.starts).all() and (stop[begin:begin + inside] == w.stops).all()
    assert (start[:begin] == 0).all() and (stop[begin + inside:] == 0).all()
    return got


def sim_where(simdir, o, w, T, descending, top=10, first=0, frac_digits=0, **kw):
    """judge and mirror over the KEPT hits of a Where; returns the judge's answer"""
    want = judge_where_top(o, w, T, descending, top, first, frac_digits)
    got = run_top_sim(simdir, want, T, w.n, w.kept_off, w.kept_locs, w.lens, o.getInputLength() - 1, descending, top, first, frac_digits, **kw)
    check_top(got, want, "%r descending %r top %d first %d F %d" % (w.where_of.tolist(), list(descending), top, first, frac_digits))
    return want


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


# the fixture's figures (HDFS_2k_multichar.log, 2,000 lines), computed with plain Python from the text by the definition.  A case:
# (pattern, the call's keywords, numbers, lines, the rows as (line, value, loc) — None: a field the figures leave open —, rows[0])
ADD, TERM = dict(all=["addStoredBlock"]), dict(all=["terminating"])
FIXTURE_CASES = [
    ("size ", dict(top=3), 485, 485, [(2, 67108864, 402), (5, None, 857), (7, None, 1212)], 3),
    ("size ", dict(first=455, top=4), 485, 485, [(1993, 67108864, 314200), (1996, 67108864, 314646), (1707, 41287838, 269231), (1537, 28508403, 237991)], 4),
    ("size ", dict(largest=False, top=5), 485, 485,
     [(1629, 2, 257267), (1207, 3530010, 186663), (1473, 3534443, 228172), (1835, 3538321, 289276), (583, 3540106, 90025)], 5),
    ("size ", dict(largest=False, top=3, where=ADD), 254, 254, [(1629, 2, 257267), (1207, 3530010, 186663), (1473, 3534443, 228172)], 3),
    ("size ", dict(largest=False, top=3, where=dict(all=["size "], none=["addStoredBlock"])), 231, 231,
     [(1835, 3538321, None), (583, 3540106, None), (41, 3542967, 6600)], 3),
    ("size ", dict(top=3, lines=(500, 1000)), 117, 117, [(503, None, None), (513, None, None), (515, None, None)], 3),
    ("blk_", dict(top=3), 1237, 1004, [(693, 9216955386716663841, 107304), (17, 9212264480425680329, 2687), (357, 9188832735514090334, 54604)], 3),
    ("blk_", dict(first=1000, top=10), 1237, 1004, [None, None, None, (167, 278357163850888, 25944)], 4),
    ("blk_", dict(largest=False, top=3), 1237, 1004, [(167, 278357163850888, 25944), (1549, 1077394056781488, 240033), (1609, 1832308388558480, 254120)], 3),
    ("blk_", dict(largest=False, first=1004), 1237, 1004, [], 0),
    ("blk_", dict(top=2, where=TERM), 154, 154, [(279, 9107849594802857322, 43277), (71, 9093049293972551787, 11123)], 2),
    ("blk_", dict(largest=False, top=2, lines=(1000, 1100)), 60, 53, [(1015, 107727140948970996, 157021), (1094, 157913239647511296, 169454)], 2),
    ("src: /10.", dict(frac_digits=3, top=4), 235, 235, [(940, 251910, None), (980, 251910, None), (1334, 251910, None), (1416, 251910, None)], 4),
    ("src: /10.", dict(frac_digits=3, largest=False, first=2, top=3), 235, 235, [(715, 250100, None), (744, 250100, None), (944, 250100, None)], 3),
    # the candidate rule: line 1578 holds 50 ids that parse (and 50 behind a minus that do not), line 72 the same id twice (the smaller position wins)
    ("blk_", dict(top=1, lines=(1578, 1579)), 50, 1, [(1578, 9174833667156726933, 246508)], 1),
    ("blk_", dict(largest=False, top=1, lines=(1578, 1579)), 50, 1, [(1578, 61908781908925992, 246613)], 1),
    ("blk_", dict(top=1, lines=(72, 73)), 2, 1, [(72, 1781953582842324563, 11235)], 1),
    ("blk_", dict(largest=False, top=1, lines=(72, 73)), 2, 1, [(72, 1781953582842324563, 11235)], 1),
]


def assert_fixture_figures(get):
    """get(pattern, **keywords of FmIndex.top_lines_by_number) -> an object with line, value, loc (the rows) and lines, numbers,
    not_number, overflow, kept as ints: the figures of the fixture, whoever computed them"""
    for pattern, kw, numbers, lines, rows, n_rows in FIXTURE_CASES:
        s = get(pattern, **kw)
        what = (pattern, kw)
        assert (s.numbers, s.lines, len(s.line), len(s.value), len(s.loc)) == (numbers, lines, n_rows, n_rows, n_rows), what
        assert s.numbers + s.not_number + s.overflow == s.kept, what
        for j, row in enumerate(rows):
            for got, field in zip((s.line[j], s.value[j], s.loc[j]), row or ()):
                assert field is None or int(got) == field, (what, j)


class JudgedRows:
    """pattern 0 of a judge's answer in the shape assert_fixture_figures reads"""

    def __init__(self, want, w):
        r = int(want.rows[0])
        self.line, self.value, self.loc = want.row_line[0, :r], want.row_value[0, :r], want.row_loc[0, :r]
        self.lines, self.numbers = int(want.lines[0]), int(want.numbers[0])
        self.not_number, self.overflow, self.kept = int(want.not_number[0]), int(want.overflow[0]), int(w.kept[0])


def fixture_where(o, T, pattern, where=None, lines=None):
    return Where("hd16", o, T, [pattern], [where] if where else [], [0 if where else -1], lines or (0, 2 ** 31 - 1))


def test_per_item_functions(simdir):
    """the ordered value at 0 and 2^63 - 1 in both orders, the minimum of (u, position) as an associative and commutative operator,
    the run key, the segments, the rows, every argument the C ABI refuses: top_lines_hostsim.cpp's self_checks, plain and under
    AddressSanitizer and UBSan"""
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_fixture_figures(simdir, hd):
    """the issue's figures on the judge over the oracle, and the stages' mirror gives the judge's answer (also through few fences,
    with slots behind the hits and under the sanitizers)"""
    o, T = hd
    assert judge_n_lines(T, len(HD)) == 2000
    calls = []

    def get(pattern, largest=True, first=0, top=10, where=None, lines=None, frac_digits=0):
        w = fixture_where(o, T, pattern, where, lines)
        fences = (4096, 3, 0)[len(calls) % 3]
        want = sim_where(simdir, o, w, T, [1 if largest else 0], top, first, frac_digits, max_fences=fences, extra_hits=5 * (fences == 3),
                         sanitize=fences == 0)
        calls.append(pattern)
        return JudgedRows(want, w)

    assert_fixture_figures(get)
    assert len(calls) == len(FIXTURE_CASES)


def test_parser_text_both_ends(simdir):
    """ONE pattern ("=") over the parser table's text at F = 0, 3, 9: 0 and the largest value sit at both ends in both orders —
    2^63 - 1 itself at F = 0 and F = 9 —, the cases that do not parse are counted by reason"""
    text, _, expected = parser_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    w = Where("parser table top", o, T, ["="], [], [-1])
    cases = len(expected) - 1  # (the last pattern of parser_text is a pattern, not a line)
    assert w.occurrences.tolist() == [cases]
    for k, F in enumerate(FRACS):
        values = [e[k] for e in expected[:cases]]
        ints = [v for v in values if isinstance(v, int)]
        for desc in (0, 1):
            want = sim_where(simdir, o, w, T, [desc], top=cases + 3, frac_digits=F, sanitize=F == 3)  # (top larger than lines)
            assert want.lines[0] == want.numbers[0] == len(ints) == want.rows[0]
            assert want.not_number[0] == sum(v is NAN for v in values) and want.overflow[0] == sum(v is OVER for v in values)
            got = want.row_value[0, :len(ints)].tolist()
            assert got == sorted(ints, reverse=bool(desc)) and got[0 if not desc else -1] == 0 and got[-1 if not desc else 0] == max(ints)
            assert (want.row_value[0, len(ints):] == 0).all() and (want.row_line[0, len(ints):] == 0).all()
            last = sim_where(simdir, o, w, T, [desc], top=1, first=len(ints) - 1, frac_digits=F)
            assert last.rows[0] == 1 and last.row_value[0, 0] == (0 if desc else max(ints))
            if not desc:  # equal values rank by line: 0 is case 0's alone, the ties of the table follow their lines
                lines_of = want.row_line[0, :len(ints)].tolist()
                assert all(a < b for a, b, x, y in zip(lines_of, lines_of[1:], got, got[1:]) if x == y)
        if F in (0, 9):
            assert max(ints) == INT64_MAX


MIX_QUERIES = [dict(all=["terminating"]), dict(all=["blk_"], none=["PacketResponder"]), dict(all=["zzzq#"])]
MIX_PATTERNS = ["blk_", "size ", "zzzq#", "INFO ", "blk_", ":", "size ", "blk_-"]
MIX_WHERE = [0, -1, -1, 1, -1, 1, 2, -1]
MIX_DESC = [1, 0, 1, 0, 0, 1, 1, 0]


def test_mixes(simdir, hd):
    """mixed orders in one batch; a pattern with no hit between two with hits; a pattern whose hits all fail to parse; a pattern
    whose query has no line; top larger than every lines[i], top = 1, first in the middle; a window of lines; raw hits with the
    terms' hits in front (hit_off[0] != 0) and slots behind; n = 0"""
    o, T = hd
    w = Where("hd16 top mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    for top, first, F in ((2500, 0, 0), (1, 0, 3), (7, 100, 9), (10, 2000, 0)):
        want = sim_where(simdir, o, w, T, MIX_DESC, top, first, F, extra_hits=37, max_fences=64, sanitize=top == 7)
        assert (want.numbers + want.not_number + want.overflow == w.kept).all()
    assert want.lines[2] == 0 and w.kept[2] == 0 and want.lines[6] == 0 and w.kept[6] == 0
    assert w.kept[3] > 0 and want.numbers[3] == 0 and want.not_number[3] == w.kept[3] and want.lines[3] == 0  # "INFO " is never followed by a digit
    assert 0 < want.lines[0] <= want.numbers[0] and want.lines[4] == 1004 and 0 < want.numbers[5] < w.kept[5]
    win = Where("hd16 top mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE, (300, 1700))
    sim_where(simdir, o, win, T, MIX_DESC, 20, 3, 0)
    raw = Where("hd16 top mix", o, T, MIX_PATTERNS, MIX_QUERIES, [-1] * len(MIX_PATTERNS))
    nt = raw.n_terms
    assert raw.hit_off[nt] > 0 and (raw.kept == raw.occurrences).all()
    want = judge_where_top(o, raw, T, MIX_DESC, 12, 1, 0)
    got = run_top_sim(simdir, want, T, raw.n, raw.hit_off[nt:], raw.packed, raw.lens, len(HD), MIX_DESC, 12, 1, 0, extra_hits=1030, sanitize=True)
    check_top(got, want, "raw hits, terms in front")
    want = judge_top_lines(o, np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), T, [], 5)
    got = run_top_sim(simdir, want, T, 0, np.zeros(1, np.int64), np.zeros(0, np.int32), [], len(HD), [], 5, extra_hits=3)
    assert all(len(v) == 0 for v in got.values())


def test_error_returns_without_a_device():
    """every refusal the arguments alone decide; fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_top_lines_of_hits_scratch_bytes", "fmx_top_lines_of_hits_dev", "fmx_top_lines_where_batch", "fmx_top_lines_where_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("size 12 is long\nsize 7 and one more line\n", 4, True, device=None)
    lens, desc, hit_off, ids = np.array([5, 2, 1], np.int32), np.array([1, 0, 1], np.uint8), np.zeros(4, np.int64), np.zeros(8, np.int32)
    out = np.full(64, SENT, np.int64)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def dcall(h=fm._h, n=3, tl=lens, d=desc, hoff=hit_off, locs=ids, n_hits=2, F=0, first=0, top=4, rows=out):
        return ia.lib.fmx_top_lines_of_hits_dev(h, n, p(tl), p(d), p(hoff), p(locs), n_hits, F, first, top, p(rows), p(out), p(out), p(out), p(out),
                                                p(out), p(out), p(out), None, None, 0, None)

    assert dcall() == E_NO_DEVICE and dcall(first=2 ** 31 - 1) == E_NO_DEVICE
    bad_shape = (dict(F=-1), dict(F=10), dict(first=-1), dict(top=0), dict(top=-3))
    for bad in (dict(h=None), dict(n=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(locs=None), dict(rows=None), dict(tl=None),
                dict(d=None), dict(tl=np.array([5, -1, 1], np.int32))) + bad_shape:
        assert dcall(**bad) == E_ARG, bad
    # (int64) n * top above 2^27
    wide = dict(n=1 << 11, tl=np.zeros(1 << 11, np.int32), d=np.zeros(1 << 11, np.uint8), hoff=np.zeros((1 << 11) + 1, np.int64))
    assert dcall(top=1 << 16, **wide) == E_NO_DEVICE and dcall(top=(1 << 16) + 1, **wide) == E_ARG and dcall(top=2 ** 31 - 1) == E_ARG
    assert (out == SENT).all()
    sb = ia.lib.fmx_top_lines_of_hits_scratch_bytes
    assert sb(0, 5, 3) == 0 and sb(5, 0, 3) == 0 and sb(5, 1 << 31, 3) == 0 and sb(5, 9, 0) == 0 and sb(5, 9, -1) == 0
    assert sb(1 << 11, 9, (1 << 16) + 1) == 0 and sb(-1, 9, 3) == 0
    # the host forms
    ch, off = ia.pack_patterns(["size ", "is", "line"])
    tch, toff = ia.pack_patterns(["long", "one", "more"])
    off, toff = off.astype(np.int32), toff.astype(np.int32)
    qoff, kinds = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.uint8)
    where_of = np.array([0, -1, 1], np.int32)
    small = np.full(3, SENT, np.int32)

    def host(h=fm._h, off_=off, n=3, toff_=toff, nt=3, qoff_=qoff, kinds_=kinds, q=2, wo=where_of, lo=0, hi=2 ** 31 - 1, d=desc, F=0, first=0, top=4,
             rows=small):
        return ia.lib.fmx_top_lines_where_batch(h, ch.ctypes.data, p(off_), n, tch.ctypes.data, p(toff_), nt, p(qoff_), p(kinds_), q, p(wo), lo, hi,
                                                p(d), F, first, top, p(rows), p(out), p(out), p(out), p(small), p(small), p(small), p(small), None,
                                                p(small), None, None)

    assert host() == E_NO_DEVICE and host(lo=1, hi=1) == E_NO_DEVICE
    query_bad = (dict(qoff_=None), dict(kinds_=None), dict(qoff_=np.array([1, 2, 3], np.int32)), dict(qoff_=np.array([0, 3, 2], np.int32)),
                 dict(kinds_=np.array([0, 3, 1], np.uint8)), dict(q=-1), dict(h=None), dict(n=-1), dict(off_=None), dict(rows=None), dict(d=None),
                 dict(off_=np.array([0, 4, 2, 10], np.int32)), dict(nt=-1), dict(toff_=None), dict(wo=None), dict(wo=np.array([2, 0, 0], np.int32)),
                 dict(wo=np.array([-2, 0, 0], np.int32)), dict(toff_=np.array([-1, 6, 9, 13], np.int32)), dict(lo=-1), dict(hi=-1), dict(lo=5, hi=4))
    for bad in query_bad + bad_shape + (dict(top=(1 << 27) // 3 + 1),):
        assert host(**bad) == E_ARG, bad
    assert (out == SENT).all() and (small == SENT).all()
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert host(h=h) == E_ARG and dcall(h=h) == E_ARG
    # the class twin judges its arrays the same way
    alt, pos_off, pat_off = (np.ascontiguousarray(x) for x in ia.pack_class_patterns([ia.ignore_case("size ")]))
    talt, tpos, tpat = (np.ascontiguousarray(x) for x in ia.pack_class_patterns([ia.ignore_case("one")]))
    q1, k1, w1, d1 = np.array([0, 1], np.int32), np.array([0], np.uint8), np.array([0], np.int32), np.array([1], np.uint8)

    def host_class(h=fm._h, max_ranges=16, wo=w1, tpat_=tpat, lo=0, hi=2 ** 31 - 1, d=d1, F=0, first=0, top=4):
        return ia.lib.fmx_top_lines_where_class_batch(h, p(alt), p(pos_off), len(pos_off) - 1, p(pat_off), 1, p(talt), p(tpos), len(tpos) - 1,
                                                      p(tpat_), 1, max_ranges, p(q1), p(k1), 1, p(wo), lo, hi, p(d), F, first, top, p(small), p(out),
                                                      p(out), p(out), None, None, None, None, None, None, None, None)

    assert host_class() == E_NO_DEVICE
    for bad in (dict(h=None), dict(max_ranges=0), dict(max_ranges=1 << 20), dict(tpat_=np.array([0, 9], np.int32)), dict(wo=np.array([1], np.int32)),
                dict(d=None), dict(lo=3, hi=2)) + bad_shape:
        assert host_class(**bad) == E_ARG, bad
    assert (out == SENT).all() and (small == SENT).all()
    # the Python mirror: an empty pattern or term raises as number_stats("") does, before anything runs; without a device the call says so
    for run in (lambda: fm.top_lines_by_number(""), lambda: fm.top_lines_by_number("size ", where=dict(all="is", none=["x", ""]))):
        with pytest.raises(IndexError, match="ArrayIndexOutOfBoundsException"):
            run()
    with pytest.raises(ValueError):
        fm.top_lines_by_number("size ", where=dict(every=["x"]))
    for run in (lambda: fm.top_lines_by_number("size "), lambda: fm.top_lines_by_number("size ", 3, False, where=dict(any=["long", "one"]), ignore_case=True)):
        with pytest.raises(ia.FmxError) as err:
            run()
        assert err.value.code == E_NO_DEVICE
    for run in (lambda: fm.top_lines_by_number("size ", top=0), lambda: fm.top_lines_by_number("size ", frac_digits=10),
                lambda: fm.top_lines_by_number("size ", first=-1), lambda: fm.top_lines_by_number("size ", lines=(3, 2))):
        with pytest.raises(ia.FmxError) as err:
            run()
        assert err.value.code == E_ARG
    res = ia.TopLines(dict(rows=[2], row_line=np.array([[7, 3, 0]]), row_value=np.array([[9, 9, 0]]), row_loc=np.array([[70, 30, 0]]), lines=[2],
                           numbers=[5], not_number=[1], overflow=[0], occurrences=[8], kept=[6]))
    assert len(res) == 2 and res.line.tolist() == [7, 3] and res.value.tolist() == [9, 9] and res.loc.tolist() == [70, 30] and res.text is None
    assert (res.lines, res.numbers, res.not_number, res.overflow, res.kept, res.occurrences) == (2, 5, 1, 0, 6, 8)

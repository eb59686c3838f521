"""Statistics of the number behind a pattern, per bucket of lines (fmx_numbers_of_hits_dev, fmx_number_stats_where_batch; stats
sum(size) p95(size) by minute where line has addStoredBlock) on the CPU: the functions the kernels of
index4j_amd/csrc/fmx_hit_numbers.hip run — fm_num_parse, fm_num_code, fm_num_segment, fm_num_pct_index, fm_num_scan_between,
fm_num_sum128 (index4j_amd/csrc/fmx_hit_numbers.hpp), with fm_val_window, fm_hit_tile / fm_hit_pattern, fm_line_of over fences and
fm_hist_bucket — compiled for the host and driven by a mirror of the stages (tests/numbers_hostsim.cpp, a stand-alone program: its
`self` mode checks the functions at their edges, its `parse` mode runs the parser over windows, its `stats` mode runs the stages lane
by lane), built once plain and once with -fsanitize=address,undefined and run directly, as a program.

The judge is Python over the oracle (judge_numbers): the windows are judge_values' (tests/test_field_values_cpu.py: the oracle's
extract over [s, e) at max_len = 32), the number a regular expression and Python's integers, the kept hits Where's
(tests/test_field_values_where_cpu.py), the buckets judge_bins' (tests/test_line_histogram_cpu.py), the percentile an index into
`sorted`.  The GPU suite runs the kernels and the host forms themselves (tests/test_gpu_number_stats.py, which shares the helpers
below)."""
import os
import re
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import judge_values
from test_field_values_where_cpu import EVERY_LINE, SENT, Trimmed, Where
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN, judge_bins
from test_match_lines_cpu import judge_n_lines, judge_table

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
WINDOW = 32
INT64_MAX = 2 ** 63 - 1
NAN, OVER = "not a number", "overflow"
KIND = {0: None, 1: NAN, 2: OVER}  # numbers_hostsim.cpp's kNumOk, kNumNotNumber, kNumOverflow
P5 = (0, 1, 500, 999, 1000)

# the parser table: (what follows the pattern, the value at frac_digits 0, 3, 9)
PARSER_TABLE = [
    ("0", (0, 0, 0)), ("007", (7, 7000, 7 * 10 ** 9)), ("12", (12, 12000, 12 * 10 ** 9)),
    ("12.5", (12, 12500, 125 * 10 ** 8)), ("1.25", (1, 1250, 125 * 10 ** 7)), ("1.", (1, 1000, 10 ** 9)),
    ("1.2345678901", (1, 1234, 1234567890)),  # truncated
    (".5", (NAN,) * 3), ("x", (NAN,) * 3), ("", (NAN,) * 3),
    ("9223372036854775807", (INT64_MAX, OVER, OVER)), ("9223372036854775808", (OVER,) * 3), ("9" * 20, (OVER,) * 3),
    ("9223372036.854775807", (9223372036, 9223372036854, INT64_MAX)), ("9223372036.854775808", (9223372036, 9223372036854, OVER)),
    ("0" * 31 + "7", (OVER,) * 3),  # D == 32
    ("0" * 30 + "7 ", (7, 7000, 7 * 10 ** 9)),
]
FRACS = (0, 3, 9)


def parser_text():
    """ONE text with one hit per case of the table: case k follows the pattern "cKK=" and ends in a line feed; the last two cases are
    a digit run cut by the end of the text ("123", the shorter number) and a window clipped to zero length at textLength (the
    pattern IS the text's tail: not a number).  Returns text, patterns, expected[k] = the three values"""
    cases = PARSER_TABLE + [("123", (123, 123000, 123 * 10 ** 9))]
    text = "".join("c%02d=%s\n" % (k, c) for k, (c, _) in enumerate(cases))[:-1]  # (no line feed behind the last case)
    patterns = ["c%02d=" % k for k in range(len(cases))] + ["c%02d=123" % (len(cases) - 1)]
    return text, patterns, [e for _, e in cases] + [(NAN,) * 3]


def parse_number(units, frac_digits):
    """the value of a window of code units by the definition: an int, NAN or OVER"""
    s = "".join(map(chr, units))
    run = re.match("[0-9]*", s).group()
    if not run:
        return NAN
    if len(run) == WINDOW:
        return OVER
    frac = ""
    if frac_digits > 0 and s[len(run):len(run) + 1] == ".":
        frac = re.match("[0-9]*", s[len(run) + 1:]).group()[:frac_digits]
    v = int(run) * 10 ** frac_digits + (int(frac) * 10 ** (frac_digits - len(frac)) if frac else 0)
    return OVER if v > INT64_MAX else v


def pct_of(values, permille):
    """nearest rank over ascending values: index max(1, ceil(permille * c / 1000)) - 1"""
    c = len(values)
    return values[max(1, -(-permille * c // 1000)) - 1] if c else 0


class Numbers:
    """the judge's rows for a batch: count, min, max (n, B), pct (n, B, P), sums[i][b] as Python ints, not_number and overflow (n),
    hist_total (n) = the hits of each pattern that lie in SOME bucket; windows: judge_values' answer (starts, stops, rows, lengths)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def judge_numbers(o, locs, hit_off, lens, T, edges=None, permille=(500, 950), frac_digits=0):
    """by the definition, over packed hits (the KEPT hits of a Where, or any others): the window of every hit from the oracle, its
    value, its line and bucket, then plain Python per (pattern, bucket)"""
    n = len(hit_off) - 1
    B = 1 if edges is None else len(edges) - 1
    P = len(permille)
    windows = judge_values(o, np.asarray(locs, np.int32), np.asarray(hit_off, np.int64), lens, "", WINDOW)
    cache = {}
    vals = []
    for row, ln in zip(windows.rows, windows.lengths):
        key = row[:ln].tobytes()
        if key not in cache:
            cache[key] = parse_number(row[:ln].tolist(), frac_digits)
        vals.append(cache[key])
    count = np.zeros((n, B), np.int32)
    vmin, vmax, pct = np.zeros((n, B), np.int64), np.zeros((n, B), np.int64), np.zeros((n, B, P), np.int64)
    sums = [[0] * B for _ in range(n)]
    nn, ov, hist_total = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        a, b = int(hit_off[i]), int(hit_off[i + 1])
        mine = vals[a:b]
        if edges is None:
            bucket = np.zeros(b - a, np.int64)
            hist_total[i] = b - a
        else:
            L = np.searchsorted(T, np.asarray(locs[a:b]), side="left")
            bucket = np.searchsorted(np.asarray(edges, np.int64), L, "right") - 1
            hist_total[i] = judge_bins(edges, L).sum()
            count[i] = judge_bins(edges, L[[isinstance(v, int) for v in mine]] if b > a else L)
        per = [[] for _ in range(B)]
        for v, bk in zip(mine, bucket.tolist()):
            if 0 <= bk < B:
                if v is NAN:
                    nn[i] += 1
                elif v is OVER:
                    ov[i] += 1
                else:
                    per[bk].append(v)
        for bk in range(B):
            s = sorted(per[bk])
            if edges is None:
                count[i, bk] = len(s)
            assert count[i, bk] == len(s)
            sums[i][bk] = sum(s)
            if s:
                vmin[i, bk], vmax[i, bk] = s[0], s[-1]
            pct[i, bk] = [pct_of(s, pm) for pm in permille]
        assert count[i].sum() + nn[i] + ov[i] == hist_total[i]  # the invariant, on the judge itself
    return Numbers(n=n, B=B, P=P, count=count, sums=sums, min=vmin, max=vmax, pct=pct, not_number=nn, overflow=ov, hist_total=hist_total,
                   windows=windows, values=vals)


def judge_where_numbers(o, w, T, edges=None, permille=(500, 950), frac_digits=0, lens=None):
    """... over the KEPT hits of a Where (or a Trimmed: the lengths are the Where's)"""
    return judge_numbers(o, w.kept_locs, w.kept_off, w.lens if lens is None else lens, T, edges, permille, frac_digits)


def check_numbers(got, want, what):
    """got: a dict of arrays (count, sum_lo, sum_hi, min, max, pct, not_number, overflow), each of the answer's shape"""
    n, B, P = want.n, want.B, want.P
    assert (np.asarray(got["count"]).reshape(n, B) == want.count).all(), "%s: count %r" % (what, np.argwhere(np.asarray(got["count"]).reshape(n, B) != want.count)[:4])
    lo, hi = np.asarray(got["sum_lo"], np.uint64).reshape(n, B), np.asarray(got["sum_hi"], np.uint64).reshape(n, B)
    sums = [[(int(hi[i, b]) << 64) | int(lo[i, b]) for b in range(B)] for i in range(n)]
    assert sums == want.sums, "%s: sums" % what
    for name in ("min", "max"):
        assert (np.asarray(got[name]).reshape(n, B) == getattr(want, name)).all(), "%s: %s" % (what, name)
    assert (np.asarray(got["pct"]).reshape(n, B, P) == want.pct).all(), "%s: percentiles" % what
    assert (np.asarray(got["not_number"]) == want.not_number).all() and (np.asarray(got["overflow"]) == want.overflow).all(), what + ": the tails"


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "numbers_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "numbers_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("numbers_hostsim")


def _run(simdir, mode, arrays, sanitize):
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), mode, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return np.fromfile(dst, np.uint8)


def run_parse_sim(simdir, windows, frac_digits, sanitize=False):
    """the parser over windows (lists of code units); [int | NAN | OVER]"""
    win_off = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64)
    win = np.array([u for w in windows for u in w], np.uint16)
    raw = _run(simdir, "parse", (np.array([len(windows), frac_digits], np.int64), win_off, win), sanitize)
    m = len(windows)
    kind, value = raw[:4 * m].view(np.int32), raw[4 * m:].view(np.int64)
    assert len(value) == m
    return [int(v) if k == 0 else KIND[int(k)] for k, v in zip(kind, value)]


def run_stats_sim(simdir, want, T, n, hit_off, locs, lens, text_len, edges=None, permille=(500, 950), frac_digits=0, n_hits=None, extra_hits=0,
                  max_fences=4096, sanitize=False):
    """the stages' mirror over a packed block (hit_off[0] may be non-zero; extra_hits slots behind hit_off[n] hold no hit; n_hits:
    fewer slots than hits) and the JUDGE's windows of the hits inside the slots, in their order; a dict as check_numbers takes it"""
    first, total = int(hit_off[0]), int(hit_off[-1])
    n_hits = total + extra_hits if n_hits is None else n_hits
    locs = np.concatenate([locs, np.full(extra_hits, SENT, np.int32)]).astype(np.int32)[:n_hits]
    inside = max(min(total, n_hits) - first, 0)
    w = want.windows
    assert inside <= len(w.lengths)
    per_slot = np.zeros(n_hits, np.int64)
    per_slot[first:first + inside] = w.lengths[:inside]
    win_off = np.concatenate([[0], np.cumsum(per_slot)]).astype(np.int64)
    keep = np.arange(WINDOW)[None, :] < w.lengths[:inside, None]
    win = w.rows[:inside][keep] if inside else np.zeros(0, np.uint16)
    e = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32)
    B, P = (1 if edges is None else len(e) - 1), len(permille)
    head = np.array([n, n_hits, len(T), max_fences, len(e), P, frac_digits, text_len], np.int64)
    raw = _run(simdir, "stats", (head, np.asarray(T, np.int32), np.asarray(lens, np.int32), np.asarray(hit_off, np.int64), locs, e,
                                 np.asarray(permille, np.int32), win_off, win.astype(np.uint16)), sanitize)
    at = 0

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += count * np.dtype(dtype).itemsize
        return out

    got = dict(count=take(np.int32, n * B), sum_lo=take(np.uint64, n * B), sum_hi=take(np.uint64, n * B), min=take(np.int64, n * B),
               max=take(np.int64, n * B), pct=take(np.int64, n * B * P), not_number=take(np.int32, n), overflow=take(np.int32, n))
    start, stop = take(np.int32, n_hits), take(np.int32, n_hits)
    assert at == len(raw)
    assert (start[first:first + inside] == w.starts[:inside]).all() and (stop[first:first + inside] == w.stops[:inside]).all()
    assert (start[:first] == 0).all() and (stop[first + inside:] == 0).all()
    return got


def sim_where(simdir, o, w, T, edges=None, permille=(500, 950), frac_digits=0, **kw):
    """judge and mirror over the KEPT hits of a Where; returns the judge's rows"""
    want = judge_where_numbers(o, w, T, edges, permille, frac_digits)
    got = run_stats_sim(simdir, want, T, w.n, w.kept_off, w.kept_locs, w.lens, o.getInputLength() - 1, edges, permille, frac_digits, **kw)
    check_numbers(got, want, "%r edges %r F %d" % (w.where_of.tolist(), None if edges is None else list(edges[:4]), frac_digits))
    return want


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


def test_per_item_functions(simdir):
    """the parser table at F = 0, 3, 9, the window, the codes and the key's width, nearest rank at segments of 1, 2, 3, 1,000 and
    1,001 values, the 128-bit sum up to 2^31 - 1 values of 2^63 - 1: numbers_hostsim.cpp's self_checks, plain and under
    AddressSanitizer and UBSan"""
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_parser_table(simdir):
    """every case of the table for F = 0, 3, 9: the Python judge gives the table's values, the compiled parser gives the judge's —
    over windows cut from the case itself, and through the stages over ONE text with one hit per case (the oracle's windows), where a
    digit run is cut by the end of the text and a window is clipped to zero length at textLength"""
    for k, F in enumerate(FRACS):
        windows = [ia.as_chars(c)[:WINDOW].tolist() for c, _ in PARSER_TABLE]
        want = [e[k] for _, e in PARSER_TABLE]
        assert [parse_number(w, F) for w in windows] == want, F
        assert run_parse_sim(simdir, windows, F, sanitize=F == 3) == want, F
    assert pct_of([5], 0) == 5 and pct_of([1, 2, 3], 500) == 2 and pct_of([1, 2], 501) == 2 and pct_of([], 500) == 0
    text, patterns, expected = parser_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    w = Where("parser table", o, T, patterns, [], [-1] * len(patterns))
    assert (w.occurrences == 1).all()
    for k, F in enumerate(FRACS):
        want = sim_where(simdir, o, w, T, None, P5, F, sanitize=F == 9)
        assert want.values == [e[k] for e in expected], F
        ok = [isinstance(e[k], int) for e in expected]
        assert want.count[:, 0].tolist() == [int(x) for x in ok]
        assert want.not_number.tolist() == [int(e[k] is NAN) for e in expected] and want.overflow.tolist() == [int(e[k] is OVER) for e in expected]
        assert [int(v) for v, x in zip(want.min[:, 0], ok) if x] == [e[k] for e, x in zip(expected, ok) if x]
    assert w.kept_locs[-1] + len(patterns[-1]) == len(text) and want.windows.lengths[-1] == 0 and want.windows.lengths[-2] == 3


# the fixture's figures (HDFS_2k_multichar.log, 2,000 lines): plain Python over the decoded text gives them
SIZE_ALL = dict(hits=608, count=485, not_number=123, overflow=0, sum=31_092_874_658, min=2, max=67_108_864, p50=67_108_864, p95=67_108_864)
SIZE_250 = [(81, 5_267_518_200), (23, 1_543_503_872), (77, 4_963_019_311), (40, 2_557_244_675), (64, 4_090_601_777), (70, 4_359_082_915),
            (64, 4_061_245_351), (66, 4_250_658_557)]
# (a query of NONE terms only has no lines — NONE filters, it does not enumerate the text —, so under none=["addStoredBlock"] alone
# nothing is kept; the figures of "the lines without addStoredBlock" are those of all=["size "], none=["addStoredBlock"])
SIZE_WHERE = [(dict(all=["addStoredBlock"]), 254, 16_264_173_630, 2, 60), (dict(none=["addStoredBlock"]), 0, 0, 0, 0),
              (dict(all=["size "], none=["addStoredBlock"]), 231, 14_828_701_028, 3_538_321, 63)]
BLK = dict(count=1237, not_number=1231, sum=5_728_063_121_572_615_439_579, min=278_357_163_850_888, max=9_216_955_386_716_663_841,
           p50=4_640_277_741_339_926_850, p95=8_823_112_510_768_971_040)
SRC = dict(count=235, sum=59_007_553, min=250_100, max=251_910, p50=251_195, p95=251_740)


def assert_fixture_figures(get):
    """get(pattern, edges, where, frac_digits) -> an object with count, sum (Python ints), min, max, pct (B, 2: p50, p95),
    not_number, overflow, occurrences: the figures of the fixture, whoever computed them"""
    s = get("size ", None, None, 0)
    assert (s.occurrences, int(s.count[0]), s.not_number, s.overflow, s.sum[0], int(s.min[0]), int(s.max[0]), int(s.pct[0][0]), int(s.pct[0][1])) == \
        tuple(SIZE_ALL[k] for k in ("hits", "count", "not_number", "overflow", "sum", "min", "max", "p50", "p95"))
    s = get("size ", EDGES_250, None, 0)
    assert list(zip(s.count.tolist(), s.sum)) == SIZE_250 and int(s.min[6]) == 2 and int(s.min[1]) == 67_108_864
    assert sum(c for c, _ in SIZE_250) == SIZE_ALL["count"] and sum(x for _, x in SIZE_250) == SIZE_ALL["sum"]
    for where, count, total, vmin, nn in SIZE_WHERE:
        s = get("size ", None, where, 0)
        assert (int(s.count[0]), s.sum[0], int(s.min[0]), s.not_number) == (count, total, vmin, nn), where
    s = get("blk_", None, None, 0)
    assert (int(s.count[0]), s.not_number, s.sum[0], int(s.min[0]), int(s.max[0]), int(s.pct[0][0]), int(s.pct[0][1])) == \
        tuple(BLK[k] for k in ("count", "not_number", "sum", "min", "max", "p50", "p95"))
    assert s.sum[0] > 2 ** 64 and s.overflow == 0 and s.occurrences == 2468  # the 128-bit sum on the fixture itself
    s = get("src: /10.", None, None, 3)
    assert (int(s.count[0]), s.sum[0], int(s.min[0]), int(s.max[0]), int(s.pct[0][0]), int(s.pct[0][1])) == \
        tuple(SRC[k] for k in ("count", "sum", "min", "max", "p50", "p95"))


class JudgedRow:
    """row 0 of a judge's answer in the shape assert_fixture_figures reads"""

    def __init__(self, want, w):
        self.count, self.sum, self.min, self.max, self.pct = want.count[0], want.sums[0], want.min[0], want.max[0], want.pct[0]
        self.not_number, self.overflow, self.occurrences = int(want.not_number[0]), int(want.overflow[0]), int(w.occurrences[0])


def test_fixture_figures(simdir, hd):
    """the issue's figures on the judge over the oracle, and the stages' mirror gives the judge's answer (also through few fences
    and under the sanitizers)"""
    o, T = hd
    assert judge_n_lines(T, len(HD)) == 2000
    calls = []

    def get(pattern, edges, where, frac_digits):
        w = Where("hd16", o, T, [pattern], [where] if where else [], [0 if where else -1])
        fences = (4096, 3, 0)[len(calls) % 3]
        want = sim_where(simdir, o, w, T, edges, (500, 950), frac_digits, max_fences=fences, extra_hits=5 * (fences == 3), sanitize=fences == 0)
        calls.append(pattern)
        return JudgedRow(want, w)

    assert_fixture_figures(get)
    assert len(calls) == 7


MIX_QUERIES = [dict(all=["terminating"]), dict(all=["blk_"], none=["PacketResponder"]), dict(all=["zzzq#"]), dict(none=["INFO"]), dict(),
               dict(any=["WARN", "Receiving"], none="src:")]
MIX_PATTERNS = ["blk_", "/10.", "INFO ", "size ", " ", "1", "blk_", "zzzq#", "dfs.", ":", "", "blk_-"]
MIX_WHERE = [0, 0, 1, -1, 2, 3, 4, 0, 5, -1, 1, -1]


def test_mixes_uneven_edges_and_tile_edges(simdir, hd):
    """the where tests' mix (with "size " and "blk_-" among the patterns) over edges that cut the fixture unevenly; raw hits with
    terms in front (hit_off[0] != 0); a pattern without hits between two with hits; slots trimmed to the tile edges; one pattern
    owning every hit"""
    o, T = hd
    w = Where("hd16 number mix", o, T, MIX_PATTERNS, MIX_QUERIES, MIX_WHERE)
    for edges, F, pm in ((EDGES_UNEVEN, 0, (500, 950)), (EDGES_BEYOND, 3, P5), (None, 9, ()), (EDGES_250, 0, tuple(range(0, 1000, 63)))):
        want = sim_where(simdir, o, w, T, edges, pm, F, extra_hits=37, max_fences=64)
        if edges is None or (edges[0] == 0 and edges[-1] >= 2000):
            assert (want.hist_total == w.kept).all()
        else:
            assert (want.hist_total <= w.kept).all() and want.hist_total.sum() < w.kept.sum()
    assert want.P == 16 and want.count[7].sum() == 0 and want.count[3].sum() == SIZE_ALL["count"] and want.count[11].sum() > 0
    assert want.not_number[9] > 0 and want.count[9].sum() > 0  # ":" is followed by numbers and by words
    # the raw hits of the value patterns, the terms' in front: hit_off + n_terms does not start at 0
    raw = Where("hd16 number mix", o, T, MIX_PATTERNS, MIX_QUERIES, [-1] * len(MIX_PATTERNS))
    nt = raw.n_terms
    assert raw.hit_off[nt] > 0 and (raw.kept == raw.occurrences).all()
    want = judge_where_numbers(o, raw, T, EDGES_UNEVEN, P5, 3)
    got = run_stats_sim(simdir, want, T, raw.n, raw.hit_off[nt:], raw.packed, raw.lens, len(HD), EDGES_UNEVEN, P5, 3, extra_hits=3)
    check_numbers(got, want, "raw hits, terms in front")
    # n_hits trimmed: 0, 1, 1,023, 1,024, 1,025 value hits, whole tiles of slots
    w3 = Where("hd16 number edges", o, T, [" ", "size ", "1"], [dict(all=["terminating"])], [-1, -1, -1], EVERY_LINE)
    first, total = int(w3.hit_off[w3.n_terms]), int(w3.hit_off[-1])
    assert first > 0 and total - first > 5 * 1024
    for n_hits in [first + k for k in (0, 1, 1023, 1024, 1025)] + [1024 * (first // 1024 + 1), 1024 * (first // 1024 + 3) + 1, total - 1]:
        t = Trimmed(w3, n_hits)
        want = judge_where_numbers(o, t, T, EDGES_UNEVEN, (500,), 0, lens=w3.lens)
        got = run_stats_sim(simdir, want, T, w3.n, w3.hit_off[w3.n_terms:], w3.packed, w3.lens, len(HD), EDGES_UNEVEN, (500,), 0, n_hits=n_hits,
                            sanitize=n_hits == first + 1025)
        check_numbers(got, want, "n_hits %d" % n_hits)
    one = Where("hd16 number one", o, T, [" "], [], [-1])
    sim_where(simdir, o, one, T, EDGES_BEYOND, (950,), 0)


def segments_text():
    """patterns "a=" .. "e=" with 1, 2, 3, 1,000 and 1,001 values, duplicates among them, ten per line"""
    rng = np.random.default_rng(3)
    fields = []
    for name, c in zip("abcde", (1, 2, 3, 1000, 1001)):
        fields += ["%s=%d" % (name, v) for v in rng.integers(0, 400, c)]
    order = rng.permutation(len(fields))
    fields = [fields[i] for i in order]
    return "\n".join(" ".join(fields[i:i + 10]) for i in range(0, len(fields), 10)) + "\n", ["%s=" % c for c in "abcde"]


def test_percentile_indices(simdir):
    """permille 0, 1, 500, 999, 1000 against segments of 1, 2, 3, 1,000 and 1,001 values with duplicates; P = 0 and P = 16"""
    text, patterns = segments_text()
    o = orc.OracleFmIndex(text, 4, True)
    T = judge_table(o, "\n")
    w = Where("segments", o, T, patterns, [], [-1] * 5)
    assert w.occurrences.tolist() == [1, 2, 3, 1000, 1001]
    want = sim_where(simdir, o, w, T, None, P5, 0, sanitize=True)
    assert want.count[:, 0].tolist() == [1, 2, 3, 1000, 1001] and (want.pct[:, 0, 0] == want.min[:, 0]).all() and (want.pct[:, 0, 4] == want.max[:, 0]).all()
    assert len(set(sorted(v for v in want.values[6:1006]))) < 1000  # duplicates
    for pm in ((), tuple(range(0, 1000, 63)), (1000,) * 16):
        sim_where(simdir, o, w, T, [0, 50, 50, 150, 300], pm, 0)


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    names = ("fmx_numbers_of_hits_scratch_bytes", "fmx_numbers_of_hits_dev", "fmx_number_stats_where_batch", "fmx_number_stats_where_class_batch")
    for name in names:
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("size 12 is long\nsize 7 and one more line\n", 4, True, device=None)
    edges, pm = np.array([0, 1, 2], np.int32), np.array([500, 950], np.int32)
    lens, hit_off, ids = np.array([5, 2, 1], np.int32), np.zeros(4, np.int64), np.zeros(8, np.int32)
    out = np.full(64, SENT, np.int64)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def dcall(h=fm._h, n=3, tl=lens, hoff=hit_off, locs=ids, n_hits=2, e=edges, ne=3, F=0, pm_=pm, P=2, count=out):
        return ia.lib.fmx_numbers_of_hits_dev(h, n, p(tl), p(hoff), p(locs), n_hits, p(e), ne, F, p(pm_), P, p(count), p(out), p(out), p(out), p(out),
                                              p(out), p(out), p(out), None, None, 0, None)

    assert dcall() == E_NO_DEVICE and dcall(e=None, ne=0) == E_NO_DEVICE and dcall(pm_=None, P=0) == E_NO_DEVICE
    bad_edges = (dict(e=None), dict(ne=1), dict(ne=-1), dict(ne=0), dict(e=np.array([-1, 1, 2], np.int32)), dict(e=np.array([0, 2, 1], np.int32)))
    bad_shape = (dict(F=-1), dict(F=10), dict(P=-1), dict(P=17, pm_=np.zeros(17, np.int32)), dict(pm_=None), dict(pm_=np.array([0, 1001], np.int32)),
                 dict(pm_=np.array([-1, 5], np.int32)))
    for bad in (dict(h=None), dict(n=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(locs=None), dict(count=None), dict(tl=None),
                dict(tl=np.array([5, -1, 1], np.int32))) + bad_edges + bad_shape:
        assert dcall(**bad) == E_ARG, bad
    # (int64) n * B and n * B * P above 2^27
    big = np.arange((1 << 16) + 2, dtype=np.int32)
    wide = dict(tl=np.zeros(1 << 11, np.int32), hoff=np.zeros((1 << 11) + 1, np.int64))
    assert dcall(n=1 << 11, e=big, ne=len(big), P=0, **wide) == E_ARG and dcall(n=1 << 11, e=big, ne=len(big) - 1, P=1, **wide) == E_NO_DEVICE
    assert dcall(n=1 << 11, e=big, ne=len(big) - 1, P=2, **wide) == E_ARG
    assert (out == SENT).all()
    sb = ia.lib.fmx_numbers_of_hits_scratch_bytes
    assert sb(0, 5, 3, 2) == 0 and sb(5, 0, 3, 2) == 0 and sb(5, 1 << 31, 3, 2) == 0 and sb(5, 9, 1, 2) == 0 and sb(5, 9, 3, 17) == 0
    assert sb(1 << 11, 9, len(big), 0) == 0 and sb(1 << 11, 9, len(big) - 1, 2) == 0 and sb(5, 9, -1, 2) == 0
    for ne in (0, 61):  # per slot: the window's 64 bytes, four 8-byte sort arrays, ranges and offsets
        assert sb(3, 1000, ne, 2) >= (64 + 32 + 28) * 1000 + ne * 4 and sb(3, 1000, ne, 2) % 256 == 0 and sb(3, 1000, ne, 2) < 400 * 1000
    # the host forms
    ch, off = ia.pack_patterns(["size ", "is", "line"])
    tch, toff = ia.pack_patterns(["long", "one", "more"])
    off, toff = off.astype(np.int32), toff.astype(np.int32)
    qoff, kinds = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.uint8)
    where_of = np.array([0, -1, 1], np.int32)
    small = np.full(3, SENT, np.int32)

    def host(h=fm._h, off_=off, n=3, toff_=toff, nt=3, qoff_=qoff, kinds_=kinds, q=2, wo=where_of, e=edges, ne=3, F=0, pm_=pm, P=2, count=out):
        return ia.lib.fmx_number_stats_where_batch(h, ch.ctypes.data, p(off_), n, tch.ctypes.data, p(toff_), nt, p(qoff_), p(kinds_), q, p(wo), p(e), ne,
                                                   F, p(pm_), P, p(count), p(out), p(out), p(out), p(out), p(out), p(small), p(small), None, p(small),
                                                   None, None)

    assert host() == E_NO_DEVICE and host(e=None, ne=0) == E_NO_DEVICE
    query_bad = (dict(qoff_=None), dict(kinds_=None), dict(qoff_=np.array([1, 2, 3], np.int32)), dict(qoff_=np.array([0, 3, 2], np.int32)),
                 dict(kinds_=np.array([0, 3, 1], np.uint8)), dict(q=-1), dict(h=None), dict(n=-1), dict(off_=None), dict(count=None),
                 dict(off_=np.array([0, 4, 2, 10], np.int32)), dict(nt=-1), dict(toff_=None), dict(wo=None), dict(wo=np.array([2, 0, 0], np.int32)),
                 dict(wo=np.array([-2, 0, 0], np.int32)), dict(toff_=np.array([-1, 6, 9, 13], np.int32)))
    for bad in query_bad + bad_edges + bad_shape:
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
    q1, k1, w1 = np.array([0, 1], np.int32), np.array([0], np.uint8), np.array([0], np.int32)

    def host_class(h=fm._h, max_ranges=16, e=edges, ne=3, wo=w1, tpat_=tpat, F=0, pm_=pm, P=2):
        return ia.lib.fmx_number_stats_where_class_batch(h, p(alt), p(pos_off), len(pos_off) - 1, p(pat_off), 1, p(talt), p(tpos), len(tpos) - 1,
                                                         p(tpat_), 1, max_ranges, p(q1), p(k1), 1, p(wo), p(e), ne, F, p(pm_), P, p(out), p(out), p(out),
                                                         p(out), p(out), p(out), None, None, None, None, None, None)

    assert host_class() == E_NO_DEVICE
    for bad in (dict(h=None), dict(max_ranges=0), dict(max_ranges=1 << 20), dict(tpat_=np.array([0, 9], np.int32)), dict(wo=np.array([1], np.int32))) + \
            bad_edges + bad_shape:
        assert host_class(**bad) == E_ARG, bad
    assert (out == SENT).all()
    # the Python mirror: an empty pattern or term raises as hit_histogram("") does, before anything runs; without a device the call says so
    for run in (lambda: fm.number_stats(""), lambda: fm.number_stats("size ", where=dict(all="is", none=["x", ""]))):
        with pytest.raises(IndexError, match="ArrayIndexOutOfBoundsException"):
            run()
    with pytest.raises(ValueError):
        fm.number_stats("size ", where=dict(every=["x"]))
    for run in (lambda: fm.number_stats("size "), lambda: fm.number_stats("size ", [0, 2], where=dict(any=["long", "one"]), ignore_case=True)):
        with pytest.raises(ia.FmxError) as err:
            run()
        assert err.value.code == E_NO_DEVICE
    for run in (lambda: fm.number_stats("size ", [2, 1]), lambda: fm.number_stats("size ", frac_digits=10), lambda: fm.number_stats("size ", permille=[1001])):
        with pytest.raises(ia.FmxError) as err:
            run()
        assert err.value.code == E_ARG
    stats = ia.NumberStats(dict(count=np.array([[2, 0]]), sum_lo=np.array([[5, 0]], np.uint64), sum_hi=np.array([[1, 0]], np.uint64), min=np.zeros((1, 2)),
                                max=np.zeros((1, 2)), pct=np.zeros((1, 2, 0)), not_number=[1], overflow=[0], occurrences=[3], kept=[3]), 0)
    assert stats.sum == [2 ** 64 + 5, 0] and stats.mean()[0] == (2 ** 64 + 5) / 2 and np.isnan(stats.mean()[1])

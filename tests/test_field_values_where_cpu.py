"""Field values and hits only within the lines of a query (fmx_hits_in_lines_dev, fmx_field_values_where_batch; grep terminating |
grep -o 'blk_[^ ]*' | sort | uniq -c) on the CPU: the functions the kernels of index4j_amd/csrc/fmx_hit_filter.hip run —
fm_filter_line_listed, fm_filter_keep, fm_filter_slot, fm_filter_kept_off (index4j_amd/csrc/fmx_hit_filter.hpp), with fm_hit_tile /
fm_hit_pattern and fm_line_of over fences — compiled for the host and driven by a mirror of the stages
(tests/hit_filter_hostsim.cpp, a stand-alone program: the flag kernel's tile loop, std::exclusive_scan, the scatter, checked against
std::stable_partition), which is additionally built with -fsanitize=address,undefined and run as such, as a program.

The judge is Python over the oracle (judge_where): the hits are expected_packed's (tests/test_locate_all_cpu.py), the line table
judge_table's and the terms' lines judge_lines' (tests/test_match_lines_cpu.py), the lines of a query numpy's set algebra over them,
the filter np.searchsorted on the line table, the values judge_values on what is left (tests/test_field_values_cpu.py).  The GPU
suite runs the kernels and the host forms themselves (tests/test_gpu_field_values_where.py, which shares the helpers below)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_cpu import check_values, judge_values, run_hostsim as run_values_hostsim
from test_locate_all_cpu import expected_packed
from test_match_lines_cpu import judge_lines, judge_n_lines, judge_table

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SENT = -0x3C3C3C3D
SIM_SENT = -77  # hit_filter_hostsim.cpp's kSentinel
INT32_MAX = 2 ** 31 - 1
EVERY_LINE = (0, INT32_MAX)
ALL, ANY, NONE = 0, 1, 2

# the fixture's two named cases: (pattern, stop, max_len, query, hits in the whole text, kept, distinct values, the most frequent)
NAMED = [
    ("blk_", " \t\r\n", 32, dict(all=["terminating"]), 2468, 310, 310, []),
    ("INFO ", " \t\r\n:", 32, dict(all=["blk_"], none=["PacketResponder"]), 1920, 1317, 248, [("dfs.FSNamesystem", 525)]),
]
# a pattern in the first and in the last line; lines that alternate kept / dropped; the last value runs to the end of the text, the
# values in front of a boundary run to it (a stop set with "\n") or across it into a dropped line (one without)
SYNTH = "\n".join("k=v%d %s k=w%d" % (i % 5, "keep" if i % 2 == 0 else "drop", i % 3) for i in range(41)) + " k=end"


class Where:
    """the judge's answer for value patterns filtered by queries and a window of lines — and the ONE packed block a call makes of
    them: the terms' hits in front, the value patterns' behind (hit_off[n_terms] != 0 unless no term has a hit)"""

    def __init__(self, key, o, T, patterns, queries, where_of, window=EVERY_LINE, stop=None, max_len=None):
        self.queries, self.where_of, self.window = queries, np.asarray(where_of, np.int32), window
        self.terms = [ia.as_chars(t) for qu in queries for word in ("all", "any", "none") for t in as_list(qu.get(word, ()))]
        self.kinds = np.array([k for qu in queries for k, word in enumerate(("all", "any", "none")) for _ in as_list(qu.get(word, ()))], np.uint8)
        self.query_off = np.concatenate([[0], np.cumsum([sum(len(as_list(qu.get(w, ()))) for w in ("all", "any", "none")) for qu in queries])])
        self.query_off = self.query_off.astype(np.int32)
        self.patterns = [ia.as_chars(p) for p in patterns]
        self.n_terms, self.n, self.q = len(self.terms), len(self.patterns), len(queries)
        ch, off = ia.pack_patterns(self.terms + self.patterns)
        self.ch, self.off = np.ascontiguousarray(ch), off.astype(np.int32)
        batch_key = "%s where %r | %r" % (key, [ia.chars_to_str(t) for t in self.terms], [ia.chars_to_str(p) for p in self.patterns])
        self.packed, self.hit_off, self.status, _, self.counts = expected_packed(batch_key, o, self.ch, self.off, -1)
        nt = self.n_terms
        # the lines of every query: judge_lines per term, then the set formula of fmx_match_query_batch
        tl, tl_off, _ = judge_lines(T, self.packed, self.hit_off[:nt + 1], 0)
        per_term = [tl[tl_off[t]:tl_off[t + 1]] for t in range(nt)]
        self.query_lines = []
        for Q in range(self.q):
            terms = range(self.query_off[Q], self.query_off[Q + 1])
            alls = [per_term[t] for t in terms if self.kinds[t] == ALL]
            anys = [per_term[t] for t in terms if self.kinds[t] == ANY]
            nones = [per_term[t] for t in terms if self.kinds[t] == NONE]
            res = None
            for a in alls:
                res = a if res is None else np.intersect1d(res, a)
            if anys:
                u = np.unique(np.concatenate(anys))
                res = u if res is None else np.intersect1d(res, u)
            if res is None:  # NONE filters, it does not enumerate the text
                res = np.zeros(0, np.int32)
            for a in nones:
                res = np.setdiff1d(res, a)
            self.query_lines.append(np.asarray(res, np.int32))
        self.line_off = np.concatenate([[0], np.cumsum([len(u) for u in self.query_lines])]).astype(np.int64)
        self.lines = np.concatenate(self.query_lines + [np.zeros(0, np.int32)]).astype(np.int32)
        # the filter: a hit belongs to the line of its first character
        lo, hi = window
        kept, flags = [], []
        for i in range(self.n):
            h = self.packed[self.hit_off[nt + i]:self.hit_off[nt + i + 1]]
            L = np.searchsorted(T, h, side="left")
            keep = (L >= lo) & (L < hi)
            if self.where_of[i] >= 0:
                keep &= np.isin(L, self.query_lines[self.where_of[i]])
            kept.append(h[keep])
            flags.append(keep)
        self.keep = np.concatenate(flags + [np.zeros(0, bool)])  # per hit of the value patterns, in the packed order
        self.kept = np.array([len(k) for k in kept], np.int32)
        self.kept_off = np.concatenate([[0], np.cumsum(self.kept)]).astype(np.int64)
        self.kept_locs = np.concatenate(kept + [np.zeros(0, np.int32)]).astype(np.int32)
        self.occurrences, self.term_status = self.counts[nt:], self.status[:nt]
        self.lens = np.diff(self.off)[nt:]
        self.values = judge_values(o, self.kept_locs, self.kept_off, self.lens, stop, max_len) if stop is not None else None
        for a in (self.kinds, self.query_off, self.line_off, self.lines, self.kept, self.kept_off, self.kept_locs):
            a.setflags(write=False)

    def term_arrays(self):
        ch, off = ia.pack_patterns(self.terms)
        return np.ascontiguousarray(ch), off.astype(np.int32)

    def pattern_arrays(self):
        ch, off = ia.pack_patterns(self.patterns)
        return np.ascontiguousarray(ch), off.astype(np.int32)


class Trimmed:
    """a Where looked at through its first n_hits slots only (n_hits below hit_off[n]: the hits behind are ignored)"""

    def __init__(self, w, n_hits):
        first = int(w.hit_off[w.n_terms])
        slots = first + np.arange(len(w.keep))
        keep = w.keep & (slots < n_hits)
        ends = np.clip(w.hit_off[w.n_terms:] - first, 0, None)
        self.kept_off = np.concatenate([[0], np.cumsum(keep)])[ends].astype(np.int64)
        self.kept_locs = w.packed[first:][keep].astype(np.int32)
        self.kept = np.diff(self.kept_off).astype(np.int32)
        for name in ("n", "q", "n_terms", "where_of", "window", "line_off", "lines", "hit_off", "packed"):
            setattr(self, name, getattr(w, name))


def as_list(group):
    return [group] if isinstance(group, str) else list(group)


def check_kept(got, want, what, tail=None):
    """got = (kept_off, kept_locs), kept_locs possibly longer than the answer: IN ORDER, and what lies behind keeps `tail`"""
    kept_off, kept_locs = got
    assert (kept_off == want.kept_off).all(), "%s: kept_off %r, expected %r" % (what, kept_off[:6], want.kept_off[:6])
    total = int(want.kept_off[-1])
    bad = np.flatnonzero(kept_locs[:total] != want.kept_locs)
    assert len(bad) == 0, "%s: %d kept hits differ, first at %r" % (what, len(bad), bad[:5])
    if tail is not None:
        assert (kept_locs[total:] == tail).all(), what + ": stored beyond kept_off[n]"


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "hit_filter_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "hit_filter_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("hit_filter_hostsim")


def run_hostsim(simdir, w, T, extra_hits=0, max_fences=4096, sanitize=False, n_hits=None):
    """the stages' mirror over the judge's packed block, line table and query lines; (kept_off, kept_locs of n_hits slots).  The
    value patterns' part of the block begins at hit_off[n_terms]; extra_hits slots behind hit_off[n] hold no hit; n_hits: fewer
    slots than hits (w is a Trimmed then)."""
    n_hits = int(w.hit_off[-1]) + extra_hits if n_hits is None else n_hits
    locs = np.concatenate([w.packed, np.full(extra_hits, SENT, np.int32)]).astype(np.int32)[:n_hits]
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    head = np.array([w.n, w.q, n_hits, len(T), w.window[0], w.window[1], max_fences, len(w.lines)], np.int64)
    with open(src, "wb") as f:
        for a in (head, w.where_of, w.line_off, w.lines, np.asarray(T, np.int32), w.hit_off[w.n_terms:], locs):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.uint8)
    kept_off = raw[:(w.n + 1) * 8].view(np.int64)
    kept_locs = raw[(w.n + 1) * 8:].view(np.int32)
    assert len(kept_locs) == n_hits
    return kept_off, kept_locs


def sim_case(simdir, key, o, T, patterns, queries, where_of, window=EVERY_LINE, what=None, **kw):
    w = Where(key, o, T, patterns, queries, where_of, window)
    check_kept(run_hostsim(simdir, w, T, **kw), w, what or "%s %r in %r" % (key, where_of, window), tail=SIM_SENT)
    return w


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


@pytest.fixture(scope="module")
def synth():
    o = orc.OracleFmIndex(SYNTH, 4, True)
    return o, judge_table(o, "\n")


def assert_named(w, hits, kept, values, top):
    """the fixture's figures (plain Python over the text gives them: tests/golden/HDFS_2k_multichar.log), on the JUDGE's answer"""
    assert w.occurrences[0] == hits and w.kept[0] == kept, (w.occurrences[0], w.kept[0])
    got = w.values.strings(0)
    assert len(got) == values and sum(c for _, c in got) == kept, (len(got), sum(c for _, c in got))
    assert sorted(got, key=lambda vc: -vc[1])[:len(top)] == top


def test_named_cases(simdir, hd):
    """"blk_" where the line holds "terminating": 2,468 hits, 310 kept, 310 values; "INFO " cut at " \\t\\r\\n:" where the line holds
    "blk_" and not "PacketResponder": 1,920 hits, 1,317 kept, 248 values, dfs.FSNamesystem 525 times.  The judge (quirk rows and all:
    the reference's answers) gives exactly the figures plain Python over the text gives."""
    o, T = hd
    text_lines = HD.split("\n")
    for pattern, stop, max_len, query, hits, kept, values, top in NAMED:
        w = Where("hd16", o, T, [pattern], [query], [0], EVERY_LINE, stop, max_len)
        assert_named(w, hits, kept, values, top)
        ok = [all(t in ln for t in query.get("all", ())) and not any(t in ln for t in query.get("none", ())) for ln in text_lines]
        assert w.kept[0] == sum(ln.count(pattern) for ln, keep in zip(text_lines, ok) if keep)  # (no pattern overlaps itself here)
        for fences in (4096, 3):
            check_kept(run_hostsim(simdir, w, T, max_fences=fences), w, "%r, %d fences" % (pattern, fences), tail=SIM_SENT)
        # ... and the values stage's mirror over the kept hits: the answer of the whole call
        got, _ = run_values_hostsim(simdir, w.values, w.kept_locs, w.kept_off, w.lens, stop, max_len, o.getInputLength() - 1)
        check_values(got, w.values, "values of the kept hits of %r" % pattern)


def test_synthetic_text_alternating_lines(simdir, synth):
    o, T = synth
    n_lines = judge_n_lines(T, len(SYNTH))
    assert n_lines == 41 and len(T) == 40
    # "k=" stands twice in every line and three times in the last one; "\nk=" starts in the line in front of the one it names
    for stop, last in ((" \n", "end"), (" ", "end")):
        w = Where("synth", o, T, ["k=", "\nk=", "k=", "keep"], [dict(all=["keep"]), dict(all=["drop"])], [0, 0, 1, -1], EVERY_LINE, stop, 8)
        assert w.kept.tolist() == [2 * 21 + 1, 20, 2 * 20, 21] and w.occurrences.tolist() == [83, 40, 83, 21]
        assert (w.query_lines[0] == np.arange(0, 41, 2)).all() and (w.query_lines[1] == np.arange(1, 41, 2)).all()
        first_line, last_line = np.searchsorted(T, w.kept_locs[:43]).min(), np.searchsorted(T, w.kept_locs[:43]).max()
        assert first_line == 0 and last_line == 40  # hits in the first and in the last line
        vals = dict(w.values.strings(0))
        assert vals[last] == 1  # the value that runs to the end of the text
        # the last value of a line runs to the boundary; without "\n" in the stop set it runs across it into a dropped line
        assert ("w0" in vals) == ("\n" in stop) and any(v.startswith("w0\nk=v") for v in vals) == ("\n" not in stop)
        # "\nk=" is found in the EVEN lines' boundary: the values are those of the odd (dropped) lines
        assert {v for v, _ in w.values.strings(1)} == {"v%d" % (i % 5) for i in range(1, 41, 2)}
        for fences in (4096, 0, 1, 7):
            check_kept(run_hostsim(simdir, w, T, extra_hits=3, max_fences=fences), w, "synth, %d fences" % fences, tail=SIM_SENT)
    # an off-by-one in the line search, or a compaction that is not stable, changes this answer
    assert (np.diff(np.searchsorted(T, w.kept_locs[:43])) != 0).any() and not (np.diff(w.kept_locs[:43]) > 0).all()


def test_where_of_mixes_and_windows(simdir, hd):
    o, T = hd
    n_lines = judge_n_lines(T, len(HD))
    queries = [dict(all=["terminating"]), dict(all=["blk_"], none=["PacketResponder"]), dict(all=["zzzq#"]), dict(none=["INFO"]), dict(),
               dict(any=["WARN", "Receiving"], none="src:")]
    patterns = ["blk_", "/10.", "INFO ", "WARN", " ", "1", "blk_", "zzzq#", "dfs.", ":"]
    where_of = [0, 0, 1, -1, 2, 3, 4, 0, 5, -1]
    w = sim_case(simdir, "hd16 mix", o, T, patterns, queries, where_of, extra_hits=37)
    assert w.kept[0] == 310 and w.kept[2] == 1317 and w.kept[3] == w.occurrences[3] > 0  # -1: every hit
    assert w.kept[4] == w.kept[5] == w.kept[6] == w.kept[7] == 0 and w.occurrences[4] > 30000  # no lines; NONE only; no terms; no hits
    assert 0 < w.kept[8] < w.occurrences[8] and w.kept[9] == w.occurrences[9]
    assert len(w.query_lines[2]) == len(w.query_lines[3]) == len(w.query_lines[4]) == 0 and w.hit_off[w.n_terms] > 0
    windows = [(7, 7), (0, 1), (n_lines - 1, n_lines), (n_lines + 5, INT32_MAX), (0, 0), (100, 1900), (1999, INT32_MAX)]
    for window in windows:
        ww = sim_case(simdir, "hd16 mix", o, T, patterns, queries, where_of, window, extra_hits=1, max_fences=64)
        if window[0] == window[1] or window[0] > n_lines:
            assert ww.kept.sum() == 0
        elif window[1] - window[0] == 1:
            assert 0 < ww.kept[9] < 20  # the ":" of one line
    # no query at all, a window alone; and no terms in front: hit_off[0] == 0
    w0 = sim_case(simdir, "hd16 mix", o, T, patterns, [], [-1] * len(patterns), (5, 1500))
    assert w0.n_terms == 0 and w0.hit_off[0] == 0 and 0 < w0.kept[0] < w0.occurrences[0]


def test_n_hits_on_the_tile_edges(simdir, hd):
    """n_hits trimmed to 0, 1, 1,023, 1,024 and 1,025 value hits and to whole tiles of slots, with and without terms in front"""
    o, T = hd
    for queries, where_of in (([], [-1, -1, -1]), ([dict(all=["terminating"]), dict(any=["WARN", "/10.250.1"])], [1, 0, -1])):
        w = Where("hd16 edges", o, T, [" ", "blk_", "1"], queries, where_of, (3, 1990))
        first, total = int(w.hit_off[w.n_terms]), int(w.hit_off[-1])
        assert total - first > 5 * 1024
        edges = [first + k for k in (0, 1, 1023, 1024, 1025)] + [k for k in (1024 * (first // 1024 + 1), 1024 * (first // 1024 + 3) + 1)]
        for n_hits in edges + [total - 1]:
            t = Trimmed(w, n_hits)
            assert t.kept.sum() <= n_hits - first and (t.kept.sum() > 0 or n_hits <= first + 1025)
            got = run_hostsim(simdir, t, T, n_hits=n_hits)
            check_kept(got, t, "n_hits %d of %d, %d in front" % (n_hits, total, first), tail=SIM_SENT)
    assert Trimmed(w, total).kept.tolist() == w.kept.tolist()


def test_sanitized_build(simdir, hd, synth):
    """the stand-alone program once more under AddressSanitizer and UBSan (nothing loaded into python is run under a sanitizer)"""
    o, T = hd
    sim_case(simdir, "hd16", o, T, ["blk_"], [NAMED[0][3]], [0], sanitize=True)
    sim_case(simdir, "hd16 mix", o, T, ["blk_", "zzzq#", ":"], [dict(all=["zzzq#"]), dict(any=["WARN"])], [1, 0, -1], (3, 1200), extra_hits=5,
             max_fences=3, sanitize=True)
    os_, Ts = synth
    sim_case(simdir, "synth", os_, Ts, ["k=", "\nk="], [dict(all=["keep"])], [0, 0], (0, 41), extra_hits=2, max_fences=0, sanitize=True)


def test_merged_batch_is_sanitizer_clean(tmp_path):
    """tests/cpp/san_merged_batch.cpp: the checks and the merge of terms and value patterns into ONE batch
    (index4j_amd/csrc/fmx_host_batch.cpp, the file the library is linked from) as a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer, against a merge written out naively, every array exactly as large as the contract makes it"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "index4j_amd", "csrc")
    exe = str(tmp_path / "san_merged_batch")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + csrc, os.path.join(root, "tests", "cpp", "san_merged_batch.cpp"),
           os.path.join(csrc, "fmx_host_batch.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.count(" ok: ") == 81 and "merged batch: 81 cases ok" in r.stdout, r.stdout[-3000:]


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    for name in ("fmx_hits_in_lines_scratch_bytes", "fmx_hits_in_lines_dev", "fmx_field_values_where_batch", "fmx_field_values_where_class_batch"):
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("This is a long string\nand one more line\n", 4, True, device=None)
    where_of = np.array([0, -1, 1], np.int32)
    line_off, hit_off, ids = np.zeros(3, np.int64), np.zeros(4, np.int64), np.zeros(8, np.int32)
    kept_off, kept_locs = np.full(4, SENT, np.int64), np.full(8, SENT, np.int32)
    dev = ia.lib.fmx_hits_in_lines_dev

    def dcall(h=fm._h, n=3, wo=where_of, q=2, loff=line_off, lo=0, hi=INT32_MAX, hoff=hit_off, locs=ids, n_hits=2, koff=kept_off, klocs=kept_locs):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return dev(h, n, p(wo), q, p(loff), ids.ctypes.data, lo, hi, p(hoff), p(locs), n_hits, p(koff), p(klocs), None, 0, None)

    assert dcall() == E_NO_DEVICE
    for bad in (dict(h=None), dict(n=-1), dict(q=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(wo=None), dict(hoff=None), dict(locs=None),
                dict(koff=None), dict(klocs=None), dict(loff=None), dict(lo=-1), dict(hi=-1), dict(lo=5, hi=4),
                dict(wo=np.array([0, -2, 1], np.int32)), dict(wo=np.array([0, 2, 1], np.int32)), dict(q=1)):
        assert dcall(**bad) == E_ARG, bad
    assert (kept_off == SENT).all() and (kept_locs == SENT).all()
    sb = ia.lib.fmx_hits_in_lines_scratch_bytes
    assert sb(0, 5) == 0 and sb(5, 0) == 0 and sb(5, 1 << 31) == 0 and sb(-1, 5) == 0
    assert sb(3, 1000) >= 8 * 1000 and sb(3, 1000) % 256 == 0 and sb(3, 1000) < 64 * 1000
    ch, off = ia.pack_patterns(["is", "long", "line"])
    tch, toff = ia.pack_patterns(["string", "one", "more"])
    off, toff = off.astype(np.int32), toff.astype(np.int32)
    qoff, kinds = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.uint8)
    stop = ia.as_chars(" \n")
    val_off = np.full(4, SENT, np.int64)
    bufs = [C.c_void_p(0x1234) for _ in range(3)]
    host = ia.lib.fmx_field_values_where_batch

    def call(h=fm._h, off_=off, n=3, toff_=toff, nt=3, qoff_=qoff, kinds_=kinds, q=2, wo=where_of, lo=0, hi=INT32_MAX, n_stop=2, max_len=8,
             voff=val_off, out=0):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        outs = [None if out == k + 1 else C.byref(bufs[k]) for k in range(3)]
        return host(h, ch.ctypes.data, p(off_), n, tch.ctypes.data, p(toff_), nt, p(qoff_), p(kinds_), q, p(wo), lo, hi, stop.ctypes.data, n_stop,
                    max_len, p(voff), *outs, None, None, None, None)

    assert call() == E_NO_DEVICE
    assert all(b.value is None for b in bufs) and (val_off == SENT).all()  # NULL on every failure, nothing written
    for bad in (dict(h=None), dict(n=-1), dict(nt=-1), dict(q=-1), dict(off_=None), dict(toff_=None), dict(qoff_=None), dict(kinds_=None),
                dict(wo=None), dict(voff=None), dict(out=1), dict(out=2), dict(out=3), dict(lo=-1), dict(lo=3, hi=2), dict(max_len=0),
                dict(max_len=65), dict(n_stop=65), dict(n_stop=-1),
                dict(qoff_=np.array([1, 2, 3], np.int32)), dict(qoff_=np.array([0, 3, 2], np.int32)), dict(qoff_=np.array([0, 1, 2], np.int32)),
                dict(kinds_=np.array([0, 3, 1], np.uint8)), dict(wo=np.array([2, 0, 0], np.int32)), dict(wo=np.array([-2, 0, 0], np.int32)),
                dict(off_=np.array([0, 4, 2, 10], np.int32)), dict(toff_=np.array([-1, 6, 9, 13], np.int32))):
        for b in bufs:
            b.value = 0x1234
        assert call(**bad) == E_ARG, bad
        assert all(b.value is None or bad.get("out") == k + 1 for k, b in enumerate(bufs)) and (val_off == SENT).all()
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert call(h=h) == E_ARG and dcall(h=h) == E_ARG
    # the class twin judges its arrays the same way
    alt, pos_off, pat_off = ia.pack_class_patterns([ia.ignore_case("is")])
    talt, tpos, tpat = ia.pack_class_patterns([ia.ignore_case("one")])
    klass = ia.lib.fmx_field_values_where_class_batch

    def ccall(h=fm._h, max_ranges=16, wo=np.array([0], np.int32), hi=INT32_MAX, tpat_=tpat):
        a = lambda x: np.ascontiguousarray(x).ctypes.data  # noqa: E731
        keep = [np.ascontiguousarray(x) for x in (alt, pos_off, pat_off, talt, tpos, tpat_)]
        return klass(h, a(keep[0]), a(keep[1]), len(pos_off) - 1, a(keep[2]), 1, a(keep[3]), a(keep[4]), len(tpos) - 1, a(keep[5]), 1, max_ranges,
                     np.array([0, 1], np.int32).ctypes.data, np.array([0], np.uint8).ctypes.data, 1, wo.ctypes.data, 0, hi, stop.ctypes.data, 2, 8,
                     val_off.ctypes.data, C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2]), None, None, None, None)

    assert ccall() == E_NO_DEVICE
    for bad in (dict(h=None), dict(max_ranges=0), dict(max_ranges=1 << 20), dict(wo=np.array([1], np.int32)), dict(hi=-4),
                dict(tpat_=np.array([0, 9], np.int32))):
        assert ccall(**bad) == E_ARG, bad
    assert (val_off == SENT).all()
    # the Python mirrors: an empty pattern or term raises as field_values("") does, before anything runs; without a device the call says so
    for kw in (dict(pattern=""), dict(pattern="is", where=dict(all=[""])), dict(pattern="is", where=dict(all="is", none=["x", ""]))):
        with pytest.raises(IndexError, match="ArrayIndexOutOfBoundsException"):
            fm.field_values(**kw, lines=(0, 2))
    with pytest.raises(ValueError):
        fm.field_values("is", where=dict(every=["x"]))
    for run in (lambda: fm.field_values("is", where=dict(all="long")), lambda: fm.field_values("is", lines=(0, 1)),
                lambda: fm.count_where("is", where=dict(any=["long", "one"]), ignore_case=True)):
        with pytest.raises(ia.FmxError) as e:
            run()
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        fm.field_values_where_batch(ch, off, tch, toff, qoff, kinds, where_of[:2], " ", 8)

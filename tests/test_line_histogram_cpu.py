"""Matching lines and hits per bucket of lines, the timeline of a log search (fmx_lines_histogram_dev, fmx_hits_histogram_dev,
fmx_line_histogram_batch, fmx_hit_histogram_where_batch) on the CPU: the functions the kernels of index4j_amd/csrc/fmx_line_hist.hip
run — fm_hist_rank, fm_hist_between, fm_hist_bucket, fm_hist_key*, fm_hist_count (index4j_amd/csrc/fmx_line_hist.hpp), with
fm_hit_tile / fm_hit_pattern and fm_line_of over fences — compiled for the host and driven by a mirror of the stages
(tests/line_hist_hostsim.cpp, a stand-alone program: its `self` mode checks the functions at their edges, its `lines` and `hits`
modes run the stages lane by lane), built once plain and once with -fsanitize=address,undefined and run directly, as a program.

The judge is np.searchsorted(edges, lines, "right") - 1 (judge_bins) over what the existing judges give: the lines of the queries
and the kept hits are Where's (tests/test_field_values_where_cpu.py), a hit's line np.searchsorted on judge_table's line table
(tests/test_match_lines_cpu.py).  The GPU suite runs the kernels and the host forms themselves
(tests/test_gpu_line_histogram.py, which shares the helpers below)."""
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_field_values_where_cpu import EVERY_LINE, INT32_MAX, SENT, SYNTH, Trimmed, Where
from test_match_lines_cpu import judge_n_lines, judge_table

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SIM_SENT, SIM_PAD = -77, 8  # line_hist_hostsim.cpp's kSentinel and kPad
EDGES_250 = np.arange(0, 2001, 250, dtype=np.int32)
# edges that cut the fixture unevenly: an empty bucket, a bucket of one line, the first lines and the last ones outside, an edge
# beyond the line count
EDGES_UNEVEN = np.array([3, 4, 4, 100, 101, 1024, 1990, 1990, 1999], np.int32)
EDGES_BEYOND = np.array([0, 7, 1999, 2000, 2500, 2 ** 31 - 1], np.int32)

# the fixture's four named cases (HDFS_2k_multichar.log, 2,000 lines, edges 0, 250, ..., 2000): (form, pattern, query, per bucket)
NAMED_HIST = [
    ("lines", None, dict(all=["terminating"]), [54, 14, 40, 26, 33, 51, 47, 45]),
    ("lines", None, dict(all=["blk_"], none=["PacketResponder"]), [139, 225, 161, 199, 184, 162, 164, 163]),
    ("hits", "blk_", None, [250, 314, 255, 301, 285, 284, 493, 286]),
    ("hits", "blk_", dict(all=["terminating"]), [54, 14, 40, 26, 33, 51, 47, 45]),
]


def judge_bins(edges, lines):
    """the counters of one row: np.searchsorted(edges, lines, "right") - 1 is the bucket of a line; -1 (below the first edge) and
    B (at or above the last) are no bucket.  Of equal edges the last one takes the line, so the empty bucket stays empty."""
    edges = np.asarray(edges, np.int64)
    B = len(edges) - 1
    b = np.searchsorted(edges, np.asarray(lines, np.int64), "right") - 1
    return np.bincount(b[(b >= 0) & (b < B)], minlength=B).astype(np.int32)[:B]


def judge_line_hist(w, edges):
    """(q, B): the lines of every query of a Where per bucket"""
    return np.array([judge_bins(edges, ql) for ql in w.query_lines], np.int32).reshape(w.q, len(edges) - 1)


def judge_hit_hist(w, T, edges):
    """(n, B): the KEPT hits of every value pattern of a Where (or Trimmed) per bucket; a hit belongs to the line of its first
    character"""
    rows = [judge_bins(edges, np.searchsorted(T, w.kept_locs[a:b], side="left")) for a, b in zip(w.kept_off[:-1], w.kept_off[1:])]
    return np.array(rows, np.int32).reshape(w.n, len(edges) - 1)


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "line_hist_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "line_hist_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("line_hist_hostsim")


def _run(simdir, mode, arrays, rows, B, sanitize):
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), mode, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = np.fromfile(dst, np.int32)
    assert len(out) == rows * B + SIM_PAD and (out[rows * B:] == SIM_SENT).all()
    return out[:rows * B].reshape(rows, B)


def run_lines_sim(simdir, line_off, lines, edges, sanitize=False):
    """the lines form's two kernels over packed ascending lists; (q, B)"""
    q = len(line_off) - 1
    head = np.array([q, len(edges), len(lines)], np.int64)
    return _run(simdir, "lines", (head, np.asarray(line_off, np.int64), np.asarray(lines, np.int32), np.asarray(edges, np.int32)), q,
                len(edges) - 1, sanitize)


def run_hits_sim(simdir, T, n, hit_off, locs, edges, n_hits=None, extra_hits=0, max_fences=4096, sanitize=False):
    """the hits form's stages over a packed block (hit_off[0] may be non-zero; extra_hits slots behind hit_off[n] hold no hit;
    n_hits: fewer slots than hits); (n, B)"""
    n_hits = int(hit_off[-1]) + extra_hits if n_hits is None else n_hits
    locs = np.concatenate([locs, np.full(extra_hits, SENT, np.int32)]).astype(np.int32)[:n_hits]
    head = np.array([n, n_hits, len(T), max_fences, len(edges)], np.int64)
    return _run(simdir, "hits", (head, np.asarray(T, np.int32), np.asarray(hit_off, np.int64), locs, np.asarray(edges, np.int32)), n,
                len(edges) - 1, sanitize)


def sim_kept(simdir, w, T, edges, **kw):
    """the hits form over the KEPT hits of a Where: what the host form hands the stage when a pattern asks for a query"""
    return run_hits_sim(simdir, T, w.n, w.kept_off, w.kept_locs, edges, **kw)


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


def named_where(o, T, form, pattern, query):
    if form == "lines":
        return Where("hd16", o, T, [], [query], [])
    return Where("hd16", o, T, [pattern], [query] if query else [], [0 if query else -1])


def test_per_item_functions(simdir):
    """the bucket of a line at every edge relation, the rank difference over empty, one-entry and duplicate lists, the key's packing
    at 1, 32 and 33 bits: line_hist_hostsim.cpp's self_checks, plain and under AddressSanitizer and UBSan"""
    for sanitize in (False, True):
        r = subprocess.run([hostsim_exe(simdir, sanitize), "self"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_judge_bins_at_every_edge_relation():
    """the Python judge itself, on the cases the C++ self-checks name"""
    e = [2, 5, 5, 8, 1000]
    assert judge_bins(e, [0, 1]).tolist() == [0, 0, 0, 0] and judge_bins(e, [2, 3, 4]).tolist() == [3, 0, 0, 0]
    assert judge_bins(e, [5, 5, 7, 8, 999, 1000, 2 ** 31 - 1]).tolist() == [0, 0, 3, 2]
    assert judge_bins([3, 3], [2, 3, 4]).tolist() == [0] and judge_bins([0, 1], []).tolist() == [0]


def test_named_cases(simdir, hd):
    """the four named cases: the judge over the oracle gives exactly what a plain string scan of the fixture gives, and the stages'
    mirror gives the judge's answer (also through few fences and under the sanitizers)"""
    o, T = hd
    text_lines = HD.split("\n")
    assert judge_n_lines(T, len(HD)) == 2000
    for form, pattern, query, per_bucket in NAMED_HIST:
        w = named_where(o, T, form, pattern, query)
        ok = [all(t in ln for t in (query or {}).get("all", ())) and not any(t in ln for t in (query or {}).get("none", ())) for ln in text_lines]
        if form == "lines":
            scan = [sum(ok[a:b]) for a, b in zip(EDGES_250[:-1], EDGES_250[1:])]
            want = judge_line_hist(w, EDGES_250)
            got = run_lines_sim(simdir, w.line_off, w.lines, EDGES_250)
            assert (run_lines_sim(simdir, w.line_off, w.lines, EDGES_250, sanitize=True) == want).all()
        else:  # (no pattern overlaps itself here)
            scan = [sum(ln.count(pattern) for ln, keep in zip(text_lines[a:b], ok[a:b]) if keep) for a, b in zip(EDGES_250[:-1], EDGES_250[1:])]
            want = judge_hit_hist(w, T, EDGES_250)
            got = sim_kept(simdir, w, T, EDGES_250)
            assert int(want.sum()) == w.kept[0]
            for fences in (3, 0):
                assert (sim_kept(simdir, w, T, EDGES_250, max_fences=fences, extra_hits=5, sanitize=fences == 0) == want).all()
        assert scan == per_bucket and want[0].tolist() == per_bucket and (got == want).all(), (form, pattern, query)
    assert sum(NAMED_HIST[0][3]) == 310 and sum(NAMED_HIST[2][3]) == 2468 and sum(NAMED_HIST[3][3]) == 310


def test_lines_form_lists_and_edge_counts(simdir):
    """lists of 0, 1, 2 and 1,025 entries and one with duplicates; n_edges 2, 3, 257 and on both sides of 4,096; all lines in one
    bucket, all outside the buckets, equal edges"""
    rng = np.random.default_rng(7)
    lists = [np.zeros(0, np.int32), np.array([77], np.int32), np.array([0, 9999], np.int32),
             np.sort(rng.choice(10000, 1025, replace=False)).astype(np.int32), np.sort(rng.integers(0, 50, 300)).astype(np.int32)]
    line_off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    lines = np.concatenate(lists)
    for k, edges in enumerate(([0, 10000], [0, 77, 78], [10000, 20000], [5, 5], [50, 50, 50, 9999], np.linspace(0, 10001, 257).astype(np.int32),
                               np.sort(rng.integers(0, 11000, 4096)), np.sort(rng.integers(0, 11000, 4097)))):
        edges = np.asarray(edges, np.int32)
        want = np.array([judge_bins(edges, a) for a in lists])
        got = run_lines_sim(simdir, line_off, lines, edges, sanitize=k % 3 == 0)
        assert (got == want).all(), edges[:8]
    assert want.sum() > 0 and (np.array([judge_bins([10000, 20000], a) for a in lists]) == 0).all()
    # a list whose every entry is the same line, an edge on it
    same = np.full(40, 6, np.int32)
    assert run_lines_sim(simdir, [0, 40], same, [0, 6, 7, 9]).tolist() == [[0, 40, 0]]


def test_hits_form_mixes_uneven_edges_and_tile_edges(simdir, hd):
    """the where tests' mix over edges that cut the fixture unevenly, raw hits with terms in front (hit_off[0] != 0), a pattern
    without hits between two with hits, and slots trimmed to the tile edges"""
    o, T = hd
    queries = [dict(all=["terminating"]), dict(all=["blk_"], none=["PacketResponder"]), dict(all=["zzzq#"]), dict(none=["INFO"]), dict(),
               dict(any=["WARN", "Receiving"], none="src:")]
    patterns = ["blk_", "/10.", "INFO ", "WARN", " ", "1", "blk_", "zzzq#", "dfs.", ":"]
    w = Where("hd16 mix", o, T, patterns, queries, [0, 0, 1, -1, 2, 3, 4, 0, 5, -1])
    for edges in (EDGES_UNEVEN, EDGES_BEYOND, EDGES_250):
        want = judge_hit_hist(w, T, edges)
        assert (sim_kept(simdir, w, T, edges, extra_hits=37, max_fences=64) == want).all()
        if edges[0] == 0 and edges[-1] >= 2000:
            assert (want.sum(axis=1) == w.kept).all()  # the edges span every line: a row adds up to kept
        else:
            assert (want.sum(axis=1) <= w.kept).all() and want.sum() < w.kept.sum()
    assert want[7].sum() == 0 and want[6].sum() == 0 and want[8].sum() > 0  # no hits; no lines; hits behind them
    # the raw hits of the value patterns, the terms' in front: hit_off + n_terms does not start at 0
    raw = Where("hd16 mix", o, T, patterns, queries, [-1] * len(patterns))
    nt = raw.n_terms
    assert raw.hit_off[nt] > 0 and (raw.kept == raw.occurrences).all()
    want = judge_hit_hist(raw, T, EDGES_UNEVEN)
    assert (run_hits_sim(simdir, T, raw.n, raw.hit_off[nt:], raw.packed, EDGES_UNEVEN, extra_hits=3) == want).all()
    # n_hits trimmed: 0, 1, 1,023, 1,024, 1,025 value hits, whole tiles of slots
    w3 = Where("hd16 edges", o, T, [" ", "blk_", "1"], [dict(all=["terminating"])], [-1, -1, -1], EVERY_LINE)
    first, total = int(w3.hit_off[w3.n_terms]), int(w3.hit_off[-1])
    assert first > 0 and total - first > 5 * 1024
    for n_hits in [first + k for k in (0, 1, 1023, 1024, 1025)] + [1024 * (first // 1024 + 1), 1024 * (first // 1024 + 3) + 1, total - 1]:
        t = Trimmed(w3, n_hits)
        got = run_hits_sim(simdir, T, w3.n, w3.hit_off[w3.n_terms:], w3.packed, EDGES_UNEVEN, n_hits=n_hits, sanitize=n_hits == first + 1025)
        assert (got == judge_hit_hist(t, T, EDGES_UNEVEN)).all(), n_hits
    # one pattern owning every hit
    one = Where("hd16 one", o, T, [" "], [], [-1])
    assert (run_hits_sim(simdir, T, 1, one.hit_off, one.packed, EDGES_BEYOND) == judge_hit_hist(one, T, EDGES_BEYOND)).all()


def test_synthetic_text(simdir):
    """a hit in the first and in the last line, two hits on one line are two"""
    o = orc.OracleFmIndex(SYNTH, 4, True)
    T = judge_table(o, "\n")
    w = Where("synth", o, T, ["k=", "keep"], [dict(all=["keep"])], [0, -1])
    edges = [0, 1, 20, 40, 41]
    want = judge_hit_hist(w, T, edges)
    assert want.tolist() == [[2, 18, 20, 3], [1, 9, 10, 1]]
    for fences in (4096, 0, 1, 7):
        assert (sim_kept(simdir, w, T, edges, max_fences=fences, sanitize=fences == 1) == want).all()
    assert (run_lines_sim(simdir, w.line_off, w.lines, edges) == [[1, 9, 10, 1]]).all()


def test_error_returns_without_a_device():
    """fails on a library without the feature (missing symbols)"""
    E_ARG, E_NO_DEVICE = ia._lib.E_ARG, ia._lib.E_NO_DEVICE
    names = ("fmx_lines_histogram_scratch_bytes", "fmx_hits_histogram_scratch_bytes", "fmx_lines_histogram_dev", "fmx_hits_histogram_dev",
             "fmx_line_histogram_batch", "fmx_line_histogram_class_batch", "fmx_hit_histogram_where_batch", "fmx_hit_histogram_where_class_batch")
    for name in names:
        assert name in ia.SYMBOLS and hasattr(ia.lib, name)
    fm = ia.FmIndex("This is a long string\nand one more line\n", 4, True, device=None)
    edges = np.array([0, 1, 2], np.int32)
    line_off, ids, hit_off = np.zeros(3, np.int64), np.zeros(8, np.int32), np.zeros(4, np.int64)
    hist = np.full(16, SENT, np.int32)
    bad_edges = (dict(e=None), dict(ne=1), dict(ne=-1), dict(e=np.array([-1, 1, 2], np.int32)), dict(e=np.array([0, 2, 1], np.int32)))
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def lcall(h=fm._h, q=2, loff=line_off, lines=ids, e=edges, ne=3, out=hist):
        return ia.lib.fmx_lines_histogram_dev(h, q, p(loff), p(lines), p(e), ne, p(out), None, 0, None)

    def hcall(h=fm._h, n=3, hoff=hit_off, locs=ids, n_hits=2, e=edges, ne=3, out=hist):
        return ia.lib.fmx_hits_histogram_dev(h, n, p(hoff), p(locs), n_hits, p(e), ne, p(out), None, 0, None)

    assert lcall() == E_NO_DEVICE and hcall() == E_NO_DEVICE
    for bad in (dict(h=None), dict(q=-1), dict(loff=None), dict(out=None)) + bad_edges:
        assert lcall(**bad) == E_ARG, bad
    for bad in (dict(h=None), dict(n=-1), dict(n_hits=-1), dict(n_hits=1 << 31), dict(hoff=None), dict(locs=None), dict(out=None)) + bad_edges:
        assert hcall(**bad) == E_ARG, bad
    # (int64) rows * B above 2^27
    big = np.arange((1 << 16) + 2, dtype=np.int32)
    assert lcall(q=1 << 11, e=big, ne=len(big) - 1) == E_NO_DEVICE and lcall(q=(1 << 11) + 1, e=big, ne=len(big) - 1) == E_ARG
    assert hcall(n=1 << 11, e=big, ne=len(big)) == E_ARG and hcall(n=1 << 11, e=big, ne=len(big) - 1) == E_NO_DEVICE
    assert (hist == SENT).all()
    lsb, hsb = ia.lib.fmx_lines_histogram_scratch_bytes, ia.lib.fmx_hits_histogram_scratch_bytes
    assert lsb(0, 5) == 0 and lsb(5, 1) == 0 and lsb(-1, 5) == 0 and lsb((1 << 11) + 1, len(big) - 1) == 0
    assert lsb(300, 61) >= 300 * 61 * 8 + 61 * 4 and lsb(300, 61) % 256 == 0 and lsb(300, 61) < 2 * 300 * 61 * 8
    assert hsb(0, 5, 3) == 0 and hsb(5, 0, 3) == 0 and hsb(5, 1 << 31, 3) == 0 and hsb(5, 9, 1) == 0 and hsb(1 << 11, 9, len(big)) == 0
    assert hsb(3, 1000, 61) >= 16 * 1000 + 61 * 4 and hsb(3, 1000, 61) % 256 == 0 and hsb(3, 1000, 61) < 64 * 1000
    # the host forms
    ch, off = ia.pack_patterns(["is", "long", "line"])
    tch, toff = ia.pack_patterns(["string", "one", "more"])
    off, toff = off.astype(np.int32), toff.astype(np.int32)
    qoff, kinds = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.uint8)
    where_of = np.array([0, -1, 1], np.int32)
    counts = np.full(3, SENT, np.int32)

    def lines_host(h=fm._h, off_=off, n=3, qoff_=qoff, kinds_=kinds, q=2, e=edges, ne=3, out=hist):
        return ia.lib.fmx_line_histogram_batch(h, ch.ctypes.data, p(off_), n, p(qoff_), p(kinds_), q, p(e), ne, p(out), p(counts), None, None)

    def hits_host(h=fm._h, off_=off, n=3, toff_=toff, nt=3, qoff_=qoff, kinds_=kinds, q=2, wo=where_of, e=edges, ne=3, out=hist):
        return ia.lib.fmx_hit_histogram_where_batch(h, ch.ctypes.data, p(off_), n, tch.ctypes.data, p(toff_), nt, p(qoff_), p(kinds_), q, p(wo), p(e),
                                                    ne, p(out), None, p(counts), None, None)

    assert lines_host() == E_NO_DEVICE and hits_host() == E_NO_DEVICE
    query_bad = (dict(qoff_=None), dict(kinds_=None), dict(qoff_=np.array([1, 2, 3], np.int32)), dict(qoff_=np.array([0, 3, 2], np.int32)),
                 dict(qoff_=np.array([0, 1, 2], np.int32)), dict(kinds_=np.array([0, 3, 1], np.uint8)), dict(q=-1), dict(h=None), dict(n=-1),
                 dict(off_=None), dict(out=None), dict(off_=np.array([0, 4, 2, 10], np.int32)))
    for bad in query_bad + bad_edges:
        assert lines_host(**bad) == E_ARG, bad
    for bad in query_bad + bad_edges + (dict(nt=-1), dict(toff_=None), dict(wo=None), dict(wo=np.array([2, 0, 0], np.int32)),
                                        dict(wo=np.array([-2, 0, 0], np.int32)), dict(toff_=np.array([-1, 6, 9, 13], np.int32))):
        assert hits_host(**bad) == E_ARG, bad
    assert (hist == SENT).all() and (counts == SENT).all()
    sa = ia.SuffixArray("banana", device=None, build_device=-1)
    sa.construct()
    rrr = ia.RrrVector([1, 0, 1, 1, 0] * 40, device=None)
    wt = ia.WaveletFixedBlockBoosting("abracadabra", device=None)
    for h in (sa._h, rrr._h, wt._h):
        assert lines_host(h=h) == E_ARG and hits_host(h=h) == E_ARG and lcall(h=h) == E_ARG and hcall(h=h) == E_ARG
    # the class twins judge their arrays the same way
    alt, pos_off, pat_off = (np.ascontiguousarray(x) for x in ia.pack_class_patterns([ia.ignore_case("is")]))
    talt, tpos, tpat = (np.ascontiguousarray(x) for x in ia.pack_class_patterns([ia.ignore_case("one")]))
    q1, k1, w1 = np.array([0, 1], np.int32), np.array([0], np.uint8), np.array([0], np.int32)

    def lines_class(h=fm._h, max_ranges=16, e=edges, ne=3, pat_=pat_off):
        return ia.lib.fmx_line_histogram_class_batch(h, p(alt), p(pos_off), len(pos_off) - 1, p(pat_), 1, max_ranges, p(q1), p(k1), 1, p(e), ne,
                                                     p(hist), None, None, None)

    def hits_class(h=fm._h, max_ranges=16, e=edges, ne=3, wo=w1, tpat_=tpat):
        return ia.lib.fmx_hit_histogram_where_class_batch(h, p(alt), p(pos_off), len(pos_off) - 1, p(pat_off), 1, p(talt), p(tpos), len(tpos) - 1,
                                                          p(tpat_), 1, max_ranges, p(q1), p(k1), 1, p(wo), p(e), ne, p(hist), None, None, None, None)

    assert lines_class() == E_NO_DEVICE and hits_class() == E_NO_DEVICE
    for bad in (dict(h=None), dict(max_ranges=0), dict(max_ranges=1 << 20)) + bad_edges:
        assert lines_class(**bad) == E_ARG and hits_class(**bad) == E_ARG, bad
    assert lines_class(pat_=np.array([0, 9], np.int32)) == E_ARG and hits_class(tpat_=np.array([0, 9], np.int32)) == E_ARG
    assert hits_class(wo=np.array([1], np.int32)) == E_ARG and (hist == SENT).all()
    # the Python mirrors: an empty pattern or term raises as match_query("") does, before anything runs; without a device the call says so
    for run in (lambda: fm.line_histogram([0, 1], all=[""]), lambda: fm.hit_histogram("", [0, 1]),
                lambda: fm.hit_histogram("is", [0, 1], where=dict(all="is", none=["x", ""]))):
        with pytest.raises(IndexError, match="ArrayIndexOutOfBoundsException"):
            run()
    with pytest.raises(ValueError):
        fm.hit_histogram("is", [0, 1], where=dict(every=["x"]))
    for run in (lambda: fm.line_histogram([0, 1, 2], all="long"), lambda: fm.hit_histogram("is", [0, 2]),
                lambda: fm.hit_histogram("is", [0, 2], where=dict(any=["long", "one"]), ignore_case=True),
                lambda: fm.line_histogram([0, 2], any=["long", "one"], ignore_case=True)):
        with pytest.raises(ia.FmxError) as e:
            run()
        assert e.value.code == E_NO_DEVICE
    for run in (lambda: fm.line_histogram([0], all="long"), lambda: fm.hit_histogram("is", [2, 1])):
        with pytest.raises(ia.FmxError) as e:
            run()
        assert e.value.code == E_ARG
    with pytest.raises(ValueError):
        fm.hit_histogram_where_batch(ch, off, tch, toff, qoff, kinds, where_of[:2], edges)
    assert INT32_MAX == 2 ** 31 - 1

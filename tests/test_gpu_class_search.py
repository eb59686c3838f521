"""Patterns of character classes on the GPU: k_class_search (both stages), fmx_class_hit_offsets_dev, fmx_class_fold_status_dev,
the EXISTING packed calls over their result (fmx_locate_all_fill_dev, fmx_lines_of_hits_dev, fmx_query_lines_of_hits_dev), the
three host forms and their Python and C++ mirrors.

The judge is the oracle plus numpy (tests/test_class_search_cpu.py: Judged / class_judge — a class pattern's answer is the union
of the oracle's answers for the literal strings it spells; its ranges are the pairs fmx_locate_all_ranges_dev leaves for those
strings, ascending by start; lines by judge_lines and TermBatch.judge of the CPU tests), computed once per cap.  The batch holds
the corner cases, asserted on the judge's answer before the GPU runs.  Outputs are prefilled with a sentinel.  Options are set
inside the tests and put back in `finally`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_class_search_cpu import (BATCH_MAX_RANGES, RANGES_MAX, SMALL_MAX_RANGES, SR, ST_AIOOBE, ST_TOO_MANY, Judged, assert_corner_cases, check,
                                   class_judge, corner_batch, expected_arrays, pack_strings)
from test_gpu_locate_all import DevAll
from test_gpu_locate_rows import _torch, options
from test_match_lines_cpu import check_lines, judge_lines, judge_table
from test_match_query_cpu import ALL, ANY, NONE, TermBatch, Universe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = hdfs_text()
NL = ord("\n")
SENT = -0x3C3C3C3D
PAD = 64


def last_error():
    return (ia.lib.fmx_last_error() or b"").decode()


def ok(rc):
    assert rc == 0, last_error()


def literal_ranges_on(fm):
    """strings -> the {start, end} pairs fmx_locate_all_ranges_dev leaves in d_range_ws for them"""
    def ranges(strings):
        ch, off = pack_strings(strings)
        d = DevAll(fm, np.ascontiguousarray(ch), off, -1)
        d.torch.cuda.synchronize()
        return d.rng.cpu().numpy()[: 2 * len(strings)].reshape(len(strings), 2)
    return ranges


class DevClass:
    """the device form: both stages with the caller's allocation between them, every output prefilled with the sentinel"""

    def __init__(self, fm, patterns, max_ranges, ws_short=0, expect=0):
        torch = _torch()
        self.torch, self.fm = torch, fm
        alt, pos_off, pat_off = ia.pack_class_patterns(patterns)
        self.n = n = len(patterns)
        self.d_alt = torch.from_numpy(alt.view(np.int16)).cuda() if len(alt) else torch.zeros(1, dtype=torch.int16, device="cuda")
        self.d_pos, self.d_pat = torch.from_numpy(pos_off).cuda(), torch.from_numpy(pat_off).cuda()
        sent = lambda k, dt=torch.int32: torch.full((max(k, 1),), SENT, dtype=dt, device="cuda")  # noqa: E731
        self.range_off, self.counts, self.status = sent(n + 1, torch.int64), sent(n), sent(n)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        need = ia.lib.fmx_class_ranges_scratch_bytes(n)
        ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        self.max_ranges = max_ranges
        self.rc = ia.lib.fmx_class_ranges_count_dev(fm.handle, self.d_alt.data_ptr(), self.d_pos.data_ptr(), self.d_pat.data_ptr(), n, max_ranges,
                                                    self.range_off.data_ptr(), self.counts.data_ptr(), self.status.data_ptr(), ws.data_ptr(),
                                                    need - ws_short, self.stream)
        torch.cuda.synchronize()
        assert self.rc == expect, last_error()
        if self.rc:
            return
        self.m = int(self.range_off[n].item())  # (the caller's allocate-between-stages)
        self.ranges = sent(2 * self.m + PAD)
        ok(ia.lib.fmx_class_ranges_fill_dev(fm.handle, self.d_alt.data_ptr(), self.d_pos.data_ptr(), self.d_pat.data_ptr(), n, max_ranges,
                                            self.range_off.data_ptr(), self.ranges.data_ptr(), self.stream))
        torch.cuda.synchronize()

    def arrays(self):
        r = self.ranges.cpu().numpy()
        assert (r[2 * self.m:] == SENT).all()  # nothing stored behind the batch's ranges
        return self.range_off.cpu().numpy(), r[: 2 * self.m], self.counts.cpu().numpy()[: self.n], self.status.cpu().numpy()[: self.n]

    def hit_layout(self):
        torch = self.torch
        self.range_hit_off = torch.full((self.m + 1,), SENT, dtype=torch.int64, device="cuda")
        self.hit_off = torch.full((self.n + 1,), SENT, dtype=torch.int64, device="cuda")
        need = ia.lib.fmx_class_hit_offsets_scratch_bytes(self.m)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        ok(ia.lib.fmx_class_hit_offsets_dev(self.fm.handle, self.n, self.range_off.data_ptr(), self.ranges.data_ptr(), self.m,
                                            self.range_hit_off.data_ptr(), self.hit_off.data_ptr(), ws.data_ptr(), need, self.stream))
        torch.cuda.synchronize()
        self.total = int(self.hit_off[self.n].item())
        self.locs = torch.full((self.total + PAD,), SENT, dtype=torch.int32, device="cuda")
        self.range_status = torch.zeros(max(self.m, 1), dtype=torch.int32, device="cuda")

    def fill(self, first, hits):
        ok(ia.lib.fmx_locate_all_fill_dev(self.fm.handle, self.m, self.range_hit_off.data_ptr(), self.ranges.data_ptr(), first, hits,
                                          self.locs.data_ptr() + 4 * first, None, self.range_status.data_ptr(), self.stream))

    def fold(self):
        ok(ia.lib.fmx_class_fold_status_dev(self.fm.handle, self.n, self.range_off.data_ptr(), self.m, self.range_status.data_ptr(),
                                            self.status.data_ptr(), self.stream))
        self.torch.cuda.synchronize()


def judge_hits(o, judged, exp):
    """(packed hits, hit_off): every string's oracle locate() list, intact, in the order of the pattern's ranges"""
    lists, hit_off = [], [0]
    for j in judged:
        got = {}
        for s in j.strings:
            a = np.array(s, np.uint16)
            k = o.count(a)
            n, locs = o.locate(a, max_matches=-1, cap=k + 1)
            assert n == k
            got[s] = locs
        # the ranges' order: ascending by start — the strings ordered as the literal ranges are (exp[1] holds them sorted)
        order = sorted(j.strings, key=lambda s: j.start_of[s])
        mine = [got[s] for s in order]
        lists += mine
        hit_off.append(hit_off[-1] + sum(len(x) for x in mine))
    return np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32), np.array(hit_off, np.int64)


def expected_with_starts(judged, literal_ranges):
    """expected_arrays, and every Judged learns the start of each of its strings' ranges (judge_hits orders the lists by it)"""
    strings = [s for j in judged for s in j.strings]
    pairs = literal_ranges(strings) if strings else np.zeros((0, 2), np.int32)
    at = 0
    for j in judged:
        j.start_of = {s: int(pairs[at + i, 0]) for i, s in enumerate(j.strings)}
        at += len(j.strings)
    return expected_arrays(judged, lambda _strings: pairs)


class FakeUniverse(Universe):
    """a Universe (tests/test_match_query_cpu.py) whose 'patterns' are class patterns: TermBatch.judge only looks at the hits"""

    def __init__(self, judged, packed, hit_off):
        self.pats = [np.zeros(1, np.uint16) for _ in judged]
        self.hits = [packed[hit_off[i]:hit_off[i + 1]] for i in range(len(judged))]
        self.status = [j.status for j in judged]
        self.counts = [j.count for j in judged]


@pytest.fixture(scope="module")
def hd():
    t16 = ia.as_chars(HD)
    o = orc.OracleFmIndex(HD, SR, True)
    T = judge_table(o, NL)
    names, patterns = (list(x) for x in zip(*corner_batch()))
    judged = class_judge(("hd", BATCH_MAX_RANGES), o, patterns, BATCH_MAX_RANGES)
    assert_corner_cases(names, judged, o, t16)
    fm = ia.FmIndex(HD, SR, True, device=0)
    assert fm.build_line_table("\n") == 2000
    exp = expected_with_starts(judged, literal_ranges_on(fm))
    packed, hit_off = judge_hits(o, judged, exp)
    # the text level: for these words the oracle's hits ARE the text's (no quirk row among them), so Python may judge grep -i
    low = "".join(c.lower() if len(c.lower()) == 1 else c for c in HD)
    assert len(low) == len(HD)
    for word, n_occ, n_lines in (("block", 2662, 1919), ("namesystem", None, None)):
        i = names.index("icase " + word)
        at, pos = low.find(word), []
        while at >= 0:
            pos.append(at)
            at = low.find(word, at + 1)
        assert np.sort(packed[hit_off[i]:hit_off[i + 1]]).tolist() == pos
        lines = np.unique(np.searchsorted(T, pos, side="left"))
        assert n_occ is None or (len(pos) == n_occ and len(lines) == n_lines)
    yield dict(t16=t16, o=o, T=T, names=names, patterns=patterns, judged=judged, fm=fm, exp=exp, packed=packed, hit_off=hit_off, low=low)
    fm.close()


def test_both_stages_hit_offsets_fill_and_lines(hd):
    fm, patterns, exp, T = hd["fm"], hd["patterns"], hd["exp"], hd["T"]
    d = DevClass(fm, patterns, BATCH_MAX_RANGES)
    check(d.arrays(), exp, "device stages")
    # the all-singleton pattern: the literal's own count, range and hits
    i = hd["names"].index("singletons")
    ch, off = ia.pack_patterns(["NameSystem"])
    lit = DevAll(fm, np.ascontiguousarray(ch), off.astype(np.int32), -1)
    lit.fill(0, lit.total)
    llocs, lhit, lst, _ = lit.result()
    got = d.arrays()
    assert got[0][i + 1] - got[0][i] == 1 and (got[1][2 * got[0][i]:2 * got[0][i] + 2] == lit.rng.cpu().numpy()[:2]).all()
    assert got[2][i] == fm.count_batch(ch, off)[0][0] == lit.total and got[3][i] == lst[0] == 0
    # hit offsets, then the EXISTING fill over the m ranges in two windows
    d.hit_layout()
    assert (d.hit_off.cpu().numpy() == hd["hit_off"]).all() and d.total == len(hd["packed"])
    widths = exp[1][1::2] - exp[1][0::2]
    assert (np.diff(d.range_hit_off.cpu().numpy()) == widths).all()
    cut = d.total // 3 + 1
    d.fill(0, cut)
    d.fill(cut, d.total - cut)
    d.fold()
    locs = d.locs.cpu().numpy()
    assert (locs[: d.total] == hd["packed"]).all() and (locs[d.total:] == SENT).all()
    assert (locs[hd["hit_off"][i]:hd["hit_off"][i + 1]] == llocs[: lit.total]).all()
    assert (d.status.cpu().numpy()[: d.n] == exp[3]).all()  # (no walk of the fixture raises a status: the fold changes nothing)
    # ... and the existing line stages over (d_hit_off, d_locs), as for n literal patterns
    torch = d.torch
    for max_lines in (0, 5):
        want = judge_lines(T, hd["packed"], hd["hit_off"], max_lines)
        need = ia.lib.fmx_lines_of_hits_scratch_bytes(d.n, d.total)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        line_off = torch.full((d.n + 1,), SENT, dtype=torch.int64, device="cuda")
        lines = torch.full((d.total + PAD,), SENT, dtype=torch.int32, device="cuda")
        line_count = torch.full((d.n,), SENT, dtype=torch.int32, device="cuda")
        ok(ia.lib.fmx_lines_of_hits_dev(fm.handle, d.n, d.hit_off.data_ptr(), d.locs.data_ptr(), d.total, max_lines, line_off.data_ptr(),
                                        lines.data_ptr(), line_count.data_ptr(), ws.data_ptr(), need, d.stream))
        torch.cuda.synchronize()
        check_lines((lines.cpu().numpy(), line_off.cpu().numpy(), line_count.cpu().numpy()), want, "lines of class hits, max_lines %d" % max_lines,
                    tail=SENT)
    assert want[2][hd["names"].index("icase block")] == 1919


def queries_of(names):
    q = lambda *terms: [(names.index(t), k) for t, k in terms]  # noqa: E731
    return [q(("icase block", ALL), ("literal INFO", NONE)), q(("icase namesystem", ALL)), [],
            q(("icase warn", ANY), ("icase delet", ANY), ("blk", NONE)), q(("icase info", ALL), ("port", ALL), ("digit", ANY)),
            q(("three digits", ALL)), q(("no positions", ALL), ("icase info", ANY)), q(("icase info", NONE))]


def test_host_forms_python_and_cpp_mirrors(hd, tmp_path):
    fm, patterns, exp, T, names, judged = hd["fm"], hd["patterns"], hd["exp"], hd["T"], hd["names"], hd["judged"]
    packed3 = ia.pack_class_patterns(patterns)
    counts, status = fm.count_class_batch(*packed3, max_ranges=BATCH_MAX_RANGES)
    assert (counts == exp[2]).all() and (status == exp[3]).all()
    locs, hit_off, st = fm.locate_all_class_batch(*packed3, max_ranges=BATCH_MAX_RANGES)
    assert (hit_off == hd["hit_off"]).all() and (locs == hd["packed"]).all() and (st == exp[3]).all()
    # class terms mixed with ALL / ANY / NONE
    U = FakeUniverse(judged, hd["packed"], hd["hit_off"])
    queries = queries_of(names)
    b = TermBatch(U, queries)
    ids = [pid for qu in queries for pid, _ in qu]
    terms3 = ia.pack_class_patterns([patterns[i] for i in ids])
    for max_lines in (0, 7):
        want = b.judge(T, max_lines)
        lines, line_off, st, line_count, occ = fm.match_query_class_batch(*terms3, b.query_off, b.kinds, max_lines, want_counts=True,
                                                                          max_ranges=BATCH_MAX_RANGES)
        check_lines((np.concatenate([lines, [SENT]]).astype(np.int32), line_off, line_count), want, "class queries, max_lines %d" % max_lines, tail=SENT)
        assert (st == b.status).all() and (occ == b.counts).all()
    text_lines = HD.split("\n")[:2000]
    low_lines = hd["low"].split("\n")[:2000]  # (the text lowered unit by unit: the fixture has confirmed block and namesystem on it)
    not_info = [k for k, ln in enumerate(text_lines) if "block" in low_lines[k] and "INFO" not in ln]
    assert b.per_query(T)[0].tolist() == not_info and len(b.per_query(T)[5]) == 0 and ST_TOO_MANY in b.status.tolist()
    # q queries of ONE ALL term are the match_lines of class patterns
    one = TermBatch(U, [[(i, ALL)] for i in range(len(patterns))])
    lines, line_off, st, line_count, occ = fm.match_query_class_batch(*packed3, one.query_off, one.kinds, 0, want_counts=True,
                                                                      max_ranges=BATCH_MAX_RANGES)
    want = judge_lines(T, hd["packed"], hd["hit_off"], 0)
    check_lines((np.concatenate([lines, [SENT]]).astype(np.int32), line_off, line_count), want, "one ALL term per query", tail=SENT)
    # the keyword on the scalar calls
    assert fm.count("block", ignore_case=True) == 2662 and fm.count("block") == 1554 == fm.count("block", ignore_case=False)
    assert fm.count("namesystem") == 0 and fm.count("namesystem", ignore_case=True) == judged[names.index("icase namesystem")].count
    i = names.index("icase block")
    assert (fm.locate_all("block", ignore_case=True) == hd["packed"][hd["hit_off"][i]:hd["hit_off"][i + 1]]).all()
    with_block = [k for k, ln in enumerate(low_lines) if "block" in ln]
    assert len(with_block) == 1919 and fm.match_lines("BLOCK", ignore_case=True).tolist() == with_block
    assert fm.match_lines("BLOCK", 3, ignore_case=True).tolist() == with_block[:3]
    assert fm.match_query(all="Block", none="NAMESYSTEM", ignore_case=True).tolist() == [k for k in with_block if "namesystem" not in low_lines[k]]
    grep = fm.grep("namesystem", ignore_case=True)
    assert grep == [(k, text_lines[k]) for k, ln in enumerate(low_lines) if "namesystem" in ln] and len(grep) > 600 and fm.grep("namesystem") == []
    counts, status = fm.count_class_batch(*ia.pack_class_patterns([[]]))
    assert counts.tolist() == [0] and status.tolist() == [ST_AIOOBE]
    with pytest.raises(IndexError):
        ia.raise_for_status(status[0])
    # the C++ mirror: tests/cpp/test_class_search_mirror.cpp prints what countClass / locateAllClass / matchQueryClass return
    exe = str(tmp_path / "test_class_search_mirror")
    libdir = os.path.join(ROOT, "index4j_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_class_search_mirror.cpp"),
                           "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    mirror = [ia.ignore_case("block"), ia.ignore_case("namesystem"), ia.parse_classes(":500[0-9][0-9]"), ["b", "", "k"], ia.ignore_case("zzqqzz")]
    mj = class_judge(("hd mirror", 256), hd["o"], mirror, 256)
    mexp = expected_with_starts(mj, literal_ranges_on(fm))
    mpacked, mhit_off = judge_hits(hd["o"], mj, mexp)
    assert out["counts"] == mexp[2].tolist() and out["hit_offsets"] == mhit_off.tolist() and out.get("hits", []) == mpacked.tolist()
    qnames = ["icase block", "literal INFO", "icase namesystem", "icase warn", "icase delet"]
    qids = [names.index(x) for x in qnames]
    bq = TermBatch(U, [[(qids[0], ALL), (qids[1], NONE)], [(qids[2], ALL)], [(qids[3], ANY), (qids[4], ANY)], []])
    lines, line_off, line_count = bq.judge(T, 0)
    assert out["n_lines"] == [2000] and out["query_offsets"] == line_off.tolist() and out.get("query_lines", []) == lines.tolist()
    assert out["query_line_count"] == line_count.tolist() and out["query_occurrences"] == bq.counts.tolist()
    assert out["cut_offsets"] == bq.judge(T, 5)[1].tolist()


def test_the_cap_is_exact(hd):
    fm, o, names, patterns = hd["fm"], hd["o"], hd["names"], hd["patterns"]
    three, six = patterns[names.index("three digits")], patterns[names.index("six digits")]
    free = Judged(o, three, RANGES_MAX)
    S = max(free.frontier)
    assert free.status == 0 and 100 < S <= RANGES_MAX
    for cap, status in ((S, 0), (S - 1, ST_TOO_MANY)):
        batch = [ia.ignore_case("block"), three, ia.ignore_case("info")]
        judged = class_judge(("three gpu", cap), o, batch, cap)
        assert judged[1].status == status
        d = DevClass(fm, batch, cap)
        got = d.arrays()
        check(got, expected_arrays(judged, literal_ranges_on(fm)), "three digits under a cap of %d" % cap)
        if status:
            assert got[0][2] == got[0][1] and got[2][1] == 0  # no ranges, count 0
        counts, st = fm.count_class_batch(*ia.pack_class_patterns(batch), max_ranges=cap)
        assert st.tolist() == [0, status, 0] and counts[1] == judged[1].count
    wide = Judged(o, six, RANGES_MAX)
    assert wide.status == ST_TOO_MANY and len(wide.frontier) == 4 and wide.frontier[3] > RANGES_MAX >= wide.frontier[2]
    d = DevClass(fm, [six, ia.ignore_case("block")], RANGES_MAX)
    got = d.arrays()
    assert got[3].tolist() == [ST_TOO_MANY, 0] and got[2].tolist() == [0, 2662] and got[0].tolist() == [0, 0, 3]
    with pytest.raises(RuntimeError, match="max_ranges"):
        ia.raise_for_status(fm.count_class_batch(*ia.pack_class_patterns([six]), max_ranges=RANGES_MAX)[1][0])


def test_errors_and_edges(hd):
    fm, patterns = hd["fm"], hd["patterns"]
    E_ARG = ia._lib.E_ARG
    for cap in (0, RANGES_MAX + 1):  # FMX_E_ARG, nothing written
        d = DevClass(fm, patterns, cap, expect=E_ARG)
        assert (d.range_off.cpu().numpy() == SENT).all() and (d.counts.cpu().numpy() == SENT).all() and (d.status.cpu().numpy() == SENT).all()
    d = DevClass(fm, patterns, BATCH_MAX_RANGES, ws_short=1, expect=E_ARG)  # a workspace one byte short
    assert (d.range_off.cpu().numpy() == SENT).all() and (d.counts.cpu().numpy() == SENT).all()
    good = DevClass(fm, patterns, BATCH_MAX_RANGES)
    p = good.d_pos.data_ptr()
    assert ia.lib.fmx_class_ranges_fill_dev(fm.handle, good.d_alt.data_ptr(), p, good.d_pat.data_ptr(), good.n, 0, good.range_off.data_ptr(),
                                            good.ranges.data_ptr(), good.stream) == E_ARG
    good.hit_layout()
    assert ia.lib.fmx_class_hit_offsets_dev(fm.handle, good.n, good.range_off.data_ptr(), good.ranges.data_ptr(), good.m, good.range_hit_off.data_ptr(),
                                            good.hit_off.data_ptr(), p, ia.lib.fmx_class_hit_offsets_scratch_bytes(good.m) - 1, good.stream) == E_ARG
    # n == 0
    none = DevClass(fm, [], 16)
    assert none.range_off.cpu().numpy().tolist() == [0] and none.m == 0
    none.hit_layout()
    assert none.hit_off.cpu().numpy().tolist() == [0] and none.total == 0
    counts, status = fm.count_class_batch(*ia.pack_class_patterns([]))
    assert len(counts) == 0 and len(status) == 0
    locs, hit_off, st = fm.locate_all_class_batch(*ia.pack_class_patterns([]))
    assert len(locs) == 0 and hit_off.tolist() == [0]
    lines, line_off, st = fm.match_query_class_batch(*ia.pack_class_patterns([]), [0, 0, 0], [])
    assert len(lines) == 0 and line_off.tolist() == [0, 0, 0]
    # a batch without hits, and the host forms' argument checks on a resident handle
    locs, hit_off, st = fm.locate_all_class_batch(*ia.pack_class_patterns([ia.ignore_case("zzqq"), []]))
    assert len(locs) == 0 and hit_off.tolist() == [0, 0, 0] and st.tolist() == [0, ST_AIOOBE]
    lines, line_off, st = fm.match_query_class_batch(*ia.pack_class_patterns([ia.ignore_case("zzqq")]), [0, 1], [ALL])
    assert len(lines) == 0 and line_off.tolist() == [0, 0]
    for bad in (0, RANGES_MAX + 1):
        with pytest.raises(ia.FmxError):
            fm.count_class_batch(*ia.pack_class_patterns(patterns), max_ranges=bad)
    with pytest.raises(ia.FmxError):
        fm.match_query_class_batch(*ia.pack_class_patterns([ia.ignore_case("info")]), [0, 2], [ALL])  # query_off does not end at n
    bare = ia.FmIndex(HD[:5000], SR, True, device=0)
    try:
        with pytest.raises(ia.FmxError, match="fmx_line_table_build"):
            bare.match_query_class_batch(*ia.pack_class_patterns([ia.ignore_case("info")]), [0, 1], [ALL])
    finally:
        bare.close()


def test_launch_shapes_image_forms_and_repeatability(hd):
    fm, o, patterns, names = hd["fm"], hd["o"], hd["patterns"], hd["names"]
    ranges_of = literal_ranges_on(fm)
    small = expected_arrays(class_judge(("hd", SMALL_MAX_RANGES), o, patterns, SMALL_MAX_RANGES), ranges_of)
    first = DevClass(fm, patterns, SMALL_MAX_RANGES).arrays()
    check(first, small, "the small cap")
    again = DevClass(fm, patterns, SMALL_MAX_RANGES).arrays()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))  # two runs, identical bytes
    with options(block=1024):
        for cap, want in ((SMALL_MAX_RANGES, small), (BATCH_MAX_RANGES, hd["exp"])):
            got = DevClass(fm, patterns, cap).arrays()
            check(got, want, "block 1024, cap %d" % cap)
    # the grid loops: a workgroup per CU, three teams per workgroup (max_ranges 1,024), about 5,000 patterns
    big = class_judge(("hd", RANGES_MAX), o, patterns, RANGES_MAX)
    assert big[names.index("three digits")].status == 0 and big[names.index("six digits")].status == ST_TOO_MANY
    e = expected_arrays(big, ranges_of)
    reps = 5000 // len(patterns) + 1
    per = np.diff(e[0])
    tiled = (np.concatenate([[0], np.cumsum(np.tile(per, reps))]).astype(np.int64), np.tile(e[1], reps), np.tile(e[2], reps), np.tile(e[3], reps))
    n_cu = _torch().cuda.get_device_properties(0).multi_processor_count
    assert len(patterns) * reps > 3 * 3 * n_cu  # every workgroup's pattern loop runs several times
    with options(groups_per_cu=1):
        got = DevClass(fm, patterns * reps, RANGES_MAX).arrays()
        check(got, tiled, "groups_per_cu 1, %d patterns" % (len(patterns) * reps))
    with options(image_compact=1):
        cfm = ia.FmIndex(HD, SR, True, device=None)
        cfm.blob()  # flattened under the option
        cfm.to_device(0)
    try:
        for cap, want in ((SMALL_MAX_RANGES, small), (BATCH_MAX_RANGES, hd["exp"]), (RANGES_MAX, e)):
            got = DevClass(cfm, patterns, cap).arrays()
            check(got, want, "compact image, cap %d" % cap)
        counts, status = cfm.count_class_batch(*ia.pack_class_patterns(patterns), max_ranges=BATCH_MAX_RANGES)
        assert (counts == hd["exp"][2]).all() and (status == hd["exp"][3]).all()
    finally:
        cfm.close()

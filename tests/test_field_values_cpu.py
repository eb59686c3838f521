"""The values that follow a pattern, with counts (fmx_values_of_hits_dev, fmx_field_values_batch; grep -o | sort | uniq -c) on the
CPU: the functions the kernels of index4j_amd/csrc/fmx_hit_values.hip run — fm_val_window, fm_val_length over both forms of the stop
set, fm_val_same, fm_val_chunk_key, fm_val_lower_bound (index4j_amd/csrc/fmx_hit_values.hpp) — compiled for the host and driven by a
mirror of the stages (tests/values_hostsim.cpp, a stand-alone program: std::stable_sort for every sorting pass, running sums for the
scans), which is additionally built with -fsanitize=address,undefined and run as such.

The judge is the oracle plus Python/numpy (judge_values): the hits are expected_packed's (tests/test_locate_all_cpu.py), the windows
the oracle's extract over [s, e) (the judge of tests/test_extract_packed_cpu.py), the grouping a dict, the order `sorted` on tuples
of code units.  The GPU suite runs the kernels themselves (tests/test_gpu_field_values.py, which shares the helpers below)."""
import os
import subprocess

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from test_locate_all_cpu import expected_packed
from test_match_sequence_cpu import occurrences_in_text

HERE = os.path.dirname(os.path.abspath(__file__))
HD = hdfs_text()
SENT16 = 0xFFFE  # a noncharacter no test text holds

# (pattern, stop set, max_len, hits, values, the most frequent values): the fixture's numbers, computed from the text itself
NAMED = [
    ("blk_", " \n", 32, 2468, 2199, [("-8775602795571523802", 4)]),
    ("blk_", " \n", 8, 2468, 2199, []),
    ("\n", " ", 6, 2000, 4, [("081110", 965), ("081111", 885), ("081109", 149), ("", 1)]),
    ("INFO ", " \n:", 64, 1920, 356, [("dfs.FSNamesystem", 525), ("dfs.DataNode$PacketResponder", 480), ("dfs.DataNode$DataXceiver", 283)]),
    (" ", " \n", 16, 30094, 9127, [("", 2585), ("INFO", 1920), ("block", 1240)]),
    ("/10.", " \n:", 24, 1040, 200, []),
]
K_TEXT = "k=a k=a. k=a- k=a k=ab k=a."


class Judged:
    """the judge's answer for a batch: the packed arrays, the values of every pattern as [(tuple of code units, count)], and the
    runs of every pattern in the ORACLE's hit order"""

    def __init__(self, val_off, counts, text_off, chars, per, runs, starts, stops, rows, lengths):
        self.val_off, self.counts, self.text_off, self.chars, self.per, self.runs = val_off, counts, text_off, chars, per, runs
        self.starts, self.stops, self.rows, self.lengths = starts, stops, rows, lengths
        for a in (val_off, counts, text_off, chars):
            a.setflags(write=False)

    def strings(self, i):
        return [(np.array(v, np.uint16).tobytes().decode("utf-16-le", "surrogatepass"), c) for v, c in self.per[i]]


def judge_values(o, locs, hit_off, lens, stop, max_len):
    """by the definition: s = min(max(h + len, 0), textLength), e = min(s + max_len, textLength), the oracle's extract over [s, e)
    (every distinct window once), the value up to the first stop unit, a dict per pattern, sorted on tuples of code units"""
    text_len = o.getInputLength() - 1
    n = len(hit_off) - 1
    stop_units = np.unique(ia.as_chars(stop))
    which = np.repeat(np.arange(n), np.diff(hit_off))
    s = np.clip(locs.astype(np.int64) + np.asarray(lens, np.int64)[which], 0, text_len)
    e = np.minimum(s + max_len, text_len)
    uk, inv = np.unique((s << 32) | e, return_inverse=True)
    us, ue = (uk >> 32).astype(np.int32), (uk & 0xFFFFFFFF).astype(np.int32)
    if len(uk):
        rows, _, st = o.extract_batch(us, ue, max_len, 0, threads=16, fill=SENT16)
        assert (st == 0).all()
    else:
        rows = np.zeros((0, max_len), np.uint16)
    ulen = (ue - us).astype(np.int64)
    inside = np.arange(max_len)[None, :] < ulen[:, None]
    stops_at = np.isin(rows, stop_units) & inside
    vlen = np.where(stops_at.any(axis=1), stops_at.argmax(axis=1), ulen)
    values = [tuple(rows[i, :vlen[i]].tolist()) for i in range(len(uk))]
    ids = {}
    vid = np.array([ids.setdefault(v, len(ids)) for v in values], np.int64)[inv] if len(uk) else np.zeros(0, np.int64)
    by_id = sorted(ids, key=ids.get)
    per, runs = [], []
    for i in range(n):
        mine = vid[hit_off[i]:hit_off[i + 1]]
        u, c = np.unique(mine, return_counts=True)
        groups = {by_id[k]: int(m) for k, m in zip(u, c)}
        per.append([(v, groups[v]) for v in sorted(groups)])
        runs.append(int(len(mine) > 0) + int((mine[1:] != mine[:-1]).sum()))
    flat = [vc for p in per for vc in p]
    val_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    counts = np.array([c for _, c in flat], np.int32)
    text_off = np.concatenate([[0], np.cumsum([len(v) for v, _ in flat])]).astype(np.int64)
    chars = np.array([u for v, _ in flat for u in v], np.uint16)
    return Judged(val_off, counts, text_off, chars, per, runs, s.astype(np.int32), e.astype(np.int32), rows[inv] if len(uk) else rows, ulen[inv])


def check_values(got, want, what):
    """got = (chars, text_off, counts, val_off), each possibly longer than the answer: what lies behind must hold the sentinel"""
    chars, text_off, counts, val_off = got
    assert (val_off == want.val_off).all(), what + ": val_off"
    G = int(want.val_off[-1])
    assert (counts[:G] == want.counts).all(), "%s: counts differ at %r" % (what, np.flatnonzero(counts[:G] != want.counts)[:5])
    assert (text_off[:G + 1] == want.text_off).all(), what + ": text_off"
    T = int(want.text_off[-1])
    assert (chars[:T] == want.chars).all(), "%s: code units differ at %r" % (what, np.flatnonzero(chars[:T] != want.chars)[:5])


def assert_named(want, i, pattern, hits, values, top):
    """the fixture's numbers, on the JUDGE's answer"""
    got = want.strings(i)
    assert sum(c for _, c in got) == hits and len(got) == values, (pattern, sum(c for _, c in got), len(got))
    by_count = sorted(got, key=lambda vc: -vc[1])
    assert by_count[:len(top)] == top, (pattern, by_count[:4])
    assert [v for v, _ in got] == sorted(v for v, _ in got)  # (Python's string order agrees on this fixture: no surrogates)


_EXE = {}


def hostsim_exe(tmpdir, sanitize=False):
    if sanitize not in _EXE:
        exe = os.path.join(str(tmpdir), "values_hostsim" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter"] + flags + ["-o", exe, os.path.join(HERE, "values_hostsim.cpp")])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


@pytest.fixture(scope="module")
def simdir(tmp_path_factory):
    return tmp_path_factory.mktemp("values_hostsim")


def run_hostsim(simdir, want, locs, hit_off, lens, stop, max_len, text_len, extra_hits=0, form="bitmap", sanitize=False):
    """the stages' mirror over the judge's windows; (chars, text_off, counts, val_off), runs"""
    n, total = len(hit_off) - 1, int(hit_off[-1])
    n_hits = total + extra_hits
    stop = ia.as_chars(stop)
    win_off = np.concatenate([[0], np.cumsum(want.lengths), np.full(extra_hits, want.lengths.sum())]).astype(np.int64)
    keep = np.arange(max_len)[None, :] < want.lengths[:, None]
    win = want.rows[keep] if total else np.zeros(0, np.uint16)
    src, dst = os.path.join(str(simdir), "in.bin"), os.path.join(str(simdir), "out.bin")
    with open(src, "wb") as f:
        for a in (np.array([n, n_hits, len(stop), max_len, text_len], np.int64), np.asarray(lens, np.int32), stop, np.asarray(hit_off, np.int64),
                  np.concatenate([locs, np.full(extra_hits, -5, np.int32)]).astype(np.int32), win_off, win.astype(np.uint16)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([hostsim_exe(simdir, sanitize), src, dst] + (["list"] if form == "list" else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(dst, np.uint8)
    G, R, T = (int(x) for x in raw[:24].view(np.int64))
    at = 24

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += count * np.dtype(dtype).itemsize
        return out

    val_off, counts, text_off, chars = take(np.int64, n + 1), take(np.int32, G), take(np.int64, G + 1), take(np.uint16, T)
    start, stop_at = take(np.int32, n_hits), take(np.int32, n_hits)
    assert at == len(raw)
    assert (start[:total] == want.starts).all() and (stop_at[:total] == want.stops).all()
    assert (start[total:] == 0).all() and (stop_at[total:] == 0).all()
    return (chars, text_off, counts, val_off), R


def sim_case(simdir, o, key, patterns, stop, max_len, lens=None, **kw):
    ch, off = ia.pack_patterns(patterns)
    off = off.astype(np.int32)
    locs, hit_off, status, _, counts = expected_packed(key, o, ch, off, -1)
    lens = np.diff(off) if lens is None else lens
    want = judge_values(o, locs, hit_off, lens, stop, max_len)
    got, R = run_hostsim(simdir, want, locs, hit_off, lens, stop, max_len, o.getInputLength() - 1, **kw)
    assert R == sum(want.runs)
    check_values(got, want, "%s, stop %r, max_len %d" % (key, stop, max_len))
    return want, locs, hit_off


@pytest.fixture(scope="module")
def hd():
    return ia.as_chars(HD), orc.OracleFmIndex(HD, 16, True)


@pytest.mark.parametrize("form", ["bitmap", "list"])
def test_named_cases(simdir, hd, form):
    t16, o = hd
    more_runs = False
    for pattern, stop, max_len, hits, values, top in NAMED:
        want, locs, hit_off = sim_case(simdir, o, "hd16 values " + repr(pattern), [pattern], stop, max_len, form=form)
        assert (np.sort(locs) == occurrences_in_text(HD, pattern)).all()  # the oracle's hits are the text's occurrences
        assert_named(want, 0, pattern, hits, values, top)
        if max_len == 8:
            assert all(len(v) == 8 for v, _ in want.per[0])  # every value is cut at max_len
        if pattern == "blk_" and max_len == 32:
            assert max(len(v) for v, _ in want.per[0]) == 20
        if pattern == "/10.":
            more_runs = want.runs[0] > values  # non-contiguous runs: a value between two occurrences of its prefix
    ok = orc.OracleFmIndex(K_TEXT, 4, True)
    wk, _, _ = sim_case(simdir, ok, "k text", ["k="], " .", 8, form=form)
    assert wk.strings(0) == [("a", 4), ("a-", 1), ("ab", 1)]  # "a" is reached by two terminators; the prefix order a, a-, ab
    # runs alone are not the answer: the index orders its rows by ITS alphabet's codes, so which of the two texts shows a value
    # between two runs of its prefix is the index's business — one of them must
    assert more_runs or wk.runs[0] > 3


def test_synthetic_texts(simdir):
    # values that differ only in the 4th, 5th, 8th and 9th code unit: the edges of the sort's chunks
    base = "abcdefghij"
    variants = [base] + [base[:k] + c + base[k + 1:] for k in (3, 4, 7, 8) for c in ("A", "z")]
    text = "".join("v=%s;" % v for v in variants + variants[::-2]) + "v="
    o = orc.OracleFmIndex(text, 4, True)
    for max_len in (1, 9, 64):
        want, _, _ = sim_case(simdir, o, "chunk edges", ["v="], ";", max_len)
        got = want.strings(0)
        assert [v for v, _ in got] == sorted({v[:max_len] for v in variants} | {""})  # (the last occurrence ends at textLength: "")
        assert dict(got)[""] == 1
    # a value and the same value followed by U+0000, in a text that holds U+0000 and whose stop set does not
    text0 = "v=ab;v=ab\0;v=ab\0\0;v=ab;v=a;v=ab\0c;v=ab\0;"
    o0 = orc.OracleFmIndex(text0, 4, True)
    want, _, _ = sim_case(simdir, o0, "nul", ["v="], ";", 12)
    assert want.strings(0) == [("a", 1), ("ab", 2), ("ab\0", 2), ("ab\0\0", 1), ("ab\0c", 1)]
    # no stop set: every value is its window; 64 units with duplicates
    want, _, _ = sim_case(simdir, o0, "nul", ["v="], "", 3)
    assert all(len(v) == 3 for v, _ in want.per[0]) and sum(c for _, c in want.per[0]) == 7
    sim_case(simdir, o0, "nul", ["v="], ";" * 40 + "c" * 24, 12, form="list")
    # the caller's lengths: a pattern "longer" than the text is left (the window clamps to textLength: the empty value)
    want, _, _ = sim_case(simdir, o0, "nul", ["v="], ";", 12, lens=[2 ** 31 - 1])
    assert want.strings(0) == [("", 7)]


def test_random_batch_cut_from_the_fixture(simdir, hd):
    t16, o = hd
    rng = np.random.default_rng(41)
    pats = [t16[s:s + m] for s, m in zip(rng.integers(0, len(t16) - 9, 300), rng.integers(1, 8, 300))]
    pats += [ia.as_chars("blk_"), np.zeros(0, np.uint16), ia.as_chars("blk_"), ia.as_chars("zzzq#"), ia.as_chars("lk_")]
    for stop, max_len, extra, form in ((" \n", 12, 0, "bitmap"), (":./ \n", 5, 37, "list")):
        want, locs, hit_off = sim_case(simdir, o, "hd16 values random", pats, stop, max_len, extra_hits=extra, form=form)
        k = len(pats) - 5
        assert want.per[k] == want.per[k + 2] and (max_len != 12 or len(want.per[k]) == 2199) and want.per[k + 1] == [] and want.per[k + 3] == []
        assert want.per[k + 4] == want.per[k]  # two patterns that share their values: two separate answers
        assert int(hit_off[-1]) > 50_000


def test_sanitized_build(simdir, hd):
    """the stand-alone program once more under AddressSanitizer and UBSan (nothing loaded into python is run under a sanitizer)"""
    t16, o = hd
    sim_case(simdir, o, "hd16 values '/10.'", ["/10."], " \n:", 24, sanitize=True)
    sim_case(simdir, orc.OracleFmIndex(K_TEXT, 4, True), "k text", ["k="], " .", 8, extra_hits=5, form="list", sanitize=True)

"""Builds tests/cpp/test_field_pairs_mirror.cpp against include/index4j/FmIndex.hpp + libfmx.so and runs it: host mode on the CPU (the
shapes the mirror judges itself, the reference's exceptions, no answer without a device), gpu mode on the MI355X, where what
fieldValuePairs, numberStatsByPair and numberStatsByPairBatch print is held to judge_pairs (tests/test_field_pairs_cpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "HDFS_2k_multichar.log")
_EXE = {}


def exe(tmp_path_factory):
    if "exe" not in _EXE:
        out = str(tmp_path_factory.mktemp("field_pairs_mirror") / "test_field_pairs_mirror")
        libdir = os.path.join(ROOT, "index4j_amd")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", out, os.path.join(ROOT, "tests", "cpp", "test_field_pairs_mirror.cpp"),
                               "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        _EXE["exe"] = out
    return _EXE["exe"]


def test_cpp_field_pairs_host_side(tmp_path_factory):
    r = subprocess.run([exe(tmp_path_factory), "host", FIXTURE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_cpp_field_pairs_on_gpu(tmp_path_factory):
    import orc
    from common import hdfs_text
    from test_field_pairs_cpu import fixture_case
    from test_match_lines_cpu import judge_table

    r = subprocess.run([exe(tmp_path_factory), "gpu", FIXTURE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().split("\n")}
    o = orc.OracleFmIndex(hdfs_text(), 16, True)
    w, want = fixture_case(o, judge_table(o, "\n"), "size ", None, None)
    assert [tuple(x.split("|")) for x in out["pairs"]] == [v for v, _ in want.values()]
    assert [int(x) for x in out["pair_lines"]] == want.pair_lines.tolist() and [int(x) for x in out["pivot_lines"]] == want.pair_lines.tolist()
    assert [int(x) for x in out["count"]] == want.count.tolist() and [int(x) for x in out["min"]] == want.min.tolist()
    assert [int(x) for x in out["max"]] == want.max.tolist() and [int(x) for x in out["pct"]] == want.pct.ravel().tolist()
    assert [(int(hi) << 64) | int(lo) for lo, hi in zip(out["sum_lo"], out["sum_hi"])] == want.sums
    assert [int(x) for x in out["counters"]] == [int(want.no_key[0]), int(want.not_number[0]), int(want.overflow[0]), int(want.kept[0])]

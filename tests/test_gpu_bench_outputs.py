"""bench.py's plain run and --dump-outputs: the plain line carries the timed figures only (the oracle, roofline and secondary
legs run with --full), --steps is the number of timed steps, and the .npy files hold what the LAST timed step computed — here
recomputed by the oracle from the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--cache-dir", str(tmp_path / "cache")] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)


def test_bench_refuses_zero_steps(tmp_path):
    r = _bench(["--steps", "0"], tmp_path)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_counts_of_its_last_step(tmp_path):
    import index4j_amd as ia
    import orc
    from index4j_amd import workload

    out = tmp_path / "out"
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--text-log2", "20", "--patterns", "5000", "--batches", "2",
                "--dump-outputs", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["cpu_baseline"] is None and line["roofline"] is None and "secondary" not in line
    assert sorted(os.listdir(out)) == ["counts.npy"]
    got = np.load(out / "counts.npy")
    assert got.dtype == np.float64 and got.shape == (5000,)
    text = ia.synth_log(1 << 20, seed=42)
    pat, off, _ = workload.count_batch_patterns(text, 5000, 8, seed=workload.PATTERN_SEED + (3 - 1) % 2)
    want, status = orc.OracleFmIndex(text, 32, True).count_batch(pat, off)
    assert (status == 0).all() and (got == want).all()


@pytest.mark.gpu
def test_segments_run_dumps_counts_and_hits_of_its_last_step(tmp_path):
    import orc
    from index4j_amd import workload

    out = tmp_path / "out"
    r = _bench(["--gpus", "1", "--workload", "segments", "--segments", "2", "--segment-log2", "18", "--patterns-total", "3000",
                "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    counts, found, locs = (np.load(out / ("%s.npy" % k)) for k in ("counts", "found", "locations"))
    assert counts.shape == (3000,) and found.shape == (3000,) and locs.shape == (3000, 16)
    texts = workload.segment_texts(2, 18)
    pat, off = workload.segment_patterns(texts, 3000, 8)
    want = sum(orc.OracleFmIndex(t, 32, True).count_batch(pat, off)[0].astype(np.int64) for t in texts)
    assert (counts == want).all() and (found == np.minimum(want, 16)).all()
    live = np.arange(16)[None, :] < found[:, None]
    assert (locs[~live] == -1).all() and (locs[live] >= 0).all()

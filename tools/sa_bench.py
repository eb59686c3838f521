#!/usr/bin/env python3
"""SuffixArray on the 256 MiB log (2^28 chars of synth_log(42)): construction in HBM, count of 1,048,576 8-char
synth_patterns(43), locate of 100,000 patterns with max_matches = 16, and the reference-shaped locate(100) of 8-31-char
substrings — each with the default fence table and without one (option sa_fences = 0).  Kernel time by hipEvents around the
device-pointer calls (operands already in HBM); every result is checked: counts against FmIndex.count minus [the largest
suffix starts with p], the runs without fences against the runs with them, located rows against the host's copy of the array.
usage: python tools/sa_bench.py [--text-log2 28] [--reps 20] [--out sa_bench.json]  (the result line is printed either way)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    """median ms of fn() between two hipEvents on the current stream"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    import torch

    import index4j_amd as ia

    ia.SuffixArray("warm up", device=0).construct()
    text = ia.synth_log(1 << args.text_log2, seed=42)
    n = len(text)
    builds = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = ia.SuffixArray(text, device=0).construct()
        builds.append(time.perf_counter() - t0)
    sa = s.getSuffixArray()
    fm = ia.FmIndexBuilder().setSampleRate(32).setEnableExtraction(False).setBuildDevice(0).build(text, device=0)
    top = int(sa[n])

    def largest(pat, off):
        m = np.diff(off)
        if (m == m[0]).all() and m[0] <= n - top:
            return (pat.reshape(-1, int(m[0])) == text[top:top + int(m[0])]).all(axis=1).astype(np.int32)
        out = np.zeros(len(m), dtype=np.int32)
        for i in np.nonzero(m <= n - top)[0]:
            out[i] = int((pat[off[i]:off[i + 1]] == text[top:top + m[i]]).all())
        return out

    rng = np.random.default_rng(45)
    ref_starts = rng.integers(0, n - 32, 100)
    ref_lens = rng.integers(8, 32, 100)
    workloads = {
        "count_1M_8": ia.synth_patterns(text, 8, 1 << 20, seed=43)[:2] + (None,),
        "locate_100k_16": ia.synth_patterns(text, 8, 100000, seed=44)[:2] + (16,),
        "locate_ref_100": ia.pack_patterns([text[a:a + b] for a, b in zip(ref_starts, ref_lens)]) + (100,),
    }
    rows = {"text_chars": n, "build_s": min(builds)}
    results = {}
    for fences in (4096, 0):
        assert ia.lib.fmx_set_option(b"sa_fences", fences) == 0
        assert ia.lib.fmx_to_device(s._h, 0) == 0  # the fence table follows the option
        for name, (pat, off, mm) in workloads.items():
            k = len(off) - 1
            d_pat = torch.from_numpy(pat.view(np.int16)).cuda()
            d_off = torch.from_numpy(off).cuda()
            d_counts = torch.zeros(k, dtype=torch.int32, device="cuda")
            if mm is None:
                ms = timed(torch, lambda: s.count_batch_dev(d_pat, d_off, k, d_counts,
                                                            stream=torch.cuda.current_stream()), args.reps)
                got = (d_counts.cpu().numpy(),)
            else:
                d_locs = torch.full((k, mm), -1, dtype=torch.int32, device="cuda")
                d_found = torch.zeros(k, dtype=torch.int32, device="cuda")
                ms = timed(torch, lambda: s.locate_batch_dev(d_pat, d_off, k, mm, d_locs, d_found, d_counts,
                                                             stream=torch.cuda.current_stream()), args.reps)
                got = (d_counts.cpu().numpy(), d_found.cpu().numpy(), d_locs.cpu().numpy())
            if name in results:  # without fences: the same answers
                assert all((a == b).all() for a, b in zip(got, results[name])), name
            else:
                exp, st = fm.count_batch(pat, off)
                assert (st == 0).all() and (got[0] == exp - largest(pat, off)).all(), name
                if mm is not None:
                    assert (got[1] == np.minimum(got[0], mm)).all(), name
                results[name] = got
            rows["%s_ms%s" % (name, "" if fences else "_nofence")] = ms
    ia.lib.fmx_set_option(b"sa_fences", 4096)
    # rows are consecutive entries of the array: checked against the host copy for a sample
    inv = np.empty(n + 1, dtype=np.int64)
    inv[sa] = np.arange(n + 1)
    for name in ("locate_100k_16", "locate_ref_100"):
        counts, found, locs = results[name]
        for i in range(0, len(found), 13):
            f = int(found[i])
            if f:
                r = inv[locs[i, :f]]
                assert (r == r[0] + np.arange(f)).all(), (name, i)
    rows["queries_per_s_count"] = (1 << 20) / (rows["count_1M_8_ms"] / 1e3)
    print(json.dumps(rows))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

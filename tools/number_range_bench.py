#!/usr/bin/env python3
"""Query terms on the number behind a pattern — fmx_match_query_number_batch (the windows, the parse and the comparison on the
device; only the lines and the per-term counters come down) — against the composition it replaces, as a caller would run it on the
same library's other entry points, and against fmx_match_query_batch of the same term unranged: the same pipeline less the windows,
the parse and the compaction — the floor this stage can approach, not a target.  One index per process (the log text of bench.py,
2^--text-log2 characters, sampleRate 32, the default residency, its line table built): the index and the timing method of
tools/number_stats_bench.py.

"latency_ms=" and "blk_" (its digits where the id is not negative), each as ONE ALL term under a range that keeps every number
([0, 2^63 - 1]), one that keeps about 1 % (from the pattern's 99th percentile up: number_stats' p99) and one that keeps nothing
([3, 2]).  The composition: locate_all_batch + extract_packed_batch of the 32-unit windows + parsing (Horner over the columns of the
padded windows) + the comparison + line_bounds of every line / np.searchsorted (the line of each passing hit) + np.unique, with numpy
on one host core.  Both sides are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one
call; two untimed calls first, the routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the
slower route's min is above the faster route's max.  No speed-up is fixed in advance.  Before anything is timed the new form's lines
and counters are compared with what the composition computes.

EVERY LEG RUNS IN A PROCESS OF ITS OWN (tools/number_stats_bench.py showed the host's 2 GiB cache of device scratch blocks carrying
one leg's blocks into the next): without --leg this tool starts one child per leg, one after the other, and merges their records.
usage: python tools/number_range_bench.py [--text-log2 28] [--repeats 5] [--out profiles/number_range.json] [--leg PATTERN/RANGE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from number_stats_bench import WINDOW, parse_windows  # noqa: E402

NUMBER_MAX = 2 ** 63 - 1
PATTERNS = ("latency_ms=", "blk_")
RANGES = ("every", "percent", "nothing")


def run_leg(args, pattern, name):
    import index4j_amd as ia
    from index4j_amd import workload

    def timed(calls):
        for call in calls.values():
            call()
            call()
        times = {leg: [] for leg in calls}
        for _ in range(args.repeats):
            for leg, call in calls.items():
                t0 = time.perf_counter()
                call()
                times[leg].append((time.perf_counter() - t0) * 1e3)
        return {leg: {"ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for leg, t in times.items()}

    def compare(row, new, old):
        a, b = row[old], row[new]
        row["ratio_%s_over_%s" % (old, new)] = a["ms"] / b["ms"]
        row["%s_faster_than_%s_by_more_than_the_spread" % (new, old)] = bool(a["min_ms"] > b["max_ms"])
        row["%s_faster_than_%s_by_more_than_the_spread" % (old, new)] = bool(b["min_ms"] > a["max_ms"])

    text = workload.log_text(args.text_log2)
    text_len = len(ia.as_chars(text))
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = int(fm.build_line_table("\n"))
    ch, off = ia.pack_patterns([pattern])
    off = np.ascontiguousarray(off, dtype=np.int32)
    query_off, kinds = np.array([0, 1], np.int32), np.array([0], np.uint8)
    p99 = int(fm.number_stats(pattern, permille=(990,)).pct[0][0])
    lo, hi = {"every": (0, NUMBER_MAX), "percent": (p99, NUMBER_MAX), "nothing": (3, 2)}[name]

    def new():
        return fm.match_query_number_batch(ch, off, query_off, kinds, [lo], [hi], 0, 0, True)

    def floor():
        return fm.match_query_batch(ch, off, query_off, kinds, 0, True)

    def composition():
        locs, hit_off, _ = fm.locate_all_batch(ch, off, -1)
        s = np.minimum(locs.astype(np.int64) + len(pattern), text_len)
        chars, text_off, _ = fm.extract_packed_batch(s, np.minimum(s + WINDOW, text_len))
        ok, value = parse_windows(chars, text_off)
        passing = ok & (value >= np.uint64(lo)) & (value <= np.uint64(max(hi, 0))) if lo <= hi else np.zeros(len(locs), bool)
        start = fm.line_bounds(np.arange(n_lines, dtype=np.int32))[0]
        lines = np.unique(np.searchsorted(start, locs[passing], side="right") - 1).astype(np.int32)
        return lines, int(passing.sum()), int((~ok).sum())

    lines, line_off, status, line_count, occ, kept, nn, ov = new()
    c_lines, c_kept, c_nn = composition()
    f_lines = floor()[0]
    assert (lines == c_lines).all() and lines.shape == c_lines.shape and int(kept[0]) == c_kept and int(nn[0]) == c_nn and int(ov[0]) == 0
    assert int(status[0]) == 0 and int(line_count[0]) == len(lines) and len(lines) <= len(f_lines)
    if name == "every" and c_nn == 0:  # (every hit is a number: the unranged term's lines)
        assert (lines == f_lines).all()
    row = timed({"match_query_number": new, "match_query": floor, "composition": composition})
    hits = int(occ[0])
    row.update({"pattern": pattern, "range": [lo, hi], "hits": hits, "kept": c_kept, "kept_over_hits": c_kept / max(hits, 1), "not_number": c_nn,
                "lines": int(len(lines)), "lines_unranged": int(len(f_lines)), "bytes_down_match_query_number": int(len(lines)) * 4 + 16 + 6 * 4,
                "bytes_down_composition_at_most": hits * (4 + 2 * WINDOW) + n_lines * 8})
    compare(row, "match_query_number", "composition")
    compare(row, "match_query", "match_query_number")
    fm.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="one leg, as pattern/range: what a child process of this tool runs")
    args = ap.parse_args()
    assert args.repeats >= 5
    if args.leg:
        pattern, name = args.leg.rsplit("/", 1)
        print(json.dumps(run_leg(args, pattern, name)))
        return
    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "legs": {}}
    for pattern in PATTERNS:
        for name in RANGES:
            leg = "%s/%s" % (pattern, name)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--text-log2", str(args.text_log2), "--repeats", str(args.repeats), "--leg", leg],
                               capture_output=True, text=True, timeout=1200)
            if r.returncode != 0:
                print("[number_range_bench] %s failed (%d): %s" % (leg, r.returncode, r.stderr[-2000:]), file=sys.stderr, flush=True)
                sys.exit(1)  # (nothing more is started on the GPU after a failure)
            result["legs"][leg] = json.loads(r.stdout.strip().split("\n")[-1])
            print("[number_range_bench] %s: %s" % (leg, json.dumps(result["legs"][leg])), file=sys.stderr, flush=True)
            if args.out:  # (every leg that is done is on disk)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

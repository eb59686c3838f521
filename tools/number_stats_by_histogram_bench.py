#!/usr/bin/env python3
"""Statistics of the number behind a pattern by the value of a field of the same line, per bucket of lines —
fmx_number_stats_by_histogram_batch (one search, one filter, one grouping of the keys, the ranking by lines on the device; only the
top key rows and their cells come down) — against the composition it replaces, as a caller would run it on the same library's other
entry points: one number_stats_by_batch call per bucket with lines=(edges[b], edges[b + 1]) and a top-k over the merged groups on
the host; and against the FLOOR: one number_stats_by_batch over the whole window plus one number_stats_where_batch with the same
edges, the two calls whose work this one contains, without the join of rank and bucket.  One index (the log text of bench.py,
2^--text-log2 characters, sampleRate 32, the default residency, its line table built) and the timing method of
tools/number_stats_by_bench.py.  Every leg runs in a process of its own: without --leg the tool starts one child per leg, each of
which merges its result into --out.

Legs, each with --buckets buckets of equal width over all lines and --top key rows: "latency_ms=" by "status=" (few groups),
"latency_ms=" by "request id=" (about as many groups as lines that hold the number), and the first again under a filter that keeps
about 1 % (all = "status=503") and under one that keeps nothing (all = "terminating").  All sides are host-synchronous calls over
host arrays, so the clock is the host's (time.perf_counter) around one route; two untimed runs first, the routes ALTERNATED
--repeats times; median, min and max per route; a comparison holds when the slower route's min is above the faster route's max.  No
time is fixed in advance.  Before anything is timed the new form's key rows and cells are compared with what the composition
computes.
usage: python tools/number_stats_by_histogram_bench.py [--text-log2 28] [--buckets 60] [--top 10] [--repeats 5]
           [--out profiles/number_stats_by_histogram.json] [--leg LEG]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STOP, MAX_LEN, PERMILLE = " \t\r\n", 32, (500, 950)
LEGS = {"status/every": ("latency_ms=", "status=", None), "request_id/every": ("latency_ms=", "request id=", None),
        "status/percent": ("latency_ms=", "status=", dict(all=["status=503"])), "status/nothing": ("latency_ms=", "status=", dict(all=["terminating"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--buckets", type=int, default=60)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "number_stats_by_histogram.json"))
    ap.add_argument("--leg", default=None, help="this leg only, in this process; the result is merged into --out")
    args = ap.parse_args()
    assert args.repeats >= 5 and args.buckets >= 1 and args.top >= 1
    if args.leg is None:  # a fresh child process per leg
        for name in LEGS:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--text-log2", str(args.text_log2), "--buckets", str(args.buckets), "--top",
                            str(args.top), "--repeats", str(args.repeats), "--out", args.out, "--leg", name], check=True)
        with open(args.out) as f:
            print(json.dumps(json.load(f)))
        return
    import index4j_amd as ia
    from index4j_amd import workload

    result = {"text_log2": args.text_log2, "buckets": args.buckets, "top": args.top, "repeats": args.repeats, "sample_rate": 32, "stop": STOP,
              "max_len": MAX_LEN, "permille": PERMILLE, "legs": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        if all(old.get(k) == result[k] for k in ("text_log2", "buckets", "top")):
            result["legs"] = old.get("legs", {})

    def log(msg):
        print("[number_stats_by_histogram_bench] " + msg, file=sys.stderr, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)

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
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = int(fm.build_line_table("\n"))
    result["lines"] = n_lines
    B, top = args.buckets, args.top
    edges = np.linspace(0, n_lines, B + 1).astype(np.int32)
    number, key, query = LEGS[args.leg]
    nch, noff = ia.pack_patterns([number])
    kch, koff = ia.pack_patterns([key])
    terms = [t for word in ("all", "any", "none") for t in (query or {}).get(word, ())]
    kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in (query or {}).get(word, ())], np.uint8)
    tch, toff = ia.pack_patterns(terms)
    query_off, where_of = ([0, len(terms)], [0]) if query else ([0], [-1])

    def by(lines):
        return fm.number_stats_by_batch(kch, koff, nch, noff, [0], tch, toff, query_off, kinds, where_of, where_of, STOP, MAX_LEN, lines, PERMILLE, 0)

    def new():
        return fm.number_stats_by_histogram_batch(kch, koff, nch, noff, [0], tch, toff, query_off, kinds, where_of, where_of, STOP, MAX_LEN, edges, top,
                                                  PERMILLE, 0)

    def floor():
        return by((int(edges[0]), int(edges[-1]))), fm.number_stats_where_batch(nch, noff, tch, toff, query_off, kinds, where_of, edges, PERMILLE, 0)

    def composition():
        """a call per bucket, the groups merged by their text, the top keys by lines (ties in value order) picked on the host"""
        per, lines_of = [], {}
        for b in range(B):
            s = ia.NumberStatsBy(by((int(edges[b]), int(edges[b + 1]))))
            per.append(s)
            for g in s.groups:
                lines_of[g["value"]] = lines_of.get(g["value"], 0) + g["lines"]
        values = sorted(lines_of, key=lambda v: [ord(c) for c in v])
        rows = sorted(values, key=lambda v: -lines_of[v])[:top]
        cells = {v: [(0, 0)] * B for v in rows}
        other = [[0, 0] for _ in range(B)]
        for b, s in enumerate(per):
            for g in s.groups:
                if g["value"] in cells:
                    cells[g["value"]][b] = (g["count"], g["sum"])
                else:
                    other[b][0] += g["count"]
                    other[b][1] += g["sum"]
        tails = [sum(getattr(s, name) for s in per) for name in ("no_key", "not_number", "overflow", "kept")]
        return [(v, lines_of[v], [c for c, _ in cells[v]], [t for _, t in cells[v]]) for v in rows], other, tails, len(values)

    out = ia.NumberStatsByHistogram(new())
    c_rows, c_other, c_tails, c_groups = composition()
    assert [(r["value"], r["lines"], r["count"], r["sum"]) for r in out.rows] == [tuple(r) for r in c_rows]
    assert out.other["count"] == [c for c, _ in c_other] and out.other["sum"] == [t for _, t in c_other]
    # (a bucket's call sees a line's key only inside the bucket, which is where the line lies: the counters agree)
    assert [out.no_key, out.not_number, out.overflow, out.kept] == c_tails and out.n_groups == c_groups
    row = timed({"number_stats_by_histogram": new, "floor": floor, "composition": composition})
    row.update({"number": number, "key": key, "query": query, "hits": out.occurrences, "key_hits": out.key_occurrences, "kept": out.kept,
                "key_kept": out.key_kept, "groups": out.n_groups, "rows": len(out.rows), "no_key": out.no_key})
    compare(row, "number_stats_by_histogram", "composition")
    compare(row, "floor", "number_stats_by_histogram")
    result["legs"][args.leg] = row
    log("%s: %s" % (args.leg, json.dumps(row)))
    fm.close()


if __name__ == "__main__":
    main()

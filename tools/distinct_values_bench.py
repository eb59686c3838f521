#!/usr/bin/env python3
"""The distinct values of a field per bucket of lines, dc over time — fmx_distinct_values_histogram_where_batch (the filter, the
grouping, the two sorts and the counters on the device; n * B pairs of ints come down) — against (a) the composition it replaces:
one field_values_where_batch(lines=(edges[b], edges[b + 1])) per bucket with len() taken on the host, plus a host set of the values'
text for first_seen; and against (b) the FLOOR: field_values_histogram_where_batch of the same call with top = 1, which runs the same
filter and values stage and one sort over the kept hits, so the new call is expected to cost about one narrow sort more.  One index
(the log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default residency, its line table built) and the timing
method of tools/field_values_histogram_bench.py; --leg runs one leg, so that every leg can have a process of its own.

Legs (60 buckets of equal numbers of lines): "status=" (a handful of groups), "request id=" (about as many groups as hits), "blk_",
and "status=" under a filter that keeps about 1 % (all = "status=503") and one that keeps nothing (all = "terminating").  All sides
are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two untimed calls first,
the routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower route's min is above the
faster route's max.  No ratio is fixed in advance.  Before anything is timed the new form's distinct and first_seen of the leg are
compared with what the composition computes.
usage: python tools/distinct_values_bench.py [--text-log2 28] [--repeats 5] [--out profiles/distinct_values.json] [--leg LEG]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STOP, MAX_LEN, BUCKETS = " \t\r\n", 32, 60
LEGS = {"status": ("status=", None), "request_id": ("request id=", None), "blk": ("blk_", None),
        "status/percent": ("status=", dict(all=["status=503"])), "status/nothing": ("status=", dict(all=["terminating"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="this leg only (a process of its own); the result is merged into --out")
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "stop": STOP, "max_len": MAX_LEN, "buckets": BUCKETS, "legs": {}}
    if args.out and os.path.exists(args.out) and args.leg:
        with open(args.out) as f:
            old = json.load(f)
        if old.get("text_log2") == args.text_log2:
            result["legs"] = old.get("legs", {})

    def log(msg):
        print("[distinct_values_bench] " + msg, file=sys.stderr, flush=True)
        if args.out:  # (every leg that is done is on disk)
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
    edges = np.linspace(0, n_lines, BUCKETS + 1).astype(np.int32)
    for name, (pattern, query) in LEGS.items():
        if args.leg and args.leg != name:
            continue
        ch, off = ia.pack_patterns([pattern])
        terms = [t for word in ("all", "any", "none") for t in (query or {}).get(word, ())]
        kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in (query or {}).get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        query_off, where_of = ([0, len(terms)], [0]) if query else ([0], [-1])

        def new():
            return fm.distinct_values_histogram_where_batch(ch, off, tch, toff, query_off, kinds, where_of, edges, STOP, MAX_LEN)

        def floor():
            return fm.field_values_histogram_where_batch(ch, off, tch, toff, query_off, kinds, where_of, edges, 1, STOP, MAX_LEN)

        def composition():
            distinct, first_seen, seen = np.zeros(BUCKETS, np.int64), np.zeros(BUCKETS, np.int64), set()
            for b in range(BUCKETS):
                chars, text_off = fm.field_values_where_batch(ch, off, tch, toff, query_off, kinds, where_of, STOP, MAX_LEN, (int(edges[b]), int(edges[b + 1])))[:2]
                distinct[b] = len(text_off) - 1
                raw = chars.tobytes()
                here = {raw[2 * int(a):2 * int(e)] for a, e in zip(text_off[:-1], text_off[1:])}
                first_seen[b] = len(here - seen)
                seen |= here
            return distinct, first_seen

        out = new()
        c_distinct, c_first = composition()
        assert (out["distinct"][0] == c_distinct).all() and (out["first_seen"][0] == c_first).all() and (out["status"] == 0).all()
        assert int(out["first_seen"].sum()) == int(out["n_values"][0]) == floor()["n_values"][0]
        row = timed({"distinct_values": new, "floor": floor, "composition": composition})
        row.update({"pattern": pattern, "query": query, "hits": int(out["occurrences"][0]), "kept": int(out["kept"][0]), "groups": int(out["n_values"][0]),
                    "bytes_down_distinct_values": 2 * BUCKETS * 4})
        compare(row, "distinct_values", "composition")
        compare(row, "floor", "distinct_values")
        result["legs"][name] = row
        log("%s: %s" % (name, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

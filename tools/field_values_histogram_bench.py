#!/usr/bin/env python3
"""The top values of a field per bucket of lines, the stacked timeline — fmx_field_values_histogram_where_batch (the filter, the
grouping, the ranking and the binning on the device; only top * B counters and the text of top values come down) — against (a) the
host composition it replaces, as a caller would run it on the same library's other entry points, and against (b) the FLOOR:
field_values_where_batch plus hit_histogram_where_batch as two calls, the two answers this call joins, without the join.  One
index (the log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default residency, its line table built) and the timing
method of tools/number_stats_by_bench.py; --leg runs one leg, so that every leg can have a process of its own.

Legs (60 buckets of equal numbers of lines, top 10): "status=" (a handful of groups), "request id=" (about as many groups as hits:
the case the device-side top-k exists for), "blk_", and "status=" under a filter that keeps every hit (all = "status="), one that
keeps about 1 % (all = "status=503") and one that keeps nothing (all = "terminating").  The composition: field_values_where_batch (the groups and their counts: the ranking) + locate_all_batch (every
hit comes down) + match_query_batch and line_bounds for the filter + line_bounds of the edges and np.searchsorted (the bucket of
every hit) + extract_packed_batch of the window behind every kept hit + cutting and grouping with numpy on one host core (np.unique
over the padded values, np.bincount over rank * B + bucket).  Both sides are host-synchronous calls over host arrays, so the clock
is the host's (time.perf_counter) around one call; two untimed calls first, the routes ALTERNATED --repeats times; median, min and
max per route; a comparison holds when the slower route's min is above the faster route's max.  No speed-up is fixed in advance.
Before anything is timed the new form's rows and `other` of the leg are compared with what the composition computes.
usage: python tools/field_values_histogram_bench.py [--text-log2 28] [--repeats 5] [--out profiles/field_values_histogram.json] [--leg LEG] [--alone]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from field_values_bench import windows_of  # noqa: E402

STOP, MAX_LEN, TOP, BUCKETS = " \t\r\n", 32, 10, 60
LEGS = {"status": ("status=", None), "request_id": ("request id=", None), "blk": ("blk_", None),
        "status/every": ("status=", dict(all=["status="])), "status/percent": ("status=", dict(all=["status=503"])),
        "status/nothing": ("status=", dict(all=["terminating"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="this leg only (a process of its own); the result is merged into --out")
    ap.add_argument("--alone", action="store_true", help="the new form and the floor without the composition between their calls (recorded as LEG/alone)")
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "stop": STOP, "max_len": MAX_LEN, "top": TOP, "buckets": BUCKETS,
              "legs": {}}
    if args.out and os.path.exists(args.out) and args.leg:
        with open(args.out) as f:
            old = json.load(f)
        if old.get("text_log2") == args.text_log2:
            result["legs"] = old.get("legs", {})

    def log(msg):
        print("[field_values_histogram_bench] " + msg, file=sys.stderr, flush=True)
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
    text_len = len(ia.as_chars(text))
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = int(fm.build_line_table("\n"))
    result["lines"] = n_lines
    edges = np.linspace(0, n_lines, BUCKETS + 1).astype(np.int32)
    # where the lines of the edges start: the bucket of a hit is one np.searchsorted over them (the last edge is no line: the text's end)
    edge_start = np.concatenate([fm.line_bounds(edges[:-1])[0].astype(np.int64), [text_len + 1]])
    stop_units = ia.as_chars(STOP)
    for name, (pattern, query) in LEGS.items():
        if args.leg and args.leg != name:
            continue
        ch, off = ia.pack_patterns([pattern])
        lens = np.diff(np.asarray(off, np.int64))
        terms = [t for word in ("all", "any", "none") for t in (query or {}).get(word, ())]
        kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in (query or {}).get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        query_off, where_of = ([0, len(terms)], [0]) if query else ([0], [-1])

        def new():
            return fm.field_values_histogram_where_batch(ch, off, tch, toff, query_off, kinds, where_of, edges, TOP, STOP, MAX_LEN)

        def floor():
            v = fm.field_values_where_batch(ch, off, tch, toff, query_off, kinds, where_of, STOP, MAX_LEN, (int(edges[0]), int(edges[-1])))
            h = fm.hit_histogram_where_batch(ch, off, tch, toff, query_off, kinds, where_of, edges)
            return v, h

        def composition():
            _, _, counts, _ = fm.field_values_where_batch(ch, off, tch, toff, query_off, kinds, where_of, STOP, MAX_LEN, (int(edges[0]), int(edges[-1])))[:4]
            order = np.argsort(-counts.astype(np.int64), kind="stable")[:TOP]  # the ranking: the groups, by count, ties in value order
            locs, _, _ = fm.locate_all_batch(ch, off, -1)
            if query:
                lines, _, _ = fm.match_query_batch(tch, toff, query_off, kinds)
                if len(lines):
                    start, stop = fm.line_bounds(lines)[:2]
                    at = np.searchsorted(start, locs, side="right") - 1
                    locs = locs[(at >= 0) & (locs < stop[np.maximum(at, 0)])]
                else:
                    locs = locs[:0]
            bucket = np.searchsorted(edge_start, locs, side="right") - 1
            inside = (bucket >= 0) & (bucket < BUCKETS)
            locs, bucket = locs[inside], bucket[inside]
            hist, other = np.zeros((len(order), BUCKETS), np.int64), np.zeros(BUCKETS, np.int64)
            if len(locs) == 0:
                return order, counts[order], hist, other, 0
            s, e, _ = windows_of(locs, np.array([0, len(locs)], np.int64), lens, MAX_LEN, text_len)
            chars, text_off, _ = fm.extract_packed_batch(s, e)
            ln = np.diff(text_off)
            rows = np.zeros((len(locs), MAX_LEN + 1), ">u2")  # (big-endian rows: np.unique's order is then the order of the values)
            within = np.arange(MAX_LEN)[None, :] < ln[:, None]
            rows[:, :MAX_LEN][within] = chars
            stops_at = np.isin(rows[:, :MAX_LEN], stop_units) & within
            vlen = np.where(stops_at.any(axis=1), stops_at.argmax(axis=1), ln)
            rows[:, :MAX_LEN][np.arange(MAX_LEN)[None, :] >= vlen[:, None]] = 0
            rows[:, MAX_LEN] = vlen
            keys = np.ascontiguousarray(rows).view(np.dtype((np.void, rows.shape[1] * 2))).reshape(-1)
            _, group = np.unique(keys, return_inverse=True)
            group = group.reshape(-1)
            rank = np.full(len(counts), len(order), np.int64)
            rank[order] = np.arange(len(order))
            cells = np.bincount(rank[group] * BUCKETS + bucket, minlength=(len(order) + 1) * BUCKETS).reshape(len(order) + 1, BUCKETS)
            return order, counts[order], cells[:-1], cells[-1], len(locs)

        out = new()
        c_group, c_count, c_hist, c_other, c_kept = composition()
        assert (out["row_group"] == c_group).all() and (out["row_count"] == c_count).all() and (out["hist"] == c_hist).all()
        assert (out["other"][0] == c_other).all() and int(out["kept"][0]) == c_kept and (out["status"] == 0).all()
        if args.alone:  # (the composition brings every hit down between two calls of the new form: this run shows what that costs it)
            row = timed({"field_values_histogram": new, "floor": floor})
            compare(row, "floor", "field_values_histogram")
            result["legs"][name + "/alone"] = row
            log("%s, alone: %s" % (name, json.dumps(row)))
            continue
        row = timed({"field_values_histogram": new, "floor": floor, "composition": composition})
        row.update({"pattern": pattern, "query": query, "hits": int(out["occurrences"][0]), "kept": c_kept, "groups": int(out["n_values"][0]),
                    "rows": int(out["row_off"][1]),
                    "bytes_down_field_values_histogram": int(out["row_off"][1]) * (8 + BUCKETS * 4) + (int(out["row_off"][1]) + 1) * 8 + len(out["chars"]) * 2
                    + BUCKETS * 4})
        compare(row, "field_values_histogram", "composition")
        compare(row, "floor", "field_values_histogram")
        result["legs"][name] = row
        log("%s: %s" % (name, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Matching lines and hits per bucket of lines, the timeline of a log search — fmx_line_histogram_batch and
fmx_hit_histogram_where_batch (the binning on the device, only q x B or n x B counters come down) — against the compositions they
replace, as a caller would run them on the same library's other entry points.  One process, one index (the log text of bench.py,
2^--text-log2 characters, sampleRate 32, the default residency, its line table built): the index and the timing method of
tools/match_query_bench.py and tools/field_values_where_bench.py.  Edges: 60 and 1,440 buckets of equal line counts over the text.

(a) lines per bucket.  heavy: ONE query over the three most frequent strings (all, all, all); heavy_none: the same strings as
    (all, all, none), the heavy leg of tools/match_query_bench.py; uniform: that tool's queries of three 8-character patterns
    (any, any, none).  line_histogram_batch against match_query_batch (the lines
    of every query come down) followed by np.searchsorted of the edges in each query's lines on one host core.
(b) hits per bucket.  "blk_" under the three filters of tools/field_values_where_bench.py (nearly every hit kept, about 1 %,
    none).  hit_histogram_where_batch against locate_all_batch + match_query_batch + line_bounds / np.searchsorted (the hits inside
    the matching lines, and their lines) + np.add.at; for 60 buckets also against 60 calls of count_where(lines=(lo, hi)).
Both sides are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  No speed-up is fixed in advance.  Before anything is timed the new form's counters
of EVERY leg are compared with what the compositions compute.
usage: python tools/line_histogram_bench.py [--text-log2 28] [--repeats 5] [--out profiles/line_histogram.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from field_values_where_bench import FILTERS  # noqa: E402

ALL, ANY, NONE = 0, 1, 2
BUCKETS = (60, 1440)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=1 << 26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload
    from locate_all_bench import frequent_strings

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "lines_per_bucket": {}, "hits_per_bucket": {}}

    def log(msg):
        print("[line_histogram_bench] " + msg, file=sys.stderr, flush=True)
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
        row["%s_faster_by_more_than_the_spread" % new] = bool(a["min_ms"] > b["max_ms"])
        row["%s_faster_by_more_than_the_spread" % old] = bool(b["min_ms"] > a["max_ms"])

    text = workload.log_text(args.text_log2)
    t16 = ia.as_chars(text)
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = int(fm.build_line_table("\n"))
    result["lines"] = n_lines
    edges_of = {B: np.linspace(0, n_lines, B + 1).astype(np.int32) for B in BUCKETS}

    # ---- (a) lines per bucket ----
    def lines_leg(queries, B):
        """queries: lists of (pattern, kind)"""
        ch, off = ia.pack_patterns([p for qu in queries for p, _ in qu])
        off = np.ascontiguousarray(off, dtype=np.int32)
        kinds = np.array([k for qu in queries for _, k in qu], np.uint8)
        query_off = np.concatenate([[0], np.cumsum([len(qu) for qu in queries])]).astype(np.int32)
        n, q, edges = len(off) - 1, len(queries), edges_of[B]

        def new():
            return fm.line_histogram_batch(ch, off, query_off, kinds, edges, want_counts=True)

        def composition():
            lines, line_off, st, line_count, occ = fm.match_query_batch(ch, off, query_off, kinds, 0, want_counts=True)
            hist = np.empty((q, B), np.int32)
            for Q in range(q):
                hist[Q] = np.diff(np.searchsorted(lines[line_off[Q]:line_off[Q + 1]], edges, side="left"))
            return hist, line_count, occ

        hist, st, line_count, occ = new()
        c_hist, c_line_count, c_occ = composition()
        assert (hist == c_hist).all() and (line_count == c_line_count).all() and (occ == c_occ).all() and (hist.sum(axis=1) == line_count).all()
        row = timed({"line_histogram": new, "composition": composition})
        total = int(line_count.astype(np.int64).sum())
        row.update({"terms": n, "queries": q, "buckets": B, "hits": int(occ.astype(np.int64).sum()), "lines_of_queries": total,
                    "bytes_down_line_histogram": q * B * 4 + q * 4 + 2 * n * 4,
                    "bytes_down_composition": total * 4 + (q + 1) * 8 + q * 4 + 2 * n * 4})
        compare(row, "line_histogram", "composition")
        return row

    strings, counts = frequent_strings(t16, fm, ia)
    order = np.argsort(-np.array(counts), kind="stable")
    strings, counts = [strings[i] for i in order], [counts[i] for i in order]
    result["strings"] = [{"string": ia.chars_to_str(s), "count": c} for s, c in zip(strings, counts)]
    heavy = [[(strings[0], ALL), (strings[1], ALL), (strings[2], ALL)]]
    heavy_none = [[(strings[0], ALL), (strings[1], ALL), (strings[2], NONE)]]  # (tools/match_query_bench.py's heavy leg)
    cpat, coff, _ = workload.count_batch_patterns(text, 100_000, 8)
    all_counts, _ = fm.count_batch(cpat, coff)
    cum = np.cumsum(all_counts.astype(np.int64))
    k = int(np.searchsorted(cum, max(args.max_hits, 1), side="right")) // 3 * 3
    assert k >= 3
    pats = [cpat[coff[i]:coff[i + 1]] for i in range(k)]
    triples = [[(pats[i], ANY), (pats[i + 1], ANY), (pats[i + 2], NONE)] for i in range(0, k, 3)]
    for name, queries in (("heavy", heavy), ("heavy_none", heavy_none), ("uniform", triples)):
        for B in BUCKETS:
            row = lines_leg(queries, B)
            result["lines_per_bucket"]["%s_%d" % (name, B)] = row
            log("lines, %s, %d buckets: %s" % (name, B, json.dumps(row)))

    # ---- (b) hits per bucket ----
    PATTERN = "blk_"
    ch, off = ia.pack_patterns([PATTERN])
    off = np.ascontiguousarray(off, dtype=np.int32)
    for name, query in FILTERS.items():
        terms = [t for word in ("all", "any", "none") for t in query.get(word, ())]
        kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in query.get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        toff = np.ascontiguousarray(toff, dtype=np.int32)
        query_off = np.array([0, len(terms)], np.int32)
        for B in BUCKETS:
            edges = edges_of[B]

            def new():
                return fm.hit_histogram_where_batch(ch, off, tch, toff, query_off, kinds, [0], edges, want_counts=True)

            def composition():
                lines, line_off, _ = fm.match_query_batch(tch, toff, query_off, kinds)
                locs, hit_off, _ = fm.locate_all_batch(ch, off, -1)
                hist = np.zeros(B, np.int32)
                if len(lines):
                    start, stop = fm.line_bounds(lines)[:2]
                    at = np.searchsorted(start, locs, side="right") - 1  # the last matching line that starts at or in front of the hit
                    keep = (at >= 0) & (locs < stop[np.maximum(at, 0)])  # (the pattern never starts on a boundary)
                    b = np.searchsorted(edges, lines[at[keep]], side="right") - 1
                    np.add.at(hist, b[(b >= 0) & (b < B)], 1)
                    return hist, int(keep.sum()), int(hit_off[-1]), len(lines)
                return hist, 0, int(hit_off[-1]), 0

            def per_bucket():
                return np.array([fm.count_where(PATTERN, where=query, lines=(int(lo), int(hi))) for lo, hi in zip(edges[:-1], edges[1:])], np.int32)

            hist, st, occ, kept, tst = new()
            c_hist, c_kept, hits, matching = composition()
            assert (hist[0] == c_hist).all() and int(kept[0]) == c_kept == int(hist.sum()) and int(occ[0]) == hits and (st == 0).all() and (tst == 0).all()
            calls = {"hit_histogram_where": new, "composition": composition}
            if B == 60:
                assert (per_bucket() == hist[0]).all()
                calls["count_where_per_bucket"] = per_bucket
            row = timed(calls)
            row.update({"query": query, "buckets": B, "hits": hits, "kept": c_kept, "kept_over_hits": c_kept / max(hits, 1), "matching_lines": matching,
                        "bytes_down_hit_histogram_where": B * 4 + 3 * 4 + len(terms) * 4,
                        "bytes_down_composition": matching * 4 + 8 + hits * 4 + 2 * 8 + matching * 8})
            compare(row, "hit_histogram_where", "composition")
            if B == 60:
                compare(row, "hit_histogram_where", "count_where_per_bucket")
            result["hits_per_bucket"]["%s_%d" % (name, B)] = row
            log("hits, %s, %d buckets: %s" % (name, B, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

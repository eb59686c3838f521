#!/usr/bin/env python3
"""Statistics of the number behind a pattern, per bucket of lines — fmx_number_stats_where_batch (the parse, the order and the
reduction on the device; only n x B rows come down) — against the composition it replaces, as a caller would run it on the same
library's other entry points, and against fmx_hit_histogram_where_batch on the same call: the same pipeline less the windows, the
value sorts and the reduction — the floor this stage can approach, not a target.  One process, one index (the log text of
bench.py, 2^--text-log2 characters, sampleRate 32, the default residency, its line table built): the index and the timing method
of tools/line_histogram_bench.py.  Edges: 60 buckets of equal line counts over the text; permille 500 and 950.

"blk_" (its digits where the id is not negative) under the three filters of tools/field_values_where_bench.py, and "latency_ms="
under a filter that keeps every hit (all = the pattern itself), one that keeps about 1 % (all = "status=503") and one that keeps
nothing (all = "terminating").  The composition: locate_all_batch + match_query_batch + line_bounds / np.searchsorted (the hits
inside the matching lines, and their lines) + extract_packed_batch of the 32-unit windows + parsing (Horner over the columns of the
padded windows) and grouping (np.lexsort, np.add.reduceat over the values' halves, the percentiles by index) with numpy on one
host core.  Both sides are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one
call; two untimed calls first, the routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the
slower route's min is above the faster route's max.  No speed-up is fixed in advance.  Before anything is timed the new form's
rows of EVERY leg are compared with what the composition computes, and the invariant with the hits histogram's rows.
usage: python tools/number_stats_bench.py [--text-log2 28] [--repeats 5] [--out profiles/number_stats.json] [--pattern PATTERN] [--only LEG]"""
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

WINDOW, BUCKETS, PERMILLE = 32, 60, (500, 950)
LEGS = {"blk_": FILTERS,
        "latency_ms=": {"every": dict(all=["latency_ms="]), "percent": dict(all=["status=503"]), "nothing": dict(all=["terminating"])}}


def parse_windows(chars, text_off):
    """(ok, value) of packed windows: the run of digits at each window's start as uint64 (runs of up to 19 digits below 2^63: what
    these legs hold — the comparison with the device's rows would show anything else)"""
    k = len(text_off) - 1
    lens = np.diff(text_off)
    pad = np.zeros((k, WINDOW), np.uint16)
    cols = np.arange(WINDOW)[None, :]
    inside = cols < lens[:, None]
    pad[inside] = chars
    digit = inside & (pad >= 48) & (pad <= 57)
    run = np.where(digit.all(axis=1), WINDOW, (~digit).argmax(axis=1))
    value = np.zeros(k, np.uint64)
    for j in range(int(run.max()) if k else 0):
        on = run > j
        value[on] = value[on] * np.uint64(10) + (pad[on, j] - 48).astype(np.uint64)
    return run > 0, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pattern", default=None, help="the legs of this pattern only, in a process of their own")
    ap.add_argument("--only", default=None, help="one leg, as pattern/filter (a profiler's run): the new form alone, --repeats times")
    args = ap.parse_args()
    assert args.repeats >= 5 or args.only
    import index4j_amd as ia
    from index4j_amd import workload

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "buckets": BUCKETS, "permille": PERMILLE, "legs": {}}

    def log(msg):
        print("[number_stats_bench] " + msg, file=sys.stderr, flush=True)
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
    B, P = BUCKETS, len(PERMILLE)
    for pattern, filters in LEGS.items():
        if args.pattern and args.pattern != pattern:
            continue
        ch, off = ia.pack_patterns([pattern])
        off = np.ascontiguousarray(off, dtype=np.int32)
        for name, query in filters.items():
            if args.only and args.only != "%s/%s" % (pattern, name):
                continue
            terms = [t for word in ("all", "any", "none") for t in query.get(word, ())]
            kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in query.get(word, ())], np.uint8)
            tch, toff = ia.pack_patterns(terms)
            toff = np.ascontiguousarray(toff, dtype=np.int32)
            query_off = np.array([0, len(terms)], np.int32)

            def new():
                return fm.number_stats_where_batch(ch, off, tch, toff, query_off, kinds, [0], edges, PERMILLE, 0)

            def floor():
                return fm.hit_histogram_where_batch(ch, off, tch, toff, query_off, kinds, [0], edges, want_counts=True)

            def composition():
                lines, line_off, _ = fm.match_query_batch(tch, toff, query_off, kinds)
                locs, hit_off, _ = fm.locate_all_batch(ch, off, -1)
                count, nn = np.zeros(B, np.int32), 0
                sums, vmin, vmax, pct = [0] * B, np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros((B, P), np.int64)
                if len(lines) == 0:
                    return count, sums, vmin, vmax, pct, nn, 0
                start, stop = fm.line_bounds(lines)[:2]
                at = np.searchsorted(start, locs, side="right") - 1  # the last matching line that starts at or in front of the hit
                keep = (at >= 0) & (locs < stop[np.maximum(at, 0)])  # (the pattern never starts on a boundary)
                kept = locs[keep]
                b = np.searchsorted(edges, lines[at[keep]], side="right") - 1
                s = np.minimum(kept.astype(np.int64) + len(pattern), text_len)
                chars, text_off, _ = fm.extract_packed_batch(s, np.minimum(s + WINDOW, text_len))
                ok, value = parse_windows(chars, text_off)
                in_bucket = (b >= 0) & (b < B)
                nn = int((in_bucket & ~ok).sum())
                use = in_bucket & ok
                b, value = b[use], value[use]
                order = np.lexsort((value, b))
                b, value = b[order], value[order]
                first = np.searchsorted(b, np.arange(B + 1), side="left")
                count[:] = np.diff(first)
                full = np.flatnonzero(count)
                if len(full):
                    lo = np.add.reduceat(value & np.uint64(0xffffffff), first[full])
                    hi = np.add.reduceat(value >> np.uint64(32), first[full])
                    for k, bk in enumerate(full):
                        sums[bk] = (int(hi[k]) << 32) + int(lo[k])
                    vmin[full], vmax[full] = value[first[full]].astype(np.int64), value[first[full + 1] - 1].astype(np.int64)
                    for j, pm in enumerate(PERMILLE):
                        c = count[full].astype(np.int64)
                        pct[full, j] = value[first[full] + np.maximum(1, -(-pm * c // 1000)) - 1].astype(np.int64)
                return count, sums, vmin, vmax, pct, nn, int(keep.sum())

            if args.only:
                for _ in range(args.repeats):
                    new()
                continue
            out = new()
            hist, _, occ, kept, _ = floor()
            c_count, c_sums, c_min, c_max, c_pct, c_nn, c_kept = composition()
            sums = [(int(h) << 64) | int(lo) for lo, h in zip(out["sum_lo"][0], out["sum_hi"][0])]
            assert (out["count"][0] == c_count).all() and sums == c_sums and (out["min"][0] == c_min).all() and (out["max"][0] == c_max).all()
            assert (out["pct"][0] == c_pct).all() and int(out["not_number"][0]) == c_nn and int(out["overflow"][0]) == 0
            assert int(out["kept"][0]) == c_kept == int(kept[0]) and (out["status"] == 0).all() and (out["term_status"] == 0).all()
            assert int(out["count"][0].sum()) + c_nn == int(hist[0].sum())  # the invariant
            row = timed({"number_stats": new, "hit_histogram_where": floor, "composition": composition})
            hits = int(occ[0])
            row.update({"query": query, "hits": hits, "kept": c_kept, "kept_over_hits": c_kept / max(hits, 1), "parsed": int(c_count.sum()),
                        "not_number": c_nn, "sum_bits": max(sums).bit_length(),
                        "bytes_down_number_stats": B * (4 + 8 * 4 + 8 * P) + 5 * 4 + len(terms) * 4})
            compare(row, "number_stats", "composition")
            compare(row, "hit_histogram_where", "number_stats")
            result["legs"]["%s/%s" % (pattern, name)] = row
            log("%s, %s: %s" % (pattern, name, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

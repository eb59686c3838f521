#!/usr/bin/env python3
"""The lines ranked by the number behind a pattern — fmx_top_lines_where_batch (the parse, the candidate of every line and the
ranking on the device; only `top` rows come down) — against (a) the composition it replaces, as a caller would run it on the same
library's other entry points, and against (b) fmx_number_stats_where_batch of the same call without edges: the same windows, extract
and parse and two sorts of its own — the floor this stage can approach, not a target.  One process PER LEG (--leg), one index (the
log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default residency, its line table built): the index and the
timing method of tools/number_stats_bench.py.  top = 10, largest first.

The legs: "blk_" (its digits where the id is not negative) and "latency_ms=" without a filter, "latency_ms=" under a filter that
keeps about 1 % (all = "status=503") and under one that keeps nothing (all = "terminating").  The composition: locate_all_batch +
match_query_batch + line_bounds / np.searchsorted (the hits inside the matching lines, and their lines; without a filter the starts
of ALL lines, fetched once outside the clock) + extract_packed_batch of the 32-unit windows + parsing (Horner over the columns of
the padded windows) + np.lexsort twice (the candidate of every line, then the ranking) with numpy on one host core.  Both sides are
host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two untimed calls first,
the routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower route's min is above the
faster route's max; --alone times the new form and the floor once more without the composition between their calls.  No speed-up
is fixed in advance.  Before anything is timed the new form's rows are compared with what the
composition computes, and its counters with the number statistics'.
usage: python tools/top_lines_bench.py [--text-log2 28] [--repeats 5] [--out profiles/top_lines.json] [--leg LEG] [--alone] [--only LEG]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from number_stats_bench import WINDOW, parse_windows  # noqa: E402

TOP = 10
LEGS = {"blk_/every": ("blk_", None), "latency_ms=/every": ("latency_ms=", None), "latency_ms=/percent": ("latency_ms=", dict(all=["status=503"])),
        "latency_ms=/nothing": ("latency_ms=", dict(all=["terminating"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="a JSON file; with --leg the leg is merged into what the file holds")
    ap.add_argument("--leg", default=None, help="one leg (%s), in a process of its own" % ", ".join(LEGS))
    ap.add_argument("--alone", action="store_true", help="time the new form and the floor without the composition between their calls")
    ap.add_argument("--only", default=None, help="one leg (a profiler's run): the new form alone, --repeats times")
    args = ap.parse_args()
    assert args.repeats >= 5 or args.only
    import index4j_amd as ia
    from index4j_amd import workload

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "top": TOP, "legs": {}}
    if args.out and args.leg and os.path.exists(args.out):
        with open(args.out) as f:
            result["legs"] = json.load(f).get("legs", {})

    def log(msg):
        print("[top_lines_bench] " + msg, file=sys.stderr, flush=True)
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
    all_starts = None
    for leg, (pattern, query) in LEGS.items():
        if (args.leg and args.leg != leg) or (args.only and args.only != leg):
            continue
        ch, off = ia.pack_patterns([pattern])
        off = np.ascontiguousarray(off, dtype=np.int32)
        query = query or {}
        terms = [t for word in ("all", "any", "none") for t in query.get(word, ())]
        kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in query.get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        toff = np.ascontiguousarray(toff, dtype=np.int32)
        query_off, where_of = (np.array([0, len(terms)], np.int32), [0]) if terms else (np.array([0], np.int32), [-1])
        if not terms and all_starts is None:  # (a caller would keep them: outside the clock)
            all_starts = np.concatenate([fm.line_bounds(np.arange(a, min(a + (1 << 22), n_lines), dtype=np.int32))[0]
                                         for a in range(0, n_lines, 1 << 22)])

        def new():
            return fm.top_lines_where_batch(ch, off, tch, toff, query_off, kinds, where_of, [1], TOP, 0, None, 0)

        def floor():
            return fm.number_stats_where_batch(ch, off, tch, toff, query_off, kinds, where_of, None, (), 0)

        def composition():
            locs, hit_off, _ = fm.locate_all_batch(ch, off, -1)
            none = (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32), 0, 0, 0, 0)
            if terms:
                lines, line_off, _ = fm.match_query_batch(tch, toff, query_off, kinds)
                if len(lines) == 0:
                    return none
                start, stop = fm.line_bounds(lines)[:2]
                at = np.searchsorted(start, locs, side="right") - 1  # the last matching line that starts at or in front of the hit
                keep = (at >= 0) & (locs < stop[np.maximum(at, 0)])  # (the pattern never starts on a boundary)
                kept, line = locs[keep], lines[at[keep]]
            else:
                kept, line = locs, (np.searchsorted(all_starts, locs, side="right") - 1).astype(np.int32)
            if len(kept) == 0:
                return none
            s = np.minimum(kept.astype(np.int64) + len(pattern), text_len)
            chars, text_off, _ = fm.extract_packed_batch(s, np.minimum(s + WINDOW, text_len))
            ok, value = parse_windows(chars, text_off)
            kept_n, nn = len(kept), int((~ok).sum())
            kept, line, value = kept[ok], line[ok], value[ok]
            u = np.uint64(2 ** 63 - 1) - value  # largest first
            order = np.lexsort((kept, u, line))  # by line, the best value first, equal values by position
            kept, line, u = kept[order], line[order], u[order]
            head = np.flatnonzero(np.concatenate([[True], line[1:] != line[:-1]])) if len(line) else np.zeros(0, np.int64)
            rank = head[np.lexsort((line[head], u[head]))][:TOP]
            return line[rank], (np.uint64(2 ** 63 - 1) - u[rank]).astype(np.int64), kept[rank], len(head), int(ok.sum()), kept_n, nn

        if args.only:
            for _ in range(args.repeats):
                new()
            continue
        out = new()
        stats = floor()
        comp = composition()
        r = int(out["rows"][0])
        assert r == len(comp[0]) and (out["row_line"][0, :r] == comp[0]).all() and (out["row_value"][0, :r] == comp[1]).all()
        assert (out["row_loc"][0, :r] == comp[2]).all() and int(out["lines"][0]) == comp[3] and int(out["numbers"][0]) == comp[4]
        assert int(out["kept"][0]) == comp[5] == int(stats["kept"][0]) and (out["status"] == 0).all() and (out["term_status"] == 0).all()
        assert int(out["numbers"][0]) == int(stats["count"][0, 0]) and int(out["not_number"][0]) == int(stats["not_number"][0])
        assert int(out["overflow"][0]) == int(stats["overflow"][0]) and (r == 0 or int(out["row_value"][0, 0]) == int(stats["max"][0, 0]))
        if args.alone:  # (beside what the leg's full run has left in the file)
            alone = timed({"top_lines": new, "number_stats": floor})
            compare(alone, "number_stats", "top_lines")
            result["legs"].setdefault(leg, {})["alone"] = alone
            log("%s, alone: %s" % (leg, json.dumps(alone)))
            continue
        row = timed({"top_lines": new, "number_stats": floor, "composition": composition})
        row.update({"query": query, "hits": int(out["occurrences"][0]), "kept": comp[5], "kept_over_hits": comp[5] / max(int(out["occurrences"][0]), 1),
                    "numbers": comp[4], "lines": comp[3], "rows": r, "bytes_down_top_lines": TOP * 16 + 8 * 4 + len(terms) * 4})
        compare(row, "top_lines", "composition")
        compare(row, "number_stats", "top_lines")
        result["legs"][leg] = row
        log("%s: %s" % (leg, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

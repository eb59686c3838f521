#!/usr/bin/env python3
"""Field values only within the lines of a query (grep terminating | grep -o 'blk_[^ ]*' | sort | uniq -c) —
fmx_field_values_where_batch (the lines of the query, the filter of the hits and the grouping on the device, only the GROUPS come
down) — against the composition it replaces, as a caller would run it on the same library's other entry points: match_query_batch
(the lines come down), locate_all_batch (every hit of the value pattern comes down), line_bounds of the matching lines and
np.searchsorted to keep the hits inside them, extract_packed_batch of the window behind every kept hit, then the grouping with numpy
on one host core (tools/field_values_bench.py: host_group).  One process, one index (the log text of bench.py, 2^--text-log2
characters, sampleRate 32, the default residency, its line table built): the index and the timing method of
tools/field_values_bench.py.

The workload is ONE frequent value pattern ("blk_", stop set " \\t\\r\\n", max_len 32) under three filters:
  most     any of INFO / WARN / ERROR / DEBUG: keeps nearly every hit
  percent  all of "terminating" and "ERROR": keeps about 1 % of the hits
  nothing  all of "terminating", none of "PacketResponder": the terms have hits by the million, no line is left
Both routes are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the two routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  No speed-up is fixed in advance.  Before anything is timed the new form's values,
offsets, counts and kept hits of EVERY filter are compared with what the composition computes.
usage: python tools/field_values_where_bench.py [--text-log2 28] [--repeats 5] [--out profiles/field_values_where.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from field_values_bench import host_group, windows_of  # noqa: E402

FILTERS = {
    "most": dict(any=["INFO", "WARN", "ERROR", "DEBUG"]),
    "percent": dict(all=["terminating", "ERROR"]),
    "nothing": dict(all=["terminating"], none=["PacketResponder"]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload

    PATTERN, STOP, MAX_LEN = "blk_", " \t\r\n", 32
    stop16 = ia.as_chars(STOP)
    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "pattern": PATTERN, "stop": STOP, "max_len": MAX_LEN,
              "filters": {}}

    def log(msg):
        print("[field_values_where_bench] " + msg, file=sys.stderr, flush=True)
        if args.out:  # (every filter that is done is on disk)
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

    text = workload.log_text(args.text_log2)
    text_len = len(text)
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    result["lines"] = int(fm.build_line_table("\n"))
    ch, off = ia.pack_patterns([PATTERN])
    off = np.ascontiguousarray(off, dtype=np.int32)
    lens = np.diff(off)

    for name, query in FILTERS.items():
        terms = [t for word in ("all", "any", "none") for t in query.get(word, ())]
        kinds = np.array([k for k, word in enumerate(("all", "any", "none")) for _ in query.get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        toff = np.ascontiguousarray(toff, dtype=np.int32)
        query_off = np.array([0, len(terms)], np.int32)

        def new():
            return fm.field_values_where_batch(ch, off, tch, toff, query_off, kinds, [0], STOP, MAX_LEN)

        def composition(parts=None):
            t0 = time.perf_counter()
            lines, line_off, _ = fm.match_query_batch(tch, toff, query_off, kinds)
            t1 = time.perf_counter()
            locs, hit_off, _ = fm.locate_all_batch(ch, off, -1)
            t2 = time.perf_counter()
            if len(lines):
                start, stop = fm.line_bounds(lines)[:2]
                at = np.searchsorted(start, locs, side="right") - 1  # the last matching line that starts at or in front of the hit
                keep = (at >= 0) & (locs < stop[np.maximum(at, 0)])  # (the pattern never starts on a boundary)
            else:
                keep = np.zeros(len(locs), bool)
            kept = locs[keep]
            kept_off = np.array([0, len(kept)], np.int64)
            t3 = time.perf_counter()
            s, e, which = windows_of(kept, kept_off, lens, MAX_LEN, text_len)
            chars, text_off, st = fm.extract_packed_batch(s, e)
            t4 = time.perf_counter()
            out = host_group(which, 1, chars, text_off, stop16, MAX_LEN)
            if parts is not None:
                parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (time.perf_counter() - t4) * 1e3))
            return out + (int(hit_off[-1]), len(kept), len(lines), int(text_off[-1]))

        chars, text_off, counts, val_off, st, occ, kept, tst = new()
        c_chars, c_off, c_counts, c_val_off, runs, hits, c_kept, n_lines, units = composition()
        assert (val_off == c_val_off).all() and (counts == c_counts).all() and (text_off == c_off).all() and (chars == c_chars).all()
        assert int(occ[0]) == hits and int(kept[0]) == c_kept == int(counts.astype(np.int64).sum()) and (st == 0).all() and (tst == 0).all()
        parts = []
        row = timed({"field_values_where": new, "composition": lambda: composition(parts)})
        a, b = row["composition"], row["field_values_where"]
        groups = int(val_off[-1])
        last = np.array(parts[-args.repeats:])
        row.update({"query": query, "hits": hits, "kept": c_kept, "kept_over_hits": c_kept / max(hits, 1), "matching_lines": n_lines,
                    "groups": groups,
                    "composition_parts_ms": {"match_query": float(np.median(last[:, 0])), "locate_all": float(np.median(last[:, 1])),
                                             "line_bounds_and_searchsorted": float(np.median(last[:, 2])),
                                             "extract_packed": float(np.median(last[:, 3])), "numpy_grouping": float(np.median(last[:, 4]))},
                    "bytes_down_field_values_where": groups * 4 + (groups + 1) * 8 + int(text_off[-1]) * 2 + 2 * 8 + 3 * 4 + len(terms) * 4,
                    "bytes_down_composition": n_lines * 4 + n_lines * 8 + hits * 4 + units * 2 + (c_kept + 1) * 8 + c_kept * 4,
                    "ratio_composition_over_field_values_where": a["ms"] / b["ms"],
                    "field_values_where_faster_by_more_than_the_spread": bool(a["min_ms"] > b["max_ms"]),
                    "composition_faster_by_more_than_the_spread": bool(b["min_ms"] > a["max_ms"])})
        result["filters"][name] = row
        log("%s: %s" % (name, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

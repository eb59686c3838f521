#!/usr/bin/env python3
"""Statistics of the number behind a pattern, grouped by the value of a field of the same line — fmx_number_stats_by_batch (the
join through the line, the grouping, the parse and the reduction on the device; only the groups and their rows come down) —
against the composition it replaces, as a caller would run it on the same library's other entry points, and against the FLOOR:
field_values_where_batch of the key pattern plus number_stats_where_batch of the number pattern with one bucket, the two stages
this call contains, without the join.  One index (the log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default
residency, its line table built) and the timing method of tools/number_stats_bench.py; --leg runs one leg, so that every leg can
have a process of its own.

Legs: "latency_ms=" by "status=" (few groups), "latency_ms=" by "request id=" (about as many groups as lines that hold the
number), and the first leg again under a filter that keeps about 1 % (all = "status=503") and under one that keeps nothing
(all = "terminating").  The composition: match_query_batch (the lines that hold the key pattern and pass the filter) + line_bounds
+ locate_all_batch of both patterns + np.searchsorted (the line of every hit, the first key hit of every line) +
extract_packed_batch of the key windows and of the 32-unit number windows + cutting, parsing and grouping with numpy on one host
core (np.unique over the padded keys, np.lexsort, np.add.reduceat).  Both sides are host-synchronous calls over host arrays, so the
clock is the host's (time.perf_counter) around one call; two untimed calls first, the routes ALTERNATED --repeats times; median,
min and max per route; a comparison holds when the slower route's min is above the faster route's max.  No speed-up is fixed in
advance.  Before anything is timed the new form's groups and rows of the leg are compared with what the composition computes.
usage: python tools/number_stats_by_bench.py [--text-log2 28] [--repeats 5] [--out profiles/number_stats_by.json] [--leg LEG] [--alone]"""
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

STOP, MAX_LEN, PERMILLE = " \t\r\n", 32, (500, 950)
LEGS = {"status/every": ("latency_ms=", "status=", None), "request_id/every": ("latency_ms=", "request id=", None),
        "status/percent": ("latency_ms=", "status=", dict(all=["status=503"])), "status/nothing": ("latency_ms=", "status=", dict(all=["terminating"]))}


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

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "stop": STOP, "max_len": MAX_LEN, "permille": PERMILLE, "legs": {}}
    if args.out and os.path.exists(args.out) and args.leg:
        with open(args.out) as f:
            old = json.load(f)
        if old.get("text_log2") == args.text_log2:
            result["legs"] = old.get("legs", {})

    def log(msg):
        print("[number_stats_by_bench] " + msg, file=sys.stderr, flush=True)
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
    result["lines"] = int(fm.build_line_table("\n"))
    stop_units = ia.as_chars(STOP)
    for name, (number, key, query) in LEGS.items():
        if args.leg and args.leg != name:
            continue
        nch, noff = ia.pack_patterns([number])
        kch, koff = ia.pack_patterns([key])
        terms = [t for word in ("all", "any", "none") for t in (query or {}).get(word, ())]
        kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in (query or {}).get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        query_off, where_of = ([0, len(terms)], [0]) if query else ([0], [-1])
        # the composition's own query: the lines that hold the key pattern and pass the filter
        cterms = [key] + terms
        cch, coff = ia.pack_patterns(cterms)
        ckinds = np.concatenate([np.zeros(1, np.uint8), kinds])

        def new():
            return fm.number_stats_by_batch(kch, koff, nch, noff, [0], tch, toff, query_off, kinds, where_of, where_of, STOP, MAX_LEN, None, PERMILLE, 0)

        def floor():
            v = fm.field_values_where_batch(kch, koff, tch, toff, query_off, kinds, where_of, STOP, MAX_LEN)
            s = fm.number_stats_where_batch(nch, noff, tch, toff, query_off, kinds, where_of, None, PERMILLE, 0)
            return v, s

        def composition():
            lines, _, _ = fm.match_query_batch(cch, coff, [0, len(cterms)], ckinds)  # the lines that have a key
            klocs, _, _ = fm.locate_all_batch(kch, koff, -1)
            nlocs, _, _ = fm.locate_all_batch(nch, noff, -1)
            if query:  # the number hits pass the filter on their own
                flines, _, _ = fm.match_query_batch(tch, toff, query_off, kinds)
                fstart, fstop = fm.line_bounds(flines)[:2] if len(flines) else (np.zeros(0, np.int32), np.zeros(0, np.int32))
                at = np.searchsorted(fstart, nlocs, side="right") - 1
                nlocs = nlocs[(at >= 0) & (nlocs < fstop[np.maximum(at, 0)])] if len(flines) else nlocs[:0]
            kept = len(nlocs)
            if len(lines) == 0:
                return [], np.zeros(0, np.int64), np.zeros(0, np.int64), [], kept, 0, kept
            start, stop = fm.line_bounds(lines)[:2]
            klocs = np.sort(klocs)
            at = np.searchsorted(start, klocs, side="right") - 1
            on = (at >= 0) & (klocs < stop[np.maximum(at, 0)])
            _, first = np.unique(at[on], return_index=True)  # the first key hit of every line that has one (they all do)
            firsts = klocs[on][first]
            s = np.minimum(firsts.astype(np.int64) + len(key), text_len)
            chars, text_off, _ = fm.extract_packed_batch(s, np.minimum(s + MAX_LEN, text_len))
            lens = np.diff(text_off)
            pad = np.zeros((len(firsts), MAX_LEN), np.uint16)
            inside = np.arange(MAX_LEN)[None, :] < lens[:, None]
            pad[inside] = chars
            stops = np.isin(pad, stop_units) & inside
            vlen = np.where(stops.any(axis=1), stops.argmax(axis=1), lens)
            pad[np.arange(MAX_LEN)[None, :] >= vlen[:, None]] = 0
            keyed = np.concatenate([pad, vlen[:, None].astype(np.uint16)], axis=1)
            uniq, group_of_line, n_lines = np.unique(keyed, axis=0, return_inverse=True, return_counts=True)
            group_of_line = group_of_line.reshape(-1)
            values = ["".join(map(chr, u[:u[-1]])) for u in uniq]
            G = len(values)
            # the numbers: the line of every hit, its group, its value
            at = np.searchsorted(start, nlocs, side="right") - 1
            has = (at >= 0) & (nlocs < stop[np.maximum(at, 0)])
            no_key = int((~has).sum())
            s = np.minimum(nlocs[has].astype(np.int64) + len(number), text_len)
            chars, text_off, _ = fm.extract_packed_batch(s, np.minimum(s + WINDOW, text_len))
            ok, value = parse_windows(chars, text_off)
            g = group_of_line[at[has]][ok]
            value = value[ok]
            order = np.lexsort((value, g))
            g, value = g[order], value[order]
            edge = np.searchsorted(g, np.arange(G + 1), side="left")
            count = np.diff(edge)
            sums = [0] * G
            full = np.flatnonzero(count)
            if len(full):
                lo = np.add.reduceat(value & np.uint64(0xffffffff), edge[full])
                hi = np.add.reduceat(value >> np.uint64(32), edge[full])
                for k, gk in enumerate(full):
                    sums[gk] = (int(hi[k]) << 32) + int(lo[k])
            return values, n_lines, count, sums, no_key, int((~ok).sum()), kept

        out = ia.NumberStatsBy(new())
        c_values, c_lines, c_count, c_sums, c_no_key, c_nn, c_kept = composition()
        order = sorted(range(len(c_values)), key=lambda k: [ord(c) for c in c_values[k]])  # (np.unique's order pads with 0)
        assert [g["value"] for g in out.groups] == [c_values[k] for k in order] and [g["lines"] for g in out.groups] == [int(c_lines[k]) for k in order]
        assert [g["count"] for g in out.groups] == [int(c_count[k]) for k in order] and [g["sum"] for g in out.groups] == [c_sums[k] for k in order]
        assert (out.no_key, out.not_number, out.overflow, out.kept) == (c_no_key, c_nn, 0, c_kept)
        if args.alone:  # (the composition brings every hit down between two calls of the new form: this run shows what that costs it)
            row = timed({"number_stats_by": new, "floor": floor})
            compare(row, "floor", "number_stats_by")
            result["legs"][name + "/alone"] = row
            log("%s, alone: %s" % (name, json.dumps(row)))
            continue
        row = timed({"number_stats_by": new, "floor": floor, "composition": composition})
        row.update({"number": number, "key": key, "query": query, "hits": out.occurrences, "key_hits": out.key_occurrences, "kept": out.kept,
                    "key_kept": out.key_kept, "groups": len(out.groups), "no_key": out.no_key})
        compare(row, "number_stats_by", "composition")
        compare(row, "floor", "number_stats_by")
        result["legs"][name] = row
        log("%s: %s" % (name, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

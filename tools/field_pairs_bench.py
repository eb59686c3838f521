#!/usr/bin/env python3
"""Statistics and line counts by the values of two fields of the same line — fmx_number_stats_by_pair_batch (the two first-hit lists
joined through the line on the device; only the groups, the pairs and their rows come down) — against the composition it replaces,
as a caller would run it on the same library's other entry points, and against the FLOOR: number_stats_by_batch of the same call by
the a-key alone, which is the same stages without the join.  One index (the log text of bench.py, 2^--text-log2 characters,
sampleRate 32, the default residency, its line table built) and the timing method of tools/number_stats_by_bench.py; --leg runs one
leg, so that every leg can have a process of its own.

Legs: "latency_ms=" by ("status=", "user=") (few pairs), "latency_ms=" by ("status=", "request id=") (as many pairs as lines), the
first leg again under a filter that keeps about 1 % (all = "status=503") and under one that keeps nothing (all = "terminating"), and
the pivot alone: ("status=", "user=") without a number pattern (n == 0; its floor is number_stats_by_batch by "status=" of a number
pattern that has no hit: the keys' stages alone).  The composition: per key pattern match_query_batch (the lines that hold it and
pass the filter) + line_bounds + locate_all_batch + np.searchsorted (the line of every hit, the first key hit of every line) +
extract_packed_batch of the key windows, np.unique over the padded keys; np.intersect1d of the two line lists and np.unique over the
pairs; then locate_all_batch of the number pattern, extract_packed_batch of its 32-unit windows, parsing and grouping with numpy
on one host core (np.lexsort, np.add.reduceat).  Both sides are host-synchronous calls over host arrays, so the clock is the host's
(time.perf_counter) around one call; two untimed calls first, the routes ALTERNATED --repeats times; median, min and max per route;
a comparison holds when the slower route's min is above the faster route's max.  No figure is fixed in advance.  Before anything is
timed the new form's pairs and rows of the leg are compared with what the composition computes.
usage: python tools/field_pairs_bench.py [--text-log2 28] [--repeats 5] [--out profiles/field_pairs.json] [--leg LEG]"""
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
LEGS = {"status_user/every": ("latency_ms=", "status=", "user=", None), "status_request_id/every": ("latency_ms=", "status=", "request id=", None),
        "status_user/percent": ("latency_ms=", "status=", "user=", dict(all=["status=503"])),
        "status_user/nothing": ("latency_ms=", "status=", "user=", dict(all=["terminating"])), "status_user/pivot": (None, "status=", "user=", None)}
ABSENT = "zzqq#latency"  # the number pattern of the pivot's floor: no hit


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

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "stop": STOP, "max_len": MAX_LEN, "permille": PERMILLE, "legs": {}}
    if args.out and os.path.exists(args.out) and args.leg:
        with open(args.out) as f:
            old = json.load(f)
        if old.get("text_log2") == args.text_log2:
            result["legs"] = old.get("legs", {})

    def log(msg):
        print("[field_pairs_bench] " + msg, file=sys.stderr, flush=True)
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
    for name, (number, key_a, key_b, query) in LEGS.items():
        if args.leg and args.leg != name:
            continue
        numbers = [number] if number else []
        nch, noff = ia.pack_patterns(numbers)
        kch, koff = ia.pack_patterns([key_a, key_b])
        terms = [t for word in ("all", "any", "none") for t in (query or {}).get(word, ())]
        kinds = np.array([kk for kk, word in enumerate(("all", "any", "none")) for _ in (query or {}).get(word, ())], np.uint8)
        tch, toff = ia.pack_patterns(terms)
        query_off, w = ([0, len(terms)], 0) if query else ([0], -1)
        fch, foff = ia.pack_patterns([number or ABSENT])  # the floor: the same call by the a-key alone
        ach, aoff = ia.pack_patterns([key_a])

        def new():
            return fm.number_stats_by_pair_batch(kch, koff, nch, noff, [0] * len(numbers), [0], [1], tch, toff, query_off, kinds, [w, w], [w] * len(numbers), STOP,
                                                 MAX_LEN, None, PERMILLE, 0)

        def floor():
            return fm.number_stats_by_batch(ach, aoff, fch, foff, [0], tch, toff, query_off, kinds, [w], [w], STOP, MAX_LEN, None, PERMILLE, 0)

        def key_lines(key):
            """the lines that hold `key` and pass the filter, ascending, the group of each by its first hit's value, the values"""
            cterms = [key] + terms
            cch, coff = ia.pack_patterns(cterms)
            lines, _, _ = fm.match_query_batch(cch, coff, [0, len(cterms)], np.concatenate([np.zeros(1, np.uint8), kinds]))
            if len(lines) == 0:
                return lines, np.zeros(0, np.int64), []
            klocs, _, _ = fm.locate_all_batch(*ia.pack_patterns([key]), -1)
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
            uniq, group_of_line = np.unique(keyed, axis=0, return_inverse=True)
            values = ["".join(map(chr, u[:u[-1]])) for u in uniq]
            order = sorted(range(len(values)), key=lambda k: [ord(ch) for ch in values[k]])  # (np.unique's order pads with 0)
            rank = np.empty(len(values), np.int64)
            rank[order] = np.arange(len(values))
            return lines, rank[group_of_line.reshape(-1)], [values[k] for k in order]

        def composition():
            la, ga, va = key_lines(key_a)
            lb, gb, vb = key_lines(key_b)
            both, ia_, ib_ = np.intersect1d(la, lb, assume_unique=True, return_indices=True)
            key = ga[ia_] * max(len(vb), 1) + gb[ib_]
            uniq, pair_of_line, pair_lines = np.unique(key, return_inverse=True, return_counts=True)
            pairs = [(va[k // max(len(vb), 1)], vb[k % max(len(vb), 1)]) for k in uniq.tolist()]
            if not number:
                return pairs, pair_lines, None, None, 0, 0, 0
            nlocs, _, _ = fm.locate_all_batch(nch, noff, -1)
            if query:  # the number hits pass the filter on their own
                flines, _, _ = fm.match_query_batch(tch, toff, query_off, kinds)
                fstart, fstop = fm.line_bounds(flines)[:2] if len(flines) else (np.zeros(0, np.int32), np.zeros(0, np.int32))
                at = np.searchsorted(fstart, nlocs, side="right") - 1
                nlocs = nlocs[(at >= 0) & (nlocs < fstop[np.maximum(at, 0)])] if len(flines) else nlocs[:0]
            kept, P = len(nlocs), len(pairs)
            if len(both) == 0:
                return pairs, pair_lines, np.zeros(0, np.int64), [], kept, 0, kept
            start, stop = fm.line_bounds(both)[:2]
            at = np.searchsorted(start, nlocs, side="right") - 1
            has = (at >= 0) & (nlocs < stop[np.maximum(at, 0)])
            no_key = int((~has).sum())
            s = np.minimum(nlocs[has].astype(np.int64) + len(number), text_len)
            chars, text_off, _ = fm.extract_packed_batch(s, np.minimum(s + WINDOW, text_len))
            ok, value = parse_windows(chars, text_off)
            g = pair_of_line.reshape(-1)[at[has]][ok]
            value = value[ok]
            order = np.lexsort((value, g))
            g, value = g[order], value[order]
            edge = np.searchsorted(g, np.arange(P + 1), side="left")
            count = np.diff(edge)
            sums = [0] * P
            full = np.flatnonzero(count)
            if len(full):
                lo = np.add.reduceat(value & np.uint64(0xffffffff), edge[full])
                hi = np.add.reduceat(value >> np.uint64(32), edge[full])
                for k, gk in enumerate(full):
                    sums[gk] = (int(hi[k]) << 32) + int(lo[k])
            return pairs, pair_lines, count, sums, no_key, int((~ok).sum()), kept

        raw = new()
        c_pairs, c_lines, c_count, c_sums, c_no_key, c_nn, c_kept = composition()
        got = ia.fmindex._pair_values(raw, 0)
        assert [v for v, _ in got] == c_pairs and [c for _, c in got] == [int(x) for x in c_lines], name
        if number:
            out = ia.NumberStatsByPair(raw)
            assert [g["count"] for g in out.groups] == [int(x) for x in c_count] and [g["sum"] for g in out.groups] == c_sums, name
            assert (out.no_key, out.not_number, out.overflow, out.kept) == (c_no_key, c_nn, 0, c_kept), name
        row = timed({"by_pair": new, "floor": floor, "composition": composition})
        row.update({"number": number, "key_a": key_a, "key_b": key_b, "query": query, "pairs": len(got), "lines_with_both": int(sum(c for _, c in got)),
                    "kept": raw["kept"].tolist(), "key_kept": raw["key_kept"].tolist(), "no_key": raw["no_key"].tolist()})
        compare(row, "by_pair", "composition")
        compare(row, "floor", "by_pair")
        result["legs"][name] = row
        log("%s: %s" % (name, json.dumps(row)))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The lines that match a query of several terms — fmx_match_query_batch (the set algebra on the device, the lines of the QUERIES
come down) — against the composition the library offered before it, as a caller would run it: fmx_match_lines_batch over all terms
(the lines of every TERM come down), then np.intersect1d / np.union1d / np.setdiff1d per query on one host core.  One process,
one index (the log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default residency), line table for '\\n': the
index and the timing method of tools/match_lines_bench.py.

Legs:
  1. heavy: ONE query over the most frequent strings of 1..4 characters (picked on a 16 MiB sample): all = the two most frequent,
     none = the third (by count()).
  2. mixed: queries of three 8-character patterns of configs[2] (any, any, none) plus two queries over the frequent strings
     (all, all, none) in one call.
  3. uniform: the queries of 8-character patterns alone.
     This version takes at most 2^31 - 1 hits per call (fmx.h); legs 2 and 3 take the longest prefix of the 100,000 patterns whose
     hits stay below --max-hits (the frequent strings of leg 2 come on top).
Both routes are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the two routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  Before anything is timed the new form's lines, offsets and counts of EVERY leg are
compared with what the composition computes.  The oracle (tests/orc.py, reading the index's own serialized form) judges the
lines of the first --oracle-sample queries of leg 3 whose terms have at most 4,096 hits each.
Recorded per leg: terms, queries, hits, lines of the terms, lines of the queries, and the bytes each route brings over PCIe
(results only; the patterns go up in both).
usage: python tools/match_query_bench.py [--text-log2 28] [--repeats 5] [--out profiles/match_query.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALL, ANY, NONE = 0, 1, 2


def algebra(per, query_off, kinds):
    """the lines of every query from the lines of every term: the set formula of fmx.h, in numpy"""
    out = []
    for Q in range(len(query_off) - 1):
        terms = range(query_off[Q], query_off[Q + 1])
        alls = [per[t] for t in terms if kinds[t] == ALL]
        anys = [per[t] for t in terms if kinds[t] == ANY]
        if not alls and not anys:
            out.append(np.zeros(0, np.int32))
            continue
        res = None
        for a in alls:
            res = a if res is None else np.intersect1d(res, a, assume_unique=True)
        if anys:
            u = anys[0]
            for a in anys[1:]:
                u = np.union1d(u, a)
            res = u if res is None else np.intersect1d(res, u, assume_unique=True)
        for t in terms:
            if kinds[t] == NONE:
                res = np.setdiff1d(res, per[t], assume_unique=True)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle-sample", type=int, default=300)
    ap.add_argument("--max-hits", type=int, default=1 << 26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload
    import orc
    from locate_all_bench import frequent_strings

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "heavy": {}, "mixed": {}, "uniform": {}}

    def log(msg):
        print("[match_query_bench] " + msg, file=sys.stderr, flush=True)
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

    text = workload.log_text(args.text_log2)
    t16 = ia.as_chars(text)
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = fm.build_line_table("\n")
    result["lines"] = int(n_lines)

    def composition(ch, off, query_off, kinds):
        lines, line_off, st, line_count, occ = fm.match_lines_batch(ch, off, 0, want_counts=True)
        per = [lines[line_off[t]:line_off[t + 1]] for t in range(len(off) - 1)]
        return algebra(per, query_off, kinds), line_off, occ

    def leg(queries):
        """queries: lists of (pattern, kind)"""
        ch, off = ia.pack_patterns([p for qu in queries for p, _ in qu])
        off = np.ascontiguousarray(off, dtype=np.int32)
        kinds = np.array([k for qu in queries for _, k in qu], np.uint8)
        query_off = np.concatenate([[0], np.cumsum([len(qu) for qu in queries])]).astype(np.int32)
        n, q = len(off) - 1, len(queries)
        lines, line_off, st, line_count, occ = fm.match_query_batch(ch, off, query_off, kinds, 0, want_counts=True)
        per, term_line_off, term_occ = composition(ch, off, query_off, kinds)
        assert (line_count == [len(u) for u in per]).all() and (occ == term_occ).all() and (np.diff(line_off) == line_count).all()
        assert (lines == (np.concatenate(per) if len(lines) else lines)).all()
        row = timed({"match_query": lambda: fm.match_query_batch(ch, off, query_off, kinds, 0, want_counts=True),
                     "composition": lambda: composition(ch, off, query_off, kinds)})
        a, b = row["composition"], row["match_query"]
        row.update({"terms": n, "queries": q, "hits": int(occ.astype(np.int64).sum()), "lines_of_terms": int(term_line_off[-1]),
                    "lines_of_queries": int(line_off[-1]),
                    "bytes_down_match_query": int(line_off[-1]) * 4 + (q + 1) * 8 + q * 4 + 2 * n * 4,
                    "bytes_down_composition": int(term_line_off[-1]) * 4 + (n + 1) * 8 + 3 * n * 4,
                    "ratio_composition_over_match_query": a["ms"] / b["ms"],
                    "match_query_faster_by_more_than_the_spread": bool(a["min_ms"] > b["max_ms"]),
                    "composition_faster_by_more_than_the_spread": bool(b["min_ms"] > a["max_ms"])})
        return row, (ch, off, query_off, kinds, lines, line_off)

    strings, counts = frequent_strings(t16, fm, ia)
    order = np.argsort(-np.array(counts), kind="stable")
    strings, counts = [strings[i] for i in order], [counts[i] for i in order]
    result["strings"] = [{"string": ia.chars_to_str(s), "count": c} for s, c in zip(strings, counts)]
    log("lines %d, strings: %s" % (n_lines, json.dumps(result["strings"])))
    #     (all, all, none) over the strings by frequency: 0 1 2, then 3 4 5
    heavy = [[(strings[i], ALL), (strings[i + 1], ALL), (strings[i + 2], NONE)] for i in (0, 3)]
    result["heavy"], _ = leg(heavy[:1])
    log("heavy: %s" % json.dumps(result["heavy"]))
    cpat, coff, _ = workload.count_batch_patterns(text, 100_000, 8)
    all_counts, _ = fm.count_batch(cpat, coff)
    budget = args.max_hits  # (of the 8-character patterns; the six frequent strings of leg 2 come on top)
    cum = np.cumsum(all_counts.astype(np.int64))
    k = int(np.searchsorted(cum, max(budget, 1), side="right")) // 3 * 3
    result["patterns_8_char"] = {"of": 100_000, "hits_of_all": int(cum[-1]), "taken": k, "hits_taken": int(cum[k - 1]) if k else 0,
                                 "max_hits": args.max_hits}
    log("8-character patterns: %s" % json.dumps(result["patterns_8_char"]))
    assert k >= 3
    pats = [cpat[coff[i]:coff[i + 1]] for i in range(k)]
    triples = [[(pats[i], ANY), (pats[i + 1], ANY), (pats[i + 2], NONE)] for i in range(0, k, 3)]
    result["mixed"], _ = leg(triples + heavy)
    log("mixed: %s" % json.dumps(result["mixed"]))
    result["uniform"], (ch, off, query_off, kinds, lines, line_off) = leg(triples)
    log("uniform: %s" % json.dumps(result["uniform"]))
    # the oracle on a sample of the uniform leg: the lines of every term from its locate(), the set formula over them
    o = orc.OracleFmIndex.read(fm.write(False))
    nl = np.array([10], np.uint16)
    kT, oT = o.locate(nl, max_matches=-1, cap=o.count(nl) + 1)
    oT = np.sort(oT).astype(np.int32)
    small = [Q for Q in range(len(triples)) if all_counts[3 * Q:3 * Q + 3].max() <= 4096][: args.oracle_sample]
    for Q in small:
        per = []
        for t in range(3 * Q, 3 * Q + 3):
            cnt, locs = o.locate(pats[t], max_matches=-1, cap=int(all_counts[t]) + 1)
            per.append(np.unique(np.searchsorted(oT, locs[:cnt], side="left")))
        want = np.setdiff1d(np.union1d(per[0], per[1]), per[2])
        assert (lines[line_off[Q]:line_off[Q + 1]] == want).all(), Q
    result["oracle"] = {"table_entries": int(kT), "queries_checked": len(small)}
    log("oracle: %d queries of the uniform leg checked" % len(small))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

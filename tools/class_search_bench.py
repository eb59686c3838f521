#!/usr/bin/env python3
"""Patterns of character classes — fmx_count_class_batch / fmx_match_query_class_batch (a frontier of SA ranges per pattern on the
device) — against the composition they replace, as a caller ran it before: every spelling of a word as a literal pattern.  One
process, one index (the log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default residency), line table for
'\\n': the index and the timing method of tools/match_query_bench.py.

Legs:
  1. count: ignore_case of --words 8-letter words of the text in ONE fmx_count_class_batch call, against the 2^8 spellings of
     every word through fmx_count_batch (one call over words x 256 patterns), summed per word on the host.
  2. query: per word ONE query whose single term is the class pattern (ALL), through fmx_match_query_class_batch, against
     fmx_match_query_batch with the word's spellings as ANY terms of one query (256 terms per query).
Both routes are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the two routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  Before anything is timed the class form's counts, lines and offsets are compared
with the composition's.  Packing the spellings is NOT timed (it favours the composition).
usage: python tools/class_search_bench.py [--text-log2 28] [--words 64] [--repeats 5] [--out profiles/class_search.json]"""
import argparse
import itertools
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ALL, ANY = 0, 1


def spellings(word):
    """every spelling of a word under ASCII case, as strs (2^k for k letters)"""
    return ["".join(s) for s in itertools.product(*[sorted({c.lower(), c.upper()}) for c in word])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--words", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-ranges", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "max_ranges": args.max_ranges, "count": {}, "query": {}}

    def log(msg):
        print("[class_search_bench] " + msg, file=sys.stderr, flush=True)
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
        row.update({"ratio_composition_over_class": a["ms"] / b["ms"], "class_faster_by_more_than_the_spread": bool(a["min_ms"] > b["max_ms"]),
                    "composition_faster_by_more_than_the_spread": bool(b["min_ms"] > a["max_ms"])})
        return row

    text = workload.log_text(args.text_log2)
    sample = ia.chars_to_str(ia.as_chars(text)[: 1 << 24])
    words = sorted(set(w.lower() for w in re.findall(r"[A-Za-z]{8}", sample)))[: args.words]
    assert len(words) >= 4, "the text has too few 8-letter words"
    result["words"] = words
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    result["lines"] = int(fm.build_line_table("\n"))

    # leg 1: counts
    packed = ia.pack_class_patterns([ia.ignore_case(w) for w in words])
    every = [spellings(w) for w in words]
    assert all(len(s) == 256 for s in every)
    ch, off = ia.pack_patterns([s for group in every for s in group])
    off = np.ascontiguousarray(off, dtype=np.int32)

    def by_class():
        return fm.count_class_batch(*packed, max_ranges=args.max_ranges)

    def by_spellings():
        counts, status = fm.count_batch(ch, off)
        return counts.reshape(len(words), 256).sum(axis=1), status

    counts, status = by_class()
    assert (status == 0).all() and (counts == by_spellings()[0]).all()
    result["count"] = compare(timed({"class": by_class, "composition": by_spellings}), "class", "composition")
    result["count"].update({"words": len(words), "literal_patterns": len(off) - 1, "occurrences": int(counts.astype(np.int64).sum())})
    log("count: %s" % json.dumps(result["count"]))

    # leg 2: the lines of every word in any case
    q = len(words)
    class_qoff, class_kinds = np.arange(q + 1, dtype=np.int32), np.full(q, ALL, np.uint8)
    lit_qoff, lit_kinds = (np.arange(q + 1) * 256).astype(np.int32), np.full(q * 256, ANY, np.uint8)

    def query_class():
        return fm.match_query_class_batch(*packed, class_qoff, class_kinds, 0, want_counts=True, max_ranges=args.max_ranges)

    def query_spellings():
        return fm.match_query_batch(ch, off, lit_qoff, lit_kinds, 0, want_counts=True)

    new, old = query_class(), query_spellings()
    assert (new[0] == old[0]).all() and (new[1] == old[1]).all() and (new[3] == old[3]).all()
    result["query"] = compare(timed({"class": query_class, "composition": query_spellings}), "class", "composition")
    result["query"].update({"queries": q, "class_terms": q, "literal_terms": q * 256, "lines": int(new[1][-1])})
    log("query: %s" % json.dumps(result["query"]))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

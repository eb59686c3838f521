#!/usr/bin/env python3
"""The lines that hold a sequence of terms in order (grep 'A.*B') — fmx_match_sequence_batch (the chaining on the device, the lines
of the SEQUENCES come down) — against the composition the library offered before it, as a caller would run it: fmx_locate_all_batch
over all terms (every hit of every TERM comes down), then the same earliest-fit chain in numpy on one host core (per sequence: the
first term's hits sorted, the first of each line, one np.searchsorted per further term).  One process, one index (the log text of
bench.py, 2^--text-log2 characters, sampleRate 32, the default residency), line table for '\\n': the index and the timing method
of tools/match_query_bench.py.  The composition gets the boundaries (locate_all of '\\n', sorted) outside the clock.

Legs:
  1. heavy: ONE sequence over the three most frequent strings of 1..4 characters that do not hold the boundary (picked on a
     16 MiB sample, ordered by count()).
  2. uniform: --sequences sequences of two and of three 8-character patterns of configs[2], alternating; the longest prefix whose
     hits stay below --max-hits.
Both routes are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the two routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  Before anything is timed the new form's lines, offsets, counts and spans of EVERY
leg are compared with what the composition computes.
Recorded per leg: terms, sequences, hits, lines of the sequences, and the bytes each route brings over PCIe (results only).
usage: python tools/match_sequence_bench.py [--text-log2 28] [--repeats 5] [--out profiles/match_sequence.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def chain(T, text_len, hits, lens):
    """(lines, spans) of ONE sequence from the hits of its terms: the earliest-fit rule of fmx.h, in numpy"""
    if not hits or min(len(h) for h in hits) == 0:
        return np.zeros(0, np.int32), np.zeros((0, 2), np.int32)
    H = [np.sort(h.astype(np.int64)) for h in hits]
    first = H[0][H[0] >= 0]
    line = np.searchsorted(T, first, side="left")
    line, head = np.unique(line, return_index=True)
    at = first[head] + lens[0]
    stop = np.where(line < len(T), T[np.minimum(line, len(T) - 1)] if len(T) else text_len, text_len).astype(np.int64)
    ok = at <= stop
    for h, m in zip(H[1:], lens[1:]):
        j = np.searchsorted(h, at, side="left")
        ok &= j < len(h)
        at = h[np.minimum(j, len(h) - 1)] + m
        ok &= at <= stop
    return line[ok].astype(np.int32), np.stack([first[head][ok], at[ok]], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=300)
    ap.add_argument("--max-hits", type=int, default=1 << 26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload
    from locate_all_bench import frequent_strings

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "heavy": {}, "uniform": {}}

    def log(msg):
        print("[match_sequence_bench] " + msg, file=sys.stderr, flush=True)
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
    log("text of %d characters" % len(t16))
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = fm.build_line_table("\n")
    result["lines"] = int(n_lines)
    T = np.sort(fm.locate_all("\n")).astype(np.int64)

    def composition(ch, off, query_off):
        locs, hit_off, st = fm.locate_all_batch(ch, off)
        lens = np.diff(off).astype(np.int64)
        out = []
        for Q in range(len(query_off) - 1):
            terms = range(query_off[Q], query_off[Q + 1])
            out.append(chain(T, len(t16), [locs[hit_off[t]:hit_off[t + 1]] for t in terms], [int(lens[t]) for t in terms]))
        return out, hit_off

    def leg(sequences):
        """sequences: lists of patterns"""
        ch, off = ia.pack_patterns([p for sq in sequences for p in sq])
        off = np.ascontiguousarray(off, dtype=np.int32)
        query_off = np.concatenate([[0], np.cumsum([len(sq) for sq in sequences])]).astype(np.int32)
        n, q = len(off) - 1, len(sequences)
        lines, line_off, st, line_count, occ, spans = fm.match_sequence_batch(ch, off, query_off, 0, want_counts=True, want_spans=True)
        per, hit_off = composition(ch, off, query_off)
        assert (line_count == [len(u) for u, _ in per]).all() and (occ == np.diff(hit_off)).all() and (np.diff(line_off) == line_count).all()
        assert (lines == np.concatenate([u for u, _ in per])).all() and (spans == np.concatenate([s for _, s in per])).all()
        row = timed({"match_sequence": lambda: fm.match_sequence_batch(ch, off, query_off, 0, want_counts=True),
                     "composition": lambda: composition(ch, off, query_off)})
        a, b = row["composition"], row["match_sequence"]
        row.update({"terms": n, "sequences": q, "hits": int(hit_off[-1]), "lines_of_sequences": int(line_off[-1]),
                    "bytes_down_match_sequence": int(line_off[-1]) * 4 + (q + 1) * 8 + q * 4 + 2 * n * 4,
                    "bytes_down_composition": int(hit_off[-1]) * 4 + (n + 1) * 8 + n * 4,
                    "ratio_composition_over_match_sequence": a["ms"] / b["ms"],
                    "match_sequence_faster_by_more_than_the_spread": bool(a["min_ms"] > b["max_ms"]),
                    "composition_faster_by_more_than_the_spread": bool(b["min_ms"] > a["max_ms"])})
        return row

    strings, counts = frequent_strings(t16, fm, ia)
    keep = [i for i in np.argsort(-np.array(counts), kind="stable") if not (strings[i] == 10).any()][:3]
    strings, counts = [strings[i] for i in keep], [counts[i] for i in keep]
    result["strings"] = [{"string": ia.chars_to_str(s), "count": c} for s, c in zip(strings, counts)]
    log("lines %d, strings: %s" % (n_lines, json.dumps(result["strings"])))
    result["heavy"] = leg([strings])
    log("heavy: %s" % json.dumps(result["heavy"]))
    sizes = [2 + (i & 1) for i in range(args.sequences)]
    cpat, coff, _ = workload.count_batch_patterns(text, sum(sizes), 8)
    all_counts, _ = fm.count_batch(cpat, coff)
    cum = np.cumsum(all_counts.astype(np.int64))
    sequences, at = [], 0
    for k in sizes:
        if cum[at + k - 1] > args.max_hits:
            break
        sequences.append([cpat[coff[i]:coff[i + 1]] for i in range(at, at + k)])
        at += k
    result["patterns_8_char"] = {"of": int(sum(sizes)), "hits_of_all": int(cum[-1]), "taken": at, "hits_taken": int(cum[at - 1]) if at else 0,
                                 "max_hits": args.max_hits}
    log("8-character patterns: %s" % json.dumps(result["patterns_8_char"]))
    assert sequences
    result["uniform"] = leg(sequences)
    log("uniform: %s" % json.dumps(result["uniform"]))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

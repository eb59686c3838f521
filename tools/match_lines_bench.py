#!/usr/bin/env python3
"""The lines that match — fmx_match_lines_batch (hits -> distinct lines on the device, the lines come down) — against today's route
as a caller would run it: fmx_locate_all_batch (every hit comes down), then np.searchsorted over the boundary positions and
np.unique per pattern on one host core.  One process, one index (the log text of bench.py, 2^--text-log2 characters, sampleRate
32, the default residency), line table for '\\n'.

Legs:
  1. heavy: the 8 most frequent strings of 1..4 characters (picked on a 16 MiB sample, exact counts from count()), each as a
     batch of ONE.
  2. mixed: 8-character patterns of configs[2] plus those 8 strings in one call.
  3. uniform: the 8-character patterns alone.
     Both routes return EVERY hit's line, and this version takes at most 2^31 - 1 hits per call (fmx.h): the 100,000 patterns of
     configs[2] have more on this text (their counts are summed first and recorded), so legs 2 and 3 take the longest prefix
     of them whose hits stay below --max-hits (2^26: 256 MiB of positions for today's route).
  4. the table build (the table replaced by an empty one for another character before every timed build).
Both routes are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the two routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  Before anything is timed the new form's lines, offsets and counts of EVERY leg are
compared with what today's route computes from the library's own locate().  The oracle (tests/orc.py, reading the index's own
serialized form) judges what it can judge in minutes on one host: the line table itself (its sorted locate() of the boundary
against the table read back through line_bounds) and the lines and counts of --oracle-sample 8-character patterns (the first
of the 100,000 with at most 4,096 hits); the
heavy strings (10^7 hits each: an hour of the oracle's single-threaded walks) are judged through today's route only.
Recorded per leg: hits, lines, and the bytes each route brings over PCIe (results only; the patterns go up in both).
usage: python tools/match_lines_bench.py [--text-log2 28] [--repeats 5] [--out profiles/match_lines.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle-sample", type=int, default=1000)
    ap.add_argument("--max-hits", type=int, default=1 << 26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload
    import orc
    from locate_all_bench import frequent_strings

    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "heavy": {}, "mixed": {}, "uniform": {}, "table_build": {}}

    def log(msg):
        print("[match_lines_bench] " + msg, file=sys.stderr, flush=True)
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
    t0 = time.perf_counter()
    n_lines = fm.build_line_table("\n")
    first_build = (time.perf_counter() - t0) * 1e3
    T = np.sort(fm.locate_all("\n"))  # today's route keeps the boundary positions on the host
    assert len(T) == fm.line_table_info()[1]
    # the oracle's table against the resident one, read back
    o = orc.OracleFmIndex.read(fm.write(False))
    nl = np.array([10], np.uint16)
    k, oT = o.locate(nl, max_matches=-1, cap=o.count(nl) + 1)
    oT = np.sort(oT).astype(np.int32)
    assert k == len(T) and (oT == T).all()
    assert (fm.line_bounds(np.arange(len(oT), dtype=np.int32))[1] == oT).all()
    result["oracle"] = {"table_entries": int(k)}
    log("line table of %d entries equals the oracle's" % k)

    def todays_route(ch, off):
        locs, hit_off, st = fm.locate_all_batch(ch, off)
        lines = [np.unique(np.searchsorted(T, locs[hit_off[i]:hit_off[i + 1]], side="left")) for i in range(len(off) - 1)]
        return lines, hit_off

    def leg(ch, off):
        off = np.ascontiguousarray(off, dtype=np.int32)
        n = len(off) - 1
        lines, line_off, st, line_count, occ = fm.match_lines_batch(ch, off, 0, want_counts=True)
        per, hit_off = todays_route(ch, off)
        assert (line_count == [len(u) for u in per]).all() and (occ == np.diff(hit_off)).all()
        assert (lines == (np.concatenate(per) if len(lines) else lines)).all()
        row = timed({"match_lines": lambda: fm.match_lines_batch(ch, off, 0, want_counts=True), "today": lambda: todays_route(ch, off)})
        a, b = row["today"], row["match_lines"]
        row.update({"patterns": n, "hits": int(hit_off[-1]), "lines": int(line_off[-1]),
                    "bytes_down_match_lines": int(line_off[-1]) * 4 + (n + 1) * 8 + 3 * n * 4,
                    "bytes_down_today": int(hit_off[-1]) * 4 + (n + 1) * 8 + n * 4,
                    "ratio_today_over_match_lines": a["ms"] / b["ms"],
                    "match_lines_faster_by_more_than_the_spread": bool(a["min_ms"] > b["max_ms"]),
                    "today_faster_by_more_than_the_spread": bool(b["min_ms"] > a["max_ms"])})
        return row

    strings, counts = frequent_strings(t16, fm, ia)
    result["lines"] = int(n_lines)
    result["strings"] = [{"string": ia.chars_to_str(s), "count": c} for s, c in zip(strings, counts)]
    log("lines %d, strings: %s" % (n_lines, json.dumps(result["strings"])))
    for s in strings:
        row = leg(s, np.array([0, len(s)], np.int32))
        result["heavy"][ia.chars_to_str(s)] = row
        log("heavy %r: %s" % (ia.chars_to_str(s), json.dumps(row)))
    cpat, coff, _ = workload.count_batch_patterns(text, 100_000, 8)
    all_counts, _ = fm.count_batch(cpat, coff)
    cum = np.cumsum(all_counts.astype(np.int64))
    k = int(np.searchsorted(cum, args.max_hits, side="right"))
    result["patterns_8_char"] = {"of": 100_000, "hits_of_all": int(cum[-1]), "taken": k, "hits_taken": int(cum[k - 1]) if k else 0,
                                 "max_hits": args.max_hits}
    log("8-character patterns: %s" % json.dumps(result["patterns_8_char"]))
    assert k >= 1
    apat, aoff = cpat, coff
    cpat, coff = cpat[coff[0]:coff[k]], (coff[: k + 1] - coff[0]).astype(np.int32)
    mch, moff = ia.pack_patterns([cpat[coff[i]:coff[i + 1]] for i in range(len(coff) - 1)] + strings)
    result["mixed"] = leg(mch, moff)
    log("mixed: %s" % json.dumps(result["mixed"]))
    result["uniform"] = leg(cpat, coff)
    log("uniform: %s" % json.dumps(result["uniform"]))
    # the oracle on a sample of the uniform leg: counts, and the lines of its hits
    keep = np.flatnonzero(all_counts <= 4096)[: args.oracle_sample]  # (of all 100,000; the oracle's rows are as wide as the largest count)
    m = len(keep)
    if m:
        sch, soff = ia.pack_patterns([apat[aoff[i]:aoff[i + 1]] for i in keep])
        soff = soff.astype(np.int32)
        oc, _ = o.count_batch(sch, soff, threads=16)
        olocs, ofound, _ = o.locate_batch(sch, soff, -1, max(int(oc.max()), 1), threads=16)
        lines, line_off, st, line_count, occ = fm.match_lines_batch(sch, soff, 0, want_counts=True)
        assert (occ == oc).all() and (ofound == oc).all()
        for i in range(m):
            assert (lines[line_off[i]:line_off[i + 1]] == np.unique(np.searchsorted(oT, olocs[i, : ofound[i]], side="left"))).all(), i
    result["oracle"]["patterns_checked"] = int(m)
    log("oracle: %d of the 8-character patterns checked" % m)
    builds = []
    for _ in range(args.repeats):
        fm.build_line_table(1)  # (another character: the table is replaced)
        t0 = time.perf_counter()
        assert fm.build_line_table("\n") == n_lines
        builds.append((time.perf_counter() - t0) * 1e3)
    nb, nbytes = fm.line_table_info()[1:]
    result["table_build"] = {"ms": float(np.median(builds)), "min_ms": float(min(builds)), "max_ms": float(max(builds)), "first_ms": first_build,
                             "boundaries": int(nb), "bytes": int(nbytes)}
    log("table build: %s" % json.dumps(result["table_build"]))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

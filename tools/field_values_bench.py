#!/usr/bin/env python3
"""The values that follow a pattern, with counts (grep -o 'blk_[^ ]*' | sort | uniq -c) — fmx_field_values_batch /
fmx_field_values_class_batch (windows, runs and the exact grouping on the device, only the GROUPS come down) — against the
composition the library offered before it, as a caller would run it: locate_all_batch (every hit comes down), extract_packed_batch
of the window behind every hit (every window comes down), then the grouping with numpy on one host core.  One process, one index
(the log text of bench.py, 2^--text-log2 characters, sampleRate 32, the default residency): the index and the timing method of
tools/match_query_bench.py.

Legs:
  1. words: the 8-letter words of tools/class_search_bench.py in any case (class patterns), stop set " \\t\\r\\n", max_len 32.
  2. prefixes: ONE frequent prefix ("blk_") plus --rare 8-character patterns of at most 16 hits each (literal patterns), the same
     stop set and max_len.
Both routes are host-synchronous calls over host arrays, so the clock is the host's (time.perf_counter) around one call; two
untimed calls first, the two routes ALTERNATED --repeats times; median, min and max per route; a comparison holds when the slower
route's min is above the faster route's max.  Before anything is timed the new form's values, offsets and counts of EVERY leg are
compared with what the composition computes.  Recorded per leg: patterns, hits, R (the runs of neighbouring hits with one value,
counted on the host from the composition's windows), groups, R / hits, groups / R, and the bytes each route brings over PCIe
(results only; the patterns go up in both, the composition's windows' ranges as well).
usage: python tools/field_values_bench.py [--text-log2 28] [--repeats 5] [--rare 4096] [--out profiles/field_values.json]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def windows_of(locs, hit_off, lens, max_len, text_len):
    """[s, e) behind every hit, by the definition of fmx.h"""
    which = np.repeat(np.arange(len(hit_off) - 1), np.diff(hit_off))
    s = np.clip(locs.astype(np.int64) + np.asarray(lens, np.int64)[which], 0, text_len)
    return s.astype(np.int32), np.minimum(s + max_len, text_len).astype(np.int32), which


def host_group(which, n, chars, text_off, stop, max_len):
    """the grouping on one host core: the windows as rows of big-endian code units padded with 0, the value's length behind them
    (np.unique over the rows' bytes is then the order of fmx.h: by code unit, a value in front of its extensions, a value in front
    of the same value followed by U+0000).  Returns (chars, text_off, counts, val_off, runs)."""
    hits = len(which)
    ln = np.diff(text_off)
    rows = np.zeros((hits, max_len + 1), ">u2")
    inside = np.arange(max_len)[None, :] < ln[:, None]
    rows[:, :max_len][inside] = chars
    stops_at = np.isin(rows[:, :max_len], np.unique(stop)) & inside
    vlen = np.where(stops_at.any(axis=1), stops_at.argmax(axis=1), ln)
    rows[:, :max_len][np.arange(max_len)[None, :] >= vlen[:, None]] = 0
    rows[:, max_len] = vlen
    keys = np.ascontiguousarray(rows).view(np.dtype((np.void, rows.shape[1] * 2))).reshape(-1)
    differs = np.ones(hits, bool)
    differs[1:] = (keys[1:] != keys[:-1]) | (which[1:] != which[:-1])
    out_rows, out_counts, val_off = [], [], [0]
    bounds = np.searchsorted(which, np.arange(n + 1))
    for i in range(n):
        u, c = np.unique(keys[bounds[i]:bounds[i + 1]], return_counts=True)
        out_rows.append(u)
        out_counts.append(c)
        val_off.append(val_off[-1] + len(u))
    allrows = np.concatenate(out_rows).view(">u2").reshape(-1, max_len + 1) if val_off[-1] else np.zeros((0, max_len + 1), ">u2")
    glen = allrows[:, max_len].astype(np.int64)
    g_off = np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)
    g_chars = allrows[:, :max_len][np.arange(max_len)[None, :] < glen[:, None]].astype(np.uint16)
    counts = np.concatenate(out_counts).astype(np.int32) if val_off[-1] else np.zeros(0, np.int32)
    return g_chars, g_off, counts, np.array(val_off, np.int64), int(differs.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rare", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import index4j_amd as ia
    from index4j_amd import workload

    STOP, MAX_LEN = " \t\r\n", 32
    stop16 = ia.as_chars(STOP)
    result = {"text_log2": args.text_log2, "repeats": args.repeats, "sample_rate": 32, "stop": STOP, "max_len": MAX_LEN, "words": {}, "prefixes": {}}

    def log(msg):
        print("[field_values_bench] " + msg, file=sys.stderr, flush=True)
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
    text_len = len(t16)
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)

    def leg(new, locate, lens):
        """new() -> field_values_*_batch's tuple; locate() -> (locs, hit_off, status)"""
        n = len(lens)

        def composition(parts=None):
            t0 = time.perf_counter()
            locs, hit_off, _ = locate()
            t1 = time.perf_counter()
            s, e, which = windows_of(locs, hit_off, lens, MAX_LEN, text_len)
            chars, text_off, st = fm.extract_packed_batch(s, e)
            t2 = time.perf_counter()
            out = host_group(which, n, chars, text_off, stop16, MAX_LEN)
            if parts is not None:
                parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
            return out + (int(hit_off[-1]), int(text_off[-1]))

        chars, text_off, counts, val_off, st, occ = new()
        c_chars, c_off, c_counts, c_val_off, runs, hits, units = composition()
        assert (val_off == c_val_off).all() and (counts == c_counts).all() and (text_off == c_off).all() and (chars == c_chars).all()
        assert int(occ.astype(np.int64).sum()) == hits == int(counts.astype(np.int64).sum())
        parts = []
        row = timed({"field_values": new, "composition": lambda: composition(parts)})
        a, b = row["composition"], row["field_values"]
        groups = int(val_off[-1])
        last = np.array(parts[-args.repeats:])
        row.update({"patterns": n, "hits": hits, "runs": runs, "groups": groups, "runs_over_hits": runs / max(hits, 1),
                    "groups_over_runs": groups / max(runs, 1),
                    "composition_parts_ms": {"locate_all": float(np.median(last[:, 0])), "extract_packed": float(np.median(last[:, 1])),
                                             "numpy_grouping": float(np.median(last[:, 2]))},
                    "bytes_down_field_values": groups * 4 + (groups + 1) * 8 + int(text_off[-1]) * 2 + (n + 1) * 8 + 2 * n * 4,
                    "bytes_down_composition": hits * 4 + (n + 1) * 8 + n * 4 + units * 2 + (hits + 1) * 8 + hits * 4,
                    "ratio_composition_over_field_values": a["ms"] / b["ms"],
                    "field_values_faster_by_more_than_the_spread": bool(a["min_ms"] > b["max_ms"]),
                    "composition_faster_by_more_than_the_spread": bool(b["min_ms"] > a["max_ms"])})
        return row

    # leg 1: the 8-letter words of tools/class_search_bench.py, in any case
    sample = ia.chars_to_str(t16[: 1 << 24])
    words = sorted(set(w.lower() for w in re.findall(r"[A-Za-z]{8}", sample)))[:64]
    assert len(words) >= 4, "the text has too few 8-letter words"
    result["word_list"] = words
    packed = ia.pack_class_patterns([ia.ignore_case(w) for w in words])
    result["words"] = leg(lambda: fm.field_values_class_batch(*packed, STOP, MAX_LEN), lambda: fm.locate_all_class_batch(*packed), [8] * len(words))
    log("words: %s" % json.dumps(result["words"]))
    # leg 2: one frequent prefix and many rare ones
    cpat, coff, _ = workload.count_batch_patterns(text, 100_000, 8)
    all_counts, _ = fm.count_batch(cpat, coff)
    rare = np.flatnonzero((all_counts >= 1) & (all_counts <= 16))[: args.rare]
    pats = ["blk_"] + [cpat[coff[i]:coff[i + 1]] for i in rare]
    ch, off = ia.pack_patterns(pats)
    off = np.ascontiguousarray(off, dtype=np.int32)
    result["prefixes"] = leg(lambda: fm.field_values_batch(ch, off, STOP, MAX_LEN), lambda: fm.locate_all_batch(ch, off, -1), np.diff(off))
    result["prefixes"]["hits_of_the_frequent_prefix"] = int(fm.count("blk_"))
    log("prefixes: %s" % json.dumps(result["prefixes"]))
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

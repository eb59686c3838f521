#!/usr/bin/env python3
"""locate(pattern, locations) — all occurrences — through the packed entry points (fmx_locate_all_ranges_dev + fmx_locate_all_fill_dev:
lanes handed to hits) against the row form (fmx_locate_batch_dev with loc_cap = the count: lanes handed to patterns), one process,
one index made resident twice: walking (the default residency) and with the row table (option "locate_rows" 1).

Legs, on the log text (2^--text-log2 characters, sampleRate 32):
  1. skewed: the 2 most frequent strings of each length 1..4 (picked on a 16 MiB sample, exact counts from count()), each as a
     batch of ONE with maxMatches -1; baseline = fmx_locate_batch_dev(loc_cap = count).
  2. mixed: 100,000 8-character patterns of configs[2] plus those 8 strings in one call (no baseline: rows of the largest count).
  3. uniform: configs[2] itself, maxMatches 16, against fmx_locate_batch_dev(16, 16).
Timing: HIP events around --batches calls (operands resident, both stages of the packed form inside the timed region, no host
wait between them: the grid is sized from the total a first call found), two untimed calls first, the legs of a comparison
ALTERNATED --repeats times; median, min and max per leg; a comparison holds when the slower leg's min is above the faster leg's
max.  Positions of the packed call are compared with the row form's before anything is timed.
usage: python tools/locate_all_bench.py [--text-log2 28] [--repeats 5] [--batches 5] [--out profiles/locate_all.json]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = {"locate_rows": 0}


@contextlib.contextmanager
def options(ia, **kw):
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
        yield
    finally:
        for k in kw:
            ia.lib.fmx_set_option(k.encode(), ia._lib.ENV_OPTIONS.get(k, DEFAULTS[k]))


def frequent_strings(t16, fm, ia, per_length=2, sample=1 << 24):
    """the most frequent strings of 1..4 characters: candidates from a sample of the text, counts from the index"""
    s = t16[:sample].astype(np.uint64)
    out = []
    for m in range(1, 5):
        key = s[: len(s) - m + 1].copy()
        for j in range(1, m):
            key = (key << np.uint64(16)) | s[j: len(s) - m + 1 + j]
        vals, cnt = np.unique(key, return_counts=True)
        for v in vals[np.argsort(cnt)[::-1][:per_length]]:
            out.append(np.array([(int(v) >> (16 * (m - 1 - j))) & 0xFFFF for j in range(m)], np.uint16))
    ch, off = ia.pack_patterns(out)
    counts, _ = fm.count_batch(ch, off)
    return out, [int(c) for c in counts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    import torch

    import index4j_amd as ia
    from index4j_amd import workload

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    result = {"text_log2": args.text_log2, "repeats": args.repeats, "batches": args.batches, "sample_rate": 32, "skewed": {}, "mixed": {},
              "uniform": {}}

    def log(msg):
        print("[locate_all_bench] " + msg, file=sys.stderr, flush=True)
        if args.out:  # (every leg that is done is on disk)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    def timed(calls, batches):
        """calls: {leg: callable}; alternated args.repeats times; {leg: {ms, min_ms, max_ms}}"""
        for call in calls.values():
            call()
            call()
        torch.cuda.synchronize()
        times = {leg: [] for leg in calls}
        for _ in range(args.repeats):
            for leg, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(batches[leg]):
                    call()
                e1.record(stream)
                torch.cuda.synchronize()
                times[leg].append(e0.elapsed_time(e1) / batches[leg])
        return {leg: {"ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for leg, t in times.items()}

    class Batch:
        """a batch resident in HBM with the buffers of both forms"""

        def __init__(self, fm, pat, off, mm, cap):
            self.h, self.n, self.mm, self.cap = fm.handle, len(off) - 1, mm, cap
            n = self.n
            self.d_pat = torch.from_numpy(np.ascontiguousarray(pat).view(np.int16)).to(dev)
            self.d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int32)).to(dev)
            z = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
            self.lf, self.st, self.rng, self.found = z(n), z(n), z(2 * n), z(n)
            self.hit_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            self.ranges()
            torch.cuda.synchronize()
            self.total = int(self.hit_off[n].item())
            self.locs = torch.full((max(self.total, 1),), -1, dtype=torch.int32, device=dev)
            self.rows = torch.full((max(n * cap, 1),), -1, dtype=torch.int32, device=dev) if cap else None

        def ranges(self):
            rc = ia.lib.fmx_locate_all_ranges_dev(self.h, self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, self.mm, self.hit_off.data_ptr(),
                                                  self.lf.data_ptr(), self.st.data_ptr(), self.rng.data_ptr(), sp)
            assert rc == 0, ia.lib.fmx_last_error()

        def packed(self):
            self.ranges()
            rc = ia.lib.fmx_locate_all_fill_dev(self.h, self.n, self.hit_off.data_ptr(), self.rng.data_ptr(), 0, self.total, self.locs.data_ptr(),
                                                self.lf.data_ptr(), self.st.data_ptr(), sp)
            assert rc == 0, ia.lib.fmx_last_error()

        def row_form(self):
            rc = ia.lib.fmx_locate_batch_dev(self.h, self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, self.mm, self.rows.data_ptr(), self.cap,
                                             self.found.data_ptr(), self.lf.data_ptr(), self.st.data_ptr(), self.rng.data_ptr(), sp)
            assert rc == 0, ia.lib.fmx_last_error()

        def check_equal(self):
            self.row_form()
            self.packed()
            torch.cuda.synchronize()
            found = self.found.cpu().numpy()[: self.n].astype(np.int64)
            hit_off = self.hit_off.cpu().numpy()
            assert (np.diff(hit_off) == found).all()
            rows = self.rows.cpu().numpy()[: self.n * self.cap].reshape(self.n, self.cap)
            assert (rows[np.arange(self.cap)[None, :] < found[:, None]] == self.locs.cpu().numpy()[: self.total]).all()

    def compare(row):
        a, b = row["row form"], row["packed"]
        row["ratio_row_over_packed"] = a["ms"] / b["ms"]
        row["packed_faster_by_more_than_the_spread"] = bool(a["min_ms"] > b["max_ms"])
        return row

    text = workload.log_text(args.text_log2)
    t16 = ia.as_chars(text)
    fm = ia.FmIndex(text, 32, True, device=None, build_device=0)
    cpat, coff, _ = workload.count_batch_patterns(text, 100_000, 8)
    strings = None
    for residency, rows_opt in (("walking", 0), ("row table", 1)):
        with options(ia, locate_rows=rows_opt):
            fm.to_device(0)
        assert (fm.locate_rows_info()[0] > 0) == bool(rows_opt)
        if strings is None:
            strings, counts = frequent_strings(t16, fm, ia)
            result["strings"] = [{"string": ia.chars_to_str(s), "count": c} for s, c in zip(strings, counts)]
            log("strings: %s" % json.dumps(result["strings"]))
        # 1. the skewed call
        for s, c in zip(strings, counts):
            b = Batch(fm, s, np.array([0, len(s)], np.int32), -1, c)
            assert b.total == c
            b.check_equal()
            few = max(1, min(args.batches, int(2e7 // max(c, 1))))  # (a row-form call over 10^7 hits takes seconds)
            row = timed({"row form": b.row_form, "packed": b.packed}, {"row form": few, "packed": args.batches})
            row["hits"] = c
            result["skewed"].setdefault(ia.chars_to_str(s), {})[residency] = compare(row)
            log("skewed %r %s: %s" % (ia.chars_to_str(s), residency, json.dumps(row)))
            del b
        # 2. the mixed batch
        mch, moff = ia.pack_patterns([cpat[coff[i]:coff[i + 1]] for i in range(len(coff) - 1)] + strings)
        b = Batch(fm, mch, moff, -1, 0)
        row = timed({"packed": b.packed}, {"packed": args.batches})
        row.update({"patterns": b.n, "hits": b.total, "bytes": b.total * 4 + (b.n + 1) * 8, "row_form_bytes": b.n * max(counts) * 4})
        result["mixed"][residency] = row
        log("mixed %s: %s" % (residency, json.dumps(row)))
        del b
        # 3. the uniform batch
        b = Batch(fm, cpat, coff, 16, 16)
        b.check_equal()
        row = timed({"row form": b.row_form, "packed": b.packed}, {"row form": args.batches, "packed": args.batches})
        row.update({"patterns": b.n, "hits": b.total})
        result["uniform"][residency] = compare(row)
        log("uniform %s: %s" % (residency, json.dumps(row)))
        del b
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

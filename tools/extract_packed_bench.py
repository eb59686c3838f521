#!/usr/bin/env python3
"""The text of ranges and lines in one packed array — fmx_extract_packed_batch / fmx_line_text_batch (lanes per PIECE of about
one sample interval, memory by the sum of the lengths) — against the composition it replaces, as a caller ran it before:
fmx_line_bounds_batch + fmx_extract_batch with dst_len = the batch's longest range (ONE lane per range, n x dst_len rows).
The composition's code is untouched by the packed form, so both run in one process on one index (the log text of bench.py,
2^--text-log2 characters, sampleRate 32, the default residency, line table for '\\n'), alternated.

Legs:
  a. 100,000 random lines.
  b. the lines of one frequent pattern (match_lines of the most frequent 4-character string without a newline, at most
     --max-lines of them).
  c. ONE range of 2^--range-log2 characters (the composition as a batch of one: a single lane walks it).
Per leg and route two times:
  host_ms    the host-synchronous call over host arrays (time.perf_counter around it; for the composition line_bounds +
             extract_batch, ids to rows);
  kernel_ms  device events around the device forms over device buffers that are allocated beforehand — the packed fill
             (fmx_extract_packed_fill_dev: fill + redo launch) and k_extract (fmx_extract_batch_dev).
Two untimed calls first, the two routes ALTERNATED --repeats times (the composition of leg c: one untimed call, --slow-repeats
timed ones — a call is a walk of 2^24 dependent steps); median, min and max; a comparison holds when the slower route's min is
above the faster route's max.  Before anything is timed the packed answer of EVERY leg is compared, character for character, with
the composition's rows cut to length.  LF-steps: the composition reports them per range (their sum is what the packed form
executes too, each range's trailing skip paid once; tests/test_extract_packed_cpu.py asserts that against the oracle) — recorded
are the total and the LONGEST CHAIN one lane walks: the longest range's steps there, at most P + sampleRate here.
usage: python tools/extract_packed_bench.py [--text-log2 28] [--repeats 5] [--out profiles/extract_packed.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--range-log2", type=int, default=24)
    ap.add_argument("--lines", type=int, default=100_000)
    ap.add_argument("--max-lines", type=int, default=1 << 19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.slow_repeats >= 3
    import torch

    import index4j_amd as ia
    from index4j_amd import workload
    from locate_all_bench import frequent_strings

    lib = ia.lib
    result = {"text_log2": args.text_log2, "repeats": args.repeats, "slow_repeats": args.slow_repeats, "sample_rate": 32}

    def log(msg):
        print("[extract_packed_bench] " + msg, file=sys.stderr, flush=True)
        if args.out:  # (every leg that is done is on disk)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    def ok(rc, where):
        assert rc == 0, "%s: %s" % (where, (lib.fmx_last_error() or b"").decode())

    def stats(t):
        return {"ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)}

    def timed(calls, repeats, warm):
        """calls: name -> (callable that returns its own milliseconds); alternated"""
        for name, call in calls.items():
            for _ in range(warm[name]):
                call()
        times = {name: [] for name in calls}
        for r in range(max(repeats.values())):
            for name, call in calls.items():
                if r < repeats[name]:
                    times[name].append(call())
        return {name: stats(t) for name, t in times.items()}

    def host_ms(call):
        def run():
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3
        return run

    text = workload.log_text(args.text_log2)
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    n_lines = fm.build_line_table("\n")
    result["lines_of_text"] = int(n_lines)
    P = 32
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dev_i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()

    def kernel_legs(starts, stops, dst_len):
        """the two device forms over buffers made here once; each returns its milliseconds by device events"""
        n = len(starts)
        d_a, d_b = dev_i32(starts), dev_i32(stops)
        text_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        piece_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        st = torch.zeros(n, dtype=torch.int32, device="cuda")
        nbytes = C.c_size_t(0)
        ok(lib.fmx_extract_packed_scratch_bytes(fm.handle, n, C.byref(nbytes)), "scratch_bytes")
        scratch = torch.zeros(nbytes.value, dtype=torch.uint8, device="cuda")
        ok(lib.fmx_extract_packed_offsets_dev(fm.handle, d_a.data_ptr(), d_b.data_ptr(), n, text_off.data_ptr(), piece_off.data_ptr(),
                                              st.data_ptr(), scratch.data_ptr(), nbytes.value, stream), "offsets_dev")
        torch.cuda.synchronize()
        total, pieces = int(text_off[n].item()), int(piece_off[n].item())
        chars = torch.zeros(total + 8, dtype=torch.int16, device="cuda")
        rows = torch.zeros(n * dst_len + 8, dtype=torch.int16, device="cuda")
        out_len, lf, st2 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))

        def events(launch):
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            return run

        def packed():
            ok(lib.fmx_extract_packed_fill_dev(fm.handle, d_a.data_ptr(), d_b.data_ptr(), n, text_off.data_ptr(), piece_off.data_ptr(),
                                               chars.data_ptr(), st.data_ptr(), scratch.data_ptr(), nbytes.value, stream), "fill_dev")

        def composition():
            ok(lib.fmx_extract_batch_dev(fm.handle, d_a.data_ptr(), d_b.data_ptr(), n, rows.data_ptr(), dst_len, 0, out_len.data_ptr(),
                                         lf.data_ptr(), st2.data_ptr(), stream), "extract_batch_dev")

        def redone():
            torch.cuda.synchronize()
            return int(scratch[:4].cpu().numpy().view(np.int32)[0])

        return events(packed), events(composition), pieces, redone

    def leg(name, ids=None, ranges=None, slow=False):
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            starts, stops = fm.line_bounds(ids)
            new = lambda: fm.line_text_batch(ids)
            old = lambda: fm.extract_batch(*fm.line_bounds(ids), dst_len, want_steps=True)
        else:
            starts, stops = (np.ascontiguousarray(x, np.int32) for x in ranges)
            new = lambda: fm.extract_packed_batch(starts, stops)
            old = lambda: fm.extract_batch(starts, stops, dst_len, want_steps=True)
        n = len(starts)
        lens = (stops.astype(np.int64) - starts).clip(min=0)
        dst_len = int(lens.max())
        # the answers first: character for character
        chars, text_off, st = new()
        rows, out_len, st_old, lf = old()
        assert (st == 0).all() and (st_old == 0).all() and (np.diff(text_off) == lens).all() and (out_len == lens).all()
        keep = np.arange(dst_len)[None, :] < lens[:, None]
        assert (chars == rows[keep]).all(), name
        del keep
        k_new, k_old, pieces, redone = kernel_legs(starts, stops, dst_len)
        rep = {"packed": args.repeats, "composition": args.slow_repeats if slow else args.repeats}
        warm = {"packed": 2, "composition": 1 if slow else 2}
        host = timed({"packed": host_ms(new), "composition": host_ms(old)}, rep, warm)
        kern = timed({"packed": k_new, "composition": k_old}, rep, warm)
        row = {"ranges": n, "characters": int(lens.sum()), "longest_range": dst_len, "pieces": pieces, "ranges_redone": redone(),
               "bytes_of_answer_packed": int(lens.sum()) * 2 + (n + 1) * 8, "bytes_of_answer_composition": n * dst_len * 2,
               "lf_steps_total": int(lf.astype(np.int64).sum()), "longest_chain_composition": int(lf.max()), "longest_chain_packed_at_most": P + 32,
               "host_ms": host, "kernel_ms": kern}
        for kind, t in (("host", host), ("kernel", kern)):
            a, b = t["composition"], t["packed"]
            row["%s_ratio_composition_over_packed" % kind] = a["ms"] / b["ms"]
            row["%s_packed_faster_by_more_than_the_spread" % kind] = bool(a["min_ms"] > b["max_ms"])
            row["%s_composition_faster_by_more_than_the_spread" % kind] = bool(b["min_ms"] > a["max_ms"])
        result[name] = row
        log("%s: %s" % (name, json.dumps(row)))

    rng = np.random.default_rng(7)
    leg("a_random_lines", ids=rng.integers(0, n_lines, args.lines))
    strings, counts = frequent_strings(ia.as_chars(text), fm, ia)
    four = [(c, s) for s, c in zip(strings, counts) if len(s) == 4 and 10 not in s.tolist()]
    assert four
    count, pattern = max(four, key=lambda x: x[0])
    ids = fm.match_lines(pattern, args.max_lines)
    result["pattern"] = {"string": ia.chars_to_str(pattern), "count": int(count), "lines_taken": int(len(ids)), "max_lines": args.max_lines}
    leg("b_lines_of_a_pattern", ids=ids)
    span = 1 << args.range_log2
    first = (len(text) - span) // 2 + 5  # (neither end on a sample)
    leg("c_one_long_range", ranges=([first], [first + span]), slow=True)
    fm.close()
    log("done")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

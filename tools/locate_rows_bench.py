#!/usr/bin/env python3
"""locate() with and without the row table (option "locate_rows"), one process, one resident index per setting.

Legs (each a replica of the same image on GPU 0, grown under its options): the walk — `locate_rows` 0 with the default directory
rule (flat at 256 MiB) and with `window_cells` 1 — and the gather — `locate_rows` 1 with each of those and with `window_cells` 0;
the gather also with the walk-order stage kept in front (`rows_order` 1).  Shapes: configs[2] (100,000 8-char patterns, maxMatches 16,
the 256 MiB log, sampleRate 32); locate(1) and locate(100) of the reference-shaped series (8..31-char substrings of the
1,099-symbol text); with --segments N the configs[4] single-GPU share (N segment indexes, fmx_locate_segments_dev).
Timing: HIP events around `--batches` calls per leg (operands in HBM), the legs ALTERNATED `--rounds` times in the same call, the
median round per leg; the first leg runs twice ("walk/default" and "walk/default again"): their difference is the spread a
comparison has to clear twice.  Outputs of every leg are compared with the first leg's at the timed size.  Fill time of a table =
seconds a replica with the option takes to become resident minus the same without.
usage: python tools/locate_rows_bench.py [--text-log2 28] [--batches 50] [--rounds 5] [--segments 0] [--out FILE]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = (("walk/default", {"locate_rows": 0}, {}), ("walk/cells", {"locate_rows": 0, "window_cells": 1}, {}),
        ("rows/default", {"locate_rows": 1}, {}), ("rows/cells", {"locate_rows": 1, "window_cells": 1}, {}),
        ("rows/none", {"locate_rows": 1, "window_cells": 0}, {}), ("rows/default ordered", {"locate_rows": 1}, {"rows_order": 1}))
DEFAULTS = {"locate_rows": 0, "window_cells": 2, "rows_order": 0}


@contextlib.contextmanager
def options(ia, **kw):
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
        yield
    finally:
        for k in kw:
            ia.lib.fmx_set_option(k.encode(), ia._lib.ENV_OPTIONS.get(k, DEFAULTS[k]))


def rows_info(ia, h):
    b, r = C.c_int64(0), C.c_int64(0)
    assert ia.lib.fmx_locate_rows_info(h, C.byref(b), C.byref(r)) == 0
    return b.value, r.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-log2", type=int, default=28)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--segments", type=int, default=0, help="also the configs[4] share over this many segment indexes")
    ap.add_argument("--skip-series", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import index4j_amd as ia
    from index4j_amd import workload

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    result = {"text_log2": args.text_log2, "batches": args.batches, "rounds": args.rounds, "shapes": {}, "tables": {}}

    def log(msg):
        print("[locate_rows_bench] " + msg, file=sys.stderr, flush=True)

    def replicas(fm, name):
        """a replica per leg; records bytes, replay rows and the seconds the table's fill added"""
        out, seconds = {}, {}
        for leg, opts, _ in LEGS:
            if leg in out or leg.endswith(" ordered"):
                continue
            with options(ia, **opts):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rs = ia.ReplicaSet(fm, [0])
                torch.cuda.synchronize()
                seconds[leg] = time.perf_counter() - t0
            out[leg] = rs
            nbytes, replay = rows_info(ia, rs.handles[0])
            assert (nbytes > 0) == bool(opts["locate_rows"]), leg
            result["tables"]["%s %s" % (name, leg)] = {"resident_s": seconds[leg], "rows_bytes": nbytes, "replay_rows": replay,
                                                      "resident_bytes": rs.resident_bytes()[0]}
        out["rows/default ordered"] = out["rows/default"]
        for a, b in (("rows/default", "walk/default"), ("rows/cells", "walk/cells")):
            result["tables"]["%s %s" % (name, a)]["fill_s"] = seconds[a] - seconds[b]
        return out

    def measure(shape, reps, pat, off, mm):
        n = len(off) - 1
        d_pat = torch.from_numpy(np.ascontiguousarray(pat).view(np.int16)).to(dev)
        d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int32)).to(dev)
        bufs = {}
        order = [("walk/default again", {}, {})] + list(LEGS)
        order[0], order[1] = order[1], order[0]  # walk/default, walk/default again, ...
        calls = {}
        for leg, _, run_opts in order:
            rs = reps["walk/default" if leg == "walk/default again" else leg]
            h = rs.handles[0]
            b = [torch.full((n * mm,), -1, dtype=torch.int32, device=dev)] + [torch.zeros(k, dtype=torch.int32, device=dev) for k in (n, n, n, 2 * n)]
            bufs[leg] = b

            def call(h=h, b=b, run_opts=run_opts):
                for k, v in run_opts.items():
                    ia.lib.fmx_set_option(k.encode(), v)
                b[2].zero_()
                rc = ia.lib.fmx_locate_batch_dev(h, d_pat.data_ptr(), d_off.data_ptr(), n, mm, b[0].data_ptr(), mm, b[1].data_ptr(),
                                                 b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr(), sp)
                for k in run_opts:
                    ia.lib.fmx_set_option(k.encode(), DEFAULTS[k])
                assert rc == 0, ia.lib.fmx_last_error()

            calls[leg] = call
            call()
            call()  # warm: scratch sized, code loaded
        torch.cuda.synchronize()
        first = [x.cpu().numpy() for x in bufs["walk/default"][:4]]
        for leg in calls:
            for x, y, what in zip(bufs[leg][:4], first, ("locs", "found", "lf_steps", "status")):
                assert (x.cpu().numpy() == y).all(), "%s: %s of leg %r differs from the walk's" % (shape, what, leg)
        times = {leg: [] for leg in calls}
        for _ in range(args.rounds):
            for leg, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.batches):
                    call()
                e1.record(stream)
                torch.cuda.synchronize()
                times[leg].append(e0.elapsed_time(e1) / args.batches)
        row = {leg: {"ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for leg, t in times.items()}
        spread = abs(row["walk/default"]["ms"] - row["walk/default again"]["ms"])
        best_walk = min(row[k]["ms"] for k in ("walk/default", "walk/default again", "walk/cells"))
        best_rows = min(row[k]["ms"] for k in row if k.startswith("rows/"))
        row["_summary"] = {"patterns": n, "max_matches": mm, "hits": int(first[1].sum()), "lf_steps": int(first[2].astype(np.int64).sum()),
                           "spread_ms": spread, "best_walk_ms": best_walk, "best_rows_ms": best_rows,
                           "rows_beat_walk_by_more_than_twice_the_spread": bool(best_walk - best_rows > 2 * spread)}
        result["shapes"][shape] = row
        log("%s: %s" % (shape, json.dumps(row["_summary"])))

    # configs[2]
    text = workload.log_text(args.text_log2)
    fm = ia.FmIndex(text, 32, True, device=0, build_device=0)
    reps = replicas(fm, "log")
    pat, off, _ = workload.count_batch_patterns(text, 100_000, 8)
    measure("configs[2]", reps, pat, off, 16)
    for rs in set(reps.values()):
        rs.close()
    fm.close()
    del text
    if not args.skip_series:  # the reference-shaped series at sampleRate 32
        rtext = workload.reference_text(args.text_log2, 1099)
        fm = ia.FmIndex(rtext, 32, True, device=0, build_device=0)
        reps = replicas(fm, "series")
        Q = 1 << 20
        pat, off, _ = workload.reference_queries(rtext, Q)
        measure("series locate(1) s=32", reps, pat, off, 1)
        q = Q // 4
        measure("series locate(100) s=32", reps, pat[: off[q]], off[: q + 1], 100)
        for rs in set(reps.values()):
            rs.close()
        fm.close()
        del rtext
    if args.segments:  # configs[4], one GPU's share: tools/bench_segments.py's set-up, the set made resident per setting
        K = args.segments
        texts = workload.segment_texts(K, args.text_log2)
        fms = [ia.FmIndex(t, 32, True, device=None, build_device=0) for t in texts]
        bases = workload.segment_bases(texts)
        n, M = 1 << 20, 16
        pat, off = workload.segment_patterns(texts, n, 8)
        d_pat = torch.from_numpy(pat.view(np.int16)).to(dev)
        d_off = torch.from_numpy(off).to(dev)
        row, firsts = {}, None
        for leg, opts in (("walk/default", {"locate_rows": 0}), ("rows/default", {"locate_rows": 1}), ("walk/default again", {"locate_rows": 0})):
            with options(ia, **opts):
                t0 = time.perf_counter()
                for f in fms:
                    f.to_device(0)
                torch.cuda.synchronize()
                resident_s = time.perf_counter() - t0
            sf = ia.SegmentedFmIndex.from_segments(fms, bases)
            d_tmp = torch.zeros(n * (4 + M), dtype=torch.int32, device=dev)
            d_locs = torch.full((n * M,), -1, dtype=torch.int64, device=dev)
            d_found, d_st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

            def call():
                rc = ia.lib.fmx_locate_segments_dev(sf.handles, K, sf.base_array.ctypes.data, d_pat.data_ptr(), d_off.data_ptr(), n, M,
                                                    d_locs.data_ptr(), d_found.data_ptr(), d_st.data_ptr(), d_tmp.data_ptr(), sp)
                assert rc == 0, ia.lib.fmx_last_error()

            call()
            call()
            torch.cuda.synchronize()
            got = [x.cpu().numpy() for x in (d_locs, d_found, d_st)]
            if firsts is None:
                firsts = got
            assert all((a == b).all() for a, b in zip(got, firsts)), "segments: leg %r differs from the walk's" % leg
            t = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(max(1, args.batches // 5)):
                    call()
                e1.record(stream)
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1) / max(1, args.batches // 5))
            row[leg] = {"ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "resident_s": resident_s,
                        "rows_bytes": sum(f.locate_rows_info()[0] for f in fms)}
        row["_summary"] = {"patterns": n, "max_matches": M, "segments": K, "hits": int(firsts[1].sum()),
                           "spread_ms": abs(row["walk/default"]["ms"] - row["walk/default again"]["ms"])}
        result["shapes"]["configs[4] share, locate"] = row
        log("segments: %s" % json.dumps(row))
        for f in fms:
            f.close()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

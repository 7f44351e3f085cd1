#!/usr/bin/env python3
"""Edge-load pass (Context.edge_load) beside the windowed table
(Context.edge_windows) on the same set in the same process: SN synthetic
traces resident in HBM, start times from fill_start_synthetic over T = 4096
windows of 1 s (the set-up of scripts/bench_edge_windows.py), aggregated once
so the set holds its parent rows.

Per leg one warm-up call, then the median of REPS (10) calls of the stage
timers (hipEvents on the ctx stream):

  windowed     stage 9 (key walk + window kernel) and stage 10 (the kernel)
  load rows    stage 11 (memset + stream kernel + scan), 12 (the stream
               kernel: 18 B/span), 13 (the scan alone)
  load keys    the same with ANOMOD_PARENT_ROWS=0: stage 11 then holds the key
               walk (24 B read + 8 written) and the stream reads 16 B/span
  load tile=0  the rows form with ANOMOD_EDGE_LOAD_TILE=0 (every partial to
               global atomics)
  load 250 us  the rows form with T windows of 250 us from t0: nearly the
               whole set is outside, and the spans inside cover several
               windows each (tail partials and difference-table adds)

Also printed: wall ms per call (tables downloaded) of both calls.

  python scripts/experiments/time_edge_load.py [--lg 24] [--windows 4096] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"), str(ROOT)]

import anomod  # noqa: E402
from anomod import _lib as L  # noqa: E402

T0_US = 1_762_000_000_000_000
STEP_US = 1_000_000
HBM_BYTES_PER_S = 8e12


def med(fn, stages, ctx, reps):
    fn()  # warm-up (allocates the scratch)
    cols = {s: [] for s in stages}
    wall = []
    for _ in range(reps):
        ctx.synchronize()
        t = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t) * 1e3)
        for s in stages:
            cols[s].append(ctx.stage_ms(s))
    return out, {s: statistics.median(v) for s, v in cols.items()}, statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    T = a.windows
    spec = anomod.SynthSpec("SN", seed=20251103, p_orphan_ppm=100)
    rows = []
    for k in ("ANOMOD_PARENT_ROWS", "ANOMOD_EDGE_LOAD_TILE", "ANOMOD_EDGE_LOAD_WGS"):
        os.environ.pop(k, None)
    with anomod.Context(0) as ctx:
        dev = ctx.generate(spec, 1 << a.lg)
        dev.fill_start_synthetic(T0_US, T * STEP_US, 50)
        table = ctx.edge_aggregate(dev, with_hist=False)   # fills the parent rows
        n = dev.n_spans

        win, ms, wall = med(lambda: ctx.edge_windows(dev, T0_US, STEP_US, T),
                            (L.STAGE_EDGE_WINDOWS, L.STAGE_EDGE_WINDOW_KERNEL), ctx, a.reps)
        rows.append({"leg": "windowed table", "spans": n, "pass_ms": ms[L.STAGE_EDGE_WINDOWS],
                     "kernel_ms": ms[L.STAGE_EDGE_WINDOW_KERNEL], "scan_ms": None,
                     "bytes_per_span": 52, "wall_ms": wall})
        print(json.dumps(rows[-1]), flush=True)

        def load_leg(name, env, bytes_per_span, t0=T0_US, step=STEP_US):
            for k, v in env.items():
                os.environ[k] = v
            got, ms, wall = med(lambda: ctx.edge_load(dev, t0, step, T),
                                (L.STAGE_EDGE_LOAD, L.STAGE_EDGE_LOAD_KERNEL,
                                 L.STAGE_EDGE_LOAD_SCAN), ctx, a.reps)
            for k in env:
                os.environ.pop(k, None)
            rows.append({"leg": name, "spans": n, "pass_ms": ms[L.STAGE_EDGE_LOAD],
                         "kernel_ms": ms[L.STAGE_EDGE_LOAD_KERNEL],
                         "scan_ms": ms[L.STAGE_EDGE_LOAD_SCAN],
                         "bytes_per_span": bytes_per_span, "wall_ms": wall,
                         "outside": got.outside, "carried": int(got.carried.sum())})
            print(json.dumps(rows[-1]), flush=True)
            return got

        r = load_leg("load, rows form", {}, 18)
        k = load_leg("load, keys form", {"ANOMOD_PARENT_ROWS": "0"}, 48)
        g = load_leg("load, rows form, tile off", {"ANOMOD_EDGE_LOAD_TILE": "0"}, 18)
        for other in (k, g):
            assert np.array_equal(r.busy_us, other.busy_us) and np.array_equal(r.carried, other.carried)
        # (the last traces' spans reach past the range: clipped, so <=)
        assert (r.busy_us.sum(axis=0) <= table.sum_us).all() and r.busy_us.sum() > 0
        load_leg("load, rows form, 250 us windows", {}, 18, step=250)
        dev.free()
    print("| leg | spans | pass ms | stream kernel ms | scan ms | B/span | pass vs 8 TB/s | "
          "wall ms (with download) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        frac = r["bytes_per_span"] * r["spans"] / (r["pass_ms"] * 1e-3) / HBM_BYTES_PER_S
        scan = "" if r["scan_ms"] is None else f"{r['scan_ms']:.3f}"
        print(f"| {r['leg']} | {r['spans']} | {r['pass_ms']:.3f} | {r['kernel_ms']:.3f} | {scan} | "
              f"{r['bytes_per_span']} | {frac:.3f} | {r['wall_ms']:.2f} |")


if __name__ == "__main__":
    main()

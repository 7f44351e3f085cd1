#!/usr/bin/env python3
"""Edge-window pass on one GPU (a tool, not part of bench.py): SN synthetic
traces with synthetic start times over T windows, time-ordered (2^lg traces,
fill_start_synthetic) and with every trace at a random time (2^lg_random
traces, set_start_us from numpy), each in the LDS sliding-tile form and with
the tile off (ANOMOD_EDGE_WINDOWS_TILE=0: every span to global atomics).

Per leg, warm, the median of `reps` calls: stage 9 (key walk + window kernel),
stage 10 (the window kernel alone), spans/s of stage 9 and the fraction of an
8 TB/s HBM roof that the pass's algorithmic traffic reaches — 52 B/span: 24
read + 8 written by the key walk, 20 read by the window kernel; the 16 B/span
key round trip is the known cost of not fusing the accumulation into the walk.
Stage 0 (the edge aggregation) on the same set is printed for scale.

  python scripts/bench_edge_windows.py [--lg 24] [--lg-random 22] [--windows 4096] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"), str(ROOT)]

import anomod  # noqa: E402
from anomod import _lib as L  # noqa: E402

T0_US = 1_762_000_000_000_000
STEP_US = 1_000_000
BYTES_PER_SPAN = 52
HBM_BYTES_PER_S = 8e12


def leg(ctx, dev, name, n_windows, reps, tile):
    if tile is None:
        os.environ.pop("ANOMOD_EDGE_WINDOWS_TILE", None)
    else:
        os.environ["ANOMOD_EDGE_WINDOWS_TILE"] = tile
    win = ctx.edge_windows(dev, T0_US, STEP_US, n_windows)  # warm-up (allocates the scratch)
    s9, s10 = [], []
    for _ in range(reps):
        win = ctx.edge_windows(dev, T0_US, STEP_US, n_windows)
        s9.append(ctx.stage_ms(L.STAGE_EDGE_WINDOWS))
        s10.append(ctx.stage_ms(L.STAGE_EDGE_WINDOW_KERNEL))
    ms9, ms10 = statistics.median(s9), statistics.median(s10)
    out = {"leg": name, "form": "tile" if tile is None else f"tile<={tile}", "spans": dev.n_spans,
           "windows": n_windows, "stage9_ms": round(ms9, 3), "window_kernel_ms": round(ms10, 3),
           "gspans_per_s": round(dev.n_spans / ms9 / 1e6, 2),
           "hbm_fraction": round(BYTES_PER_SPAN * dev.n_spans / (ms9 * 1e-3) / HBM_BYTES_PER_S, 3),
           "counted": int(win.count.sum()), "outside": win.outside}
    print(json.dumps(out), flush=True)
    return out, win


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--lg-random", type=int, default=22)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    spec = anomod.SynthSpec("SN", seed=20251103, p_orphan_ppm=100)
    period = a.windows * STEP_US
    rows = []
    with anomod.Context(0) as ctx:
        dev = ctx.generate(spec, 1 << a.lg)
        dev.fill_start_synthetic(T0_US, period, 50)
        ctx.edge_aggregate(dev, with_hist=True)
        agg = []
        for _ in range(3):
            ctx.edge_aggregate(dev, with_hist=True)
            agg.append(ctx.stage_ms(L.STAGE_EDGE_AGG))
        print(json.dumps({"leg": "edge_aggregate", "spans": dev.n_spans,
                          "stage0_ms": round(statistics.median(agg), 3)}), flush=True)
        tables = []
        for tile in (None, "0"):
            r, win = leg(ctx, dev, "time-ordered", a.windows, a.reps, tile)
            rows.append(r)
            tables.append(win)
        assert all(np.array_equal(getattr(tables[0], k), getattr(tables[1], k))
                   for k in ("count", "errors", "sum_us", "max_us")), "forms disagree"
        dev.free()

        dev = ctx.generate(spec, 1 << a.lg_random)
        ptr = dev.download().trace_ptr
        lens = np.diff(ptr).astype(np.int64)
        rng = np.random.default_rng(1)
        start = np.repeat(rng.integers(0, period - 1000, dev.n_traces).astype(np.uint64), lens)
        start += np.uint64(T0_US) + (np.arange(dev.n_spans, dtype=np.uint64)
                                     - np.repeat(ptr[:-1], lens)) * np.uint64(50)
        dev.set_start_us(start)
        tables = []
        for tile in (None, "0"):
            r, win = leg(ctx, dev, "random trace times", a.windows, a.reps, tile)
            rows.append(r)
            tables.append(win)
        assert all(np.array_equal(getattr(tables[0], k), getattr(tables[1], k))
                   for k in ("count", "errors", "sum_us", "max_us")), "forms disagree"
        dev.free()
    print("| leg | form | spans | stage 9 ms | window kernel ms | Gspans/s | 52 B/span vs 8 TB/s |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['leg']} | {r['form']} | {r['spans']} | {r['stage9_ms']} | "
              f"{r['window_kernel_ms']} | {r['gspans_per_s']} | {r['hbm_fraction']} |")


if __name__ == "__main__":
    main()

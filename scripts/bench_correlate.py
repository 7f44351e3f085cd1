#!/usr/bin/env python3
"""Series correlation on one GPU (a tool, not part of bench.py): a resident
synthetic matrix (fill_synthetic, S series x T steps, 4 B/sample), correlated
against K = 1 and K = 8 random targets, with the EWMA/z kernel on the same
matrix beside it — both read exactly the same bytes once, so EWMA/z is the
yardstick.  Per leg, warm, the median (min-max) of `reps` calls of the kernel's
stage time and the GB/s of the matrix read (4 S T bytes; EWMA/z also writes
4 S T / W).  The matrix is read in the layout it was created in: tiles
(ANOMOD_EWMA_MODE=1, what S = 10^5 gets by default) and rows (=3).

  python scripts/bench_correlate.py [--series 100000] [--steps 16384] [--window 64] [--reps 7]
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


def timed(call, stage_ms, reps):
    call()  # warm-up
    ms = []
    for _ in range(reps):
        call()
        ms.append(stage_ms())
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=1 << 14)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    S, T = a.series, a.steps
    nbytes = 4.0 * S * T
    rng = np.random.default_rng(3)
    Y = (100 + rng.standard_normal((T, 8))).astype(np.float32)
    rows = []
    with anomod.Context(0) as ctx:
        for layout, mode in (("tiles", "1"), ("rows", "3")):
            os.environ["ANOMOD_EWMA_MODE"] = mode
            ser = anomod.DeviceSeries(ctx, T, S)
            ser.fill_synthetic(7)
            legs = [("ewma_z", lambda: ser.ewma_z(2.0 / (a.window + 1), a.window, download=False),
                     L.STAGE_EWMA)]
            for K in (1, 8):
                legs.append((f"correlate K={K}", lambda K=K: ser.correlate(Y[:, :K], 3),
                             L.STAGE_SERIES_CORR))
            for name, call, stage in legs:
                med, lo, hi = timed(call, lambda: ctx.stage_ms(stage), a.reps)
                r = {"leg": name, "layout": layout, "series": S, "steps": T,
                     "gbytes": round(nbytes / 1e9, 2), "ms": round(med, 3),
                     "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                     "gb_per_s": round(nbytes / med / 1e6, 1)}
                print(json.dumps(r), flush=True)
                rows.append(r)
            r8, n8 = ser.correlate(Y, 3)
            assert (n8 == T).all() and np.isfinite(r8).all() and np.abs(r8).max() < 0.2
            ser.free()
    print("| kernel | layout | ms (min-max) | GB/s |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['leg']} | {r['layout']} | {r['ms']} ({r['ms_min']}-{r['ms_max']}) | "
              f"{r['gb_per_s']} |")


if __name__ == "__main__":
    main()

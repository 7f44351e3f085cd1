#!/usr/bin/env python3
"""Wall time per call of Context.edge_window_quantiles on generated SN traces
resident in HBM (default 2^24; EWQ_TRACES overrides) with a synthetic start
column, 64 windows, q_pct = (50, 99): one warm-up and five calls, each timed
between two ctx.synchronize(); in the same process the same for
Context.edge_windows (the same pass 1 and window rule) and
Context.edge_quantiles_exact (the same pass 1 and radix sort over 32 + 8 key
bits against 32 + 14 here) on the same set.  A last call of each sorting path
with ANOMOD_LOG_KERNEL=1 makes the library print the digit passes its sort ran
(stderr).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python3 ...` in a run of its own."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"), str(ROOT)]
import numpy as np  # noqa: E402

import anomod  # noqa: E402

CALLS = 5
WINDOWS = 64
Q_PCT = (50, 99)
T0_US = 1_700_000_000_000_000


def timed(ctx, fn):
    fn()  # warm-up
    ms = []
    for _ in range(CALLS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


traces = int(os.environ.get("EWQ_TRACES", 1 << 24))
with anomod.Context(0) as ctx:
    sp = ctx.generate(anomod.SynthSpec("SN", seed=20251103, p_orphan_ppm=100,
                                       fault_service="home-timeline-service"), traces)
    period_us = 600 * 1_000_000
    sp.fill_start_synthetic(T0_US, period_us, 50)
    ctx.edge_aggregate(sp, with_hist=False)   # settles the set's hints
    step_us = period_us // WINDOWS + 1
    out = {"spans": sp.n_spans, "traces": sp.n_traces, "calls": CALLS, "windows": WINDOWS,
           "q_pct": list(Q_PCT)}
    runs = {
        "edge_window_quantiles": lambda: ctx.edge_window_quantiles(
            sp, T0_US, step_us, WINDOWS, q_pct=Q_PCT, with_table=False),
        "edge_windows": lambda: ctx.edge_windows(sp, T0_US, step_us, WINDOWS),
        "edge_quantiles_exact": lambda: ctx.edge_quantiles_exact(sp, Q_PCT),
    }
    for name, fn in runs.items():
        ms = timed(ctx, fn)
        out[name + "_wall_ms"] = [round(x, 3) for x in ms]
        out[name + "_wall_ms_median"] = round(float(np.median(ms)), 3)
    out["window_quantiles_over_exact"] = round(
        out["edge_window_quantiles_wall_ms_median"] / out["edge_quantiles_exact_wall_ms_median"], 3)
    out["window_quantiles_over_edge_windows"] = round(
        out["edge_window_quantiles_wall_ms_median"] / out["edge_windows_wall_ms_median"], 3)
    got = runs["edge_window_quantiles"]()
    out["outside"] = got.outside
    out["non_empty_cells"] = int(np.count_nonzero(got.q_count))
    os.environ["ANOMOD_LOG_KERNEL"] = "1"
    sys.stderr.flush()
    runs["edge_window_quantiles"]()
    runs["edge_quantiles_exact"]()
    del os.environ["ANOMOD_LOG_KERNEL"]
    print(json.dumps(out), flush=True)
    sp.free()

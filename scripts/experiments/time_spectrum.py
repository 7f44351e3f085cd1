#!/usr/bin/env python3
"""Wall time per call of Context.trace_spectrum on generated SN traces resident
in HBM (default 2^24; SPECTRUM_TRACES overrides), one warm-up and five calls,
each timed between two ctx.synchronize(); in the same process the same for
Context.edge_windows on the same set with a synthetic start column (the same
pass 1; its pass 2 reads 20 B / span against 12 here).  A last call with
ANOMOD_LOG_KERNEL=1 makes the library print what its per-call workspace cost
to allocate and to free (stderr).  Kernel times: run this under
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


traces = int(os.environ.get("SPECTRUM_TRACES", 1 << 24))
with anomod.Context(0) as ctx:
    sp = ctx.generate(anomod.SynthSpec("SN", seed=20251103, p_orphan_ppm=100,
                                       fault_service="home-timeline-service"), traces)
    period_us = 600 * 1_000_000
    sp.fill_start_synthetic(1_700_000_000_000_000, period_us, 50)
    table = ctx.edge_aggregate(sp, with_hist=True)   # (also settles the set's hints)
    thr = anomod.spectrum_thresholds(table, sp.services, rows="root")
    step_us = period_us // WINDOWS + 1
    out = {"spans": sp.n_spans, "traces": sp.n_traces, "calls": CALLS}
    runs = {
        "trace_spectrum": lambda: ctx.trace_spectrum(sp, thr, True),
        "trace_spectrum_no_class_column": lambda: ctx.trace_spectrum(sp, thr, True,
                                                                     per_trace=False),
        "edge_windows": lambda: ctx.edge_windows(sp, 1_700_000_000_000_000, step_us, WINDOWS),
    }
    for name, fn in runs.items():
        ms = timed(ctx, fn)
        out[name + "_wall_ms"] = [round(x, 3) for x in ms]
        out[name + "_wall_ms_median"] = round(float(np.median(ms)), 3)
    got = ctx.trace_spectrum(sp, thr, True)
    out["abnormal_traces"] = int(got.n_traces[1])
    out["spectrum_over_edge_windows"] = round(
        out["trace_spectrum_wall_ms_median"] / out["edge_windows_wall_ms_median"], 3)
    os.environ["ANOMOD_LOG_KERNEL"] = "1"
    sys.stderr.flush()
    ctx.trace_spectrum(sp, thr, True, per_trace=False)
    del os.environ["ANOMOD_LOG_KERNEL"]
    print(json.dumps(out), flush=True)
    sp.free()

#!/usr/bin/env python3
"""Wall time per call of Context.trace_shapes against Context.self_time and
Context.trace_structure(download=False) on the same device-resident set, in
the same process: one warm-up and seven calls each, timed between two
ctx.synchronize(), median reported.  The inputs are host-generated SN, TT and
LONG traces: 2^20 SN, 2^18 TT and 2^17 LONG traces (TS_SCALE multiplies the
trace counts).  trace_shapes is timed with a cap of 64 shapes and no per-trace
or per-span column (the census alone) and again with both columns (their
download included).  Also printed: the distinct shapes, the share of the
traces in the most common one, and the off-tree spans.  Kernel times: run this
under `rocprofv3 --kernel-trace --stats -- python3 ...` in a run of its own."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"),
                str(ROOT)]
import numpy as np  # noqa: E402

import anomod  # noqa: E402

CALLS = 7
TRACES = {"SN": 1 << 20, "TT": 1 << 18, "LONG": 1 << 17}


def timed(ctx, fn):
    fn()  # warm-up
    ms = []
    for _ in range(CALLS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(x, 3) for x in ms]


scale = float(os.environ.get("TS_SCALE", 1))
with anomod.Context(0) as ctx:
    for topo, n_traces in TRACES.items():
        sp = anomod.synth_generate_host(anomod.SynthSpec(topo, seed=1, p_orphan_ppm=2000),
                                        max(1, int(n_traces * scale)))
        d = ctx.upload(sp)
        ctx.edge_aggregate(d)   # settles the set's hints
        census = ctx.trace_shapes(d, cap=64)
        sh_ms, sh_all = timed(ctx, lambda: ctx.trace_shapes(d, cap=64))
        col_ms, _ = timed(ctx, lambda: ctx.trace_shapes(d, cap=64, per_trace=True,
                                                        per_span=True))
        st_ms, st_all = timed(ctx, lambda: ctx.self_time(d))
        ts_ms, ts_all = timed(ctx, lambda: ctx.trace_structure(d, download=False))
        print(json.dumps({
            "topology": topo, "traces": sp.n_traces, "spans": sp.n_spans,
            "long_traces": int((np.diff(sp.trace_ptr) > 256).sum()),
            "trace_shapes_ms": round(sh_ms, 3), "trace_shapes_columns_ms": round(col_ms, 3),
            "self_time_ms": round(st_ms, 3), "trace_structure_ms": round(ts_ms, 3),
            "vs_self_time": round(sh_ms / st_ms, 3), "vs_trace_structure": round(sh_ms / ts_ms, 3),
            "trace_shapes_all_ms": sh_all, "self_time_all_ms": st_all,
            "trace_structure_all_ms": ts_all,
            "distinct_shapes": census.n_shapes,
            "top_shape_share": round(float(census.count[0]) / max(1, sp.n_traces), 4),
            "off_tree_spans": census.off_tree_spans}), flush=True)
        d.free()

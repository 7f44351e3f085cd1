#!/usr/bin/env python3
"""Wall time per call of Context.critical_path against Context.self_time on the
same device-resident set, in the same process: one warm-up and seven calls
each, timed between two ctx.synchronize(), median reported.  The inputs are
tests/critical_path_ref.nested_set of host-generated SN, TT and LONG traces
(children inside their parents, p_seq = 1/2): 2^20 SN, 2^18 TT and 2^17 LONG
traces, which that helper builds in 10 to 20 seconds each and the reference
pass takes about as long again (CP_SCALE multiplies the trace counts).  Also
printed: the selection rounds the reference counts (the selected children of
one parent: largest and mean over the parents that select any) and the share
of spans on the path.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python3 ...` in a run of its own."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"),
                str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402

import anomod  # noqa: E402
from critical_path_ref import critical_path_ref, nested_set  # noqa: E402
from self_time_ref import parents_ref  # noqa: E402

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


scale = float(os.environ.get("CP_SCALE", 1))
with anomod.Context(0) as ctx:
    for topo, n_traces in TRACES.items():
        t0 = time.perf_counter()
        sp = anomod.synth_generate_host(anomod.SynthSpec(topo, seed=1, p_orphan_ppm=2000),
                                        max(1, int(n_traces * scale)))
        par = parents_ref(sp)
        sp = nested_set(sp, par, 0.5, seed=7)
        build_s = time.perf_counter() - t0
        _, on, nsel = critical_path_ref(sp, par)
        d = ctx.upload(sp)
        ctx.edge_aggregate(d)   # settles the set's hints
        cp_ms, cp_all = timed(ctx, lambda: ctx.critical_path(d))
        st_ms, st_all = timed(ctx, lambda: ctx.self_time(d))
        print(json.dumps({
            "topology": topo, "traces": sp.n_traces, "spans": sp.n_spans,
            "long_traces": int((np.diff(sp.trace_ptr) > 256).sum()),
            "build_s": round(build_s, 1),
            "critical_path_ms": round(cp_ms, 3), "self_time_ms": round(st_ms, 3),
            "ratio": round(cp_ms / st_ms, 3),
            "critical_path_all_ms": cp_all, "self_time_all_ms": st_all,
            "rounds_max": int(nsel.max()),
            "rounds_mean": round(float(nsel[nsel > 0].mean()), 2),
            "on_path_share": round(float(on.mean()), 3)}), flush=True)
        d.free()

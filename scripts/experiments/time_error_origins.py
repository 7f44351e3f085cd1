#!/usr/bin/env python3
"""Wall time per call of Context.error_origins and of Context.self_time on the
same generated set resident in HBM, in the same process: SN 2^20, TT 2^18 and
LONG 2^17 traces (ORIGINS_SCALE divides the counts), each (a) without any
error flag and (b) with the generator's fault errors at 30 % on one service
and its 0.5 % base rate (the generator draws every flag independently: this
measures flag density, not chains).  One warm-up and five calls per process,
each timed between two ctx.synchronize(); ORIGINS_PROCS (3) child processes per
set, and the report is the median of the process medians with their range.

The bar for (a): the pass reads no more bytes per span than self time and
writes no per-span record, so its median must not exceed the slowest process
median of self_time on the same set ("a_within_bar").  Kernel times: run one
child under `rocprofv3 --kernel-trace --stats -- python3 ... --child SN 0` in
a run of its own."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"), str(ROOT)]
import numpy as np  # noqa: E402

CALLS = 5
SETS = {"SN": 1 << 20, "TT": 1 << 18, "LONG": 1 << 17}
FAULT = {"SN": "home-timeline-service", "TT": "ts-order-service", "LONG": "home-timeline-service"}


def timed(ctx, fn):
    fn()  # warm-up
    ms = []
    for _ in range(CALLS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def child(topo: str, flagged: bool) -> None:
    import anomod
    traces = max(1, SETS[topo] // int(os.environ.get("ORIGINS_SCALE", 1)))
    spec = anomod.SynthSpec(topo, seed=20251103, p_orphan_ppm=100, fault_service=FAULT[topo],
                            p_error_ppm=5000 if flagged else 0,
                            p_fault_error_ppm=300000 if flagged else 0)
    with anomod.Context(0) as ctx:
        sp = ctx.generate(spec, traces)
        table = ctx.edge_aggregate(sp, with_hist=False)   # (also settles the set's hints)
        out = {"topo": topo, "flagged": flagged, "spans": sp.n_spans, "traces": sp.n_traces,
               "error_spans": int(table.errors.sum()),
               "error_origins_ms": timed(ctx, lambda: ctx.error_origins(sp)),
               "self_time_ms": timed(ctx, lambda: ctx.self_time(sp, with_hist=False))}
        got = ctx.error_origins(sp)
        assert got.error_spans == out["error_spans"]
        out["origin_spans"] = int(got.origin.sum())
        print(json.dumps(out), flush=True)
        sp.free()


def main() -> None:
    procs = int(os.environ.get("ORIGINS_PROCS", 3))
    rows = []
    for topo in SETS:
        for flagged in (False, True):
            runs = []
            for _ in range(procs):   # one process at a time
                r = subprocess.run([sys.executable, __file__, "--child", topo, str(int(flagged))],
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f"child {topo} {flagged} failed ({r.returncode}):\n{r.stderr}")
                runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            eo = sorted(x["error_origins_ms"] for x in runs)
            st = sorted(x["self_time_ms"] for x in runs)
            row = {"topo": topo, "flagged": flagged, "spans": runs[0]["spans"],
                   "error_spans": runs[0]["error_spans"], "origin_spans": runs[0]["origin_spans"],
                   "error_origins_ms": [round(x, 3) for x in eo],
                   "error_origins_ms_median": round(float(np.median(eo)), 3),
                   "self_time_ms": [round(x, 3) for x in st],
                   "self_time_ms_median": round(float(np.median(st)), 3)}
            if not flagged:
                row["a_within_bar"] = bool(np.median(eo) <= st[-1])
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"calls": CALLS, "procs": procs, "rows": rows}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3] == "1")
    else:
        main()

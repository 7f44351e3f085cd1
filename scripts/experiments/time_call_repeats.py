#!/usr/bin/env python3
"""Wall time per call of Context.call_repeats — untimed, then with a start
column generated on the device — and of Context.self_time(with_hist=False) and
Context.error_origins on the same generated set resident in HBM, in the same
process: SN 2^20, TT 2^18 and LONG 2^17 traces (REPEATS_SCALE divides the
counts), with the generator's 0.5 % base error rate and 30 % on one service.
One warm-up and five calls per process, each timed between two
ctx.synchronize(); REPEATS_PROCS (3) child processes per set, and the report
is the median of the process medians with their range.

The bar, for the untimed form on SN and TT: the pass does two LDS scans per
span where self time does one and writes no 8 B/span record, so its median
must not exceed 1.5 x the slowest process median of self_time(with_hist=False)
on the same set ("within_bar").  The timed form and LONG have none.  Kernel
times: run one child under `rocprofv3 --kernel-trace --stats -- python3 ...
--child SN` in a run of its own."""
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
BAR = 1.5
KEYS = ("call_repeats_ms", "call_repeats_timed_ms", "self_time_ms", "error_origins_ms")


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


def child(topo: str) -> None:
    import anomod
    traces = max(1, SETS[topo] // int(os.environ.get("REPEATS_SCALE", 1)))
    spec = anomod.SynthSpec(topo, seed=20251103, p_orphan_ppm=100, fault_service=FAULT[topo],
                            p_error_ppm=5000, p_fault_error_ppm=300000)
    with anomod.Context(0) as ctx:
        sp = ctx.generate(spec, traces)
        table = ctx.edge_aggregate(sp, with_hist=False)   # (also settles the set's hints)
        out = {"topo": topo, "spans": sp.n_spans, "traces": sp.n_traces,
               "call_repeats_ms": timed(ctx, lambda: ctx.call_repeats(sp)),
               "self_time_ms": timed(ctx, lambda: ctx.self_time(sp, with_hist=False)),
               "error_origins_ms": timed(ctx, lambda: ctx.error_origins(sp))}
        got = ctx.call_repeats(sp)
        S = len(sp.services)
        assert not got.timed
        assert np.array_equal((got.groups + got.repeats)[:S * S], table.count[:S * S])
        sp.fill_start_synthetic(1_700_000_000_000_000, 600_000_000, 50)
        out["call_repeats_timed_ms"] = timed(ctx, lambda: ctx.call_repeats(sp))
        later = ctx.call_repeats(sp)
        assert later.timed and np.array_equal(later.groups, got.groups)
        out.update(groups=int(got.groups.sum()), repeats=int(got.repeats.sum()),
                   retried=int(got.retried.sum()), max_size=int(got.max_size),
                   after_error=int(later.after_error.sum()))
        print(json.dumps(out), flush=True)
        sp.free()


def main() -> None:
    procs = int(os.environ.get("REPEATS_PROCS", 3))
    rows = []
    for topo in SETS:
        runs = []
        for _ in range(procs):   # one process at a time
            r = subprocess.run([sys.executable, __file__, "--child", topo],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child {topo} failed ({r.returncode}):\n{r.stderr}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = {k: runs[0][k] for k in ("topo", "spans", "traces", "groups", "repeats", "retried",
                                       "max_size", "after_error")}
        for k in KEYS:
            v = sorted(x[k] for x in runs)
            row[k] = [round(x, 3) for x in v]
            row[k + "_median"] = round(float(np.median(v)), 3)
        if topo != "LONG":
            row["within_bar"] = bool(row["call_repeats_ms_median"] <= BAR * row["self_time_ms"][-1])
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"calls": CALLS, "procs": procs, "bar": BAR, "rows": rows}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()

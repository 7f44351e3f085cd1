#!/usr/bin/env python3
"""Stage times of the bench set's calls under the library ANOMOD_LIB points
at: the SocialNetwork set of bench.py (2^lg traces), calls 1-4 (walk + row
streams), call 5 (the transition), then seven warm dense calls; prints one
JSON line with the times and a digest of the last table, so that builds can be
compared for time and for bits.  TD_ERROR_PPM sets the spec's p_error_ppm (0:
an error-free set, which never enters the dense kernel's branch for an error);
TD_LABEL names the line.

  ANOMOD_LIB=... TD_ERROR_PPM=0 python scripts/experiments/time_dense_calls.py 27
"""
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "anomod-a-dataset-for-anomaly-detection-and-root-cause-analysis-in-microservice-systems_amd"), str(ROOT)]

import anomod  # noqa: E402
from anomod import _lib as L  # noqa: E402

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 27
ppm = os.environ.get("TD_ERROR_PPM")
kw = {} if ppm is None else {"p_error_ppm": int(ppm)}
with anomod.Context(0) as ctx:
    dev = ctx.generate(anomod.SynthSpec("SN", seed=20251103, p_orphan_ppm=100, **kw), 1 << lg)
    first, dense = [], []
    for k in range(12):
        t = ctx.edge_aggregate(dev, with_hist=False)
        (first if k < 5 else dense).append(round(ctx.stage_ms(L.STAGE_EDGE_AGG), 4))
    t = ctx.edge_aggregate(dev, with_hist=True)  # (not timed: the digest takes the histogram too)
    h = hashlib.sha256()
    for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist"):
        h.update(getattr(t, k).tobytes())
    print(json.dumps({"label": os.environ.get("TD_LABEL", Path(os.environ.get("ANOMOD_LIB", "libanomod.so")).name),
                      "topo": "SN", "p_error_ppm": ppm, "spans": dev.n_spans, "errors": int(t.errors.sum()),
                      "first5_ms": first, "dense_ms": dense, "min": min(dense), "max": max(dense),
                      "digest": h.hexdigest()[:16]}), flush=True)

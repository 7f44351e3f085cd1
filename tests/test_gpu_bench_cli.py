"""GPU: bench.py's plain run — headline line only — and --dump-outputs: the
edge table of the last timed step, written as float64 .npy columns, equal to
the oracle's table of the same synthetic spans."""
import json
import subprocess
import sys

import numpy as np
import pytest

import anomod
from oracle import native

from conftest import ROOT

pytestmark = pytest.mark.gpu

COLUMNS = ("count", "errors", "sum_us", "min_us", "max_us", "p50_us", "p99_us")


def test_plain_run_headline_only_and_dump_matches_oracle(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--traces-per-gpu", "30000", "--seed", "77", "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    host = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=77, p_orphan_ppm=100), 30000)
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "spans/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(host.n_spans * 3 / (line["ms_per_step"] * 3e-3))
    # nothing but the headline: the legs and CPU baselines need --full
    for key in ("cpu_baseline", "sn_general_scan", "trace_structure", "exact_quantiles",
                "sn_in_trace_shuffled", "ungrouped", "tt_width", "long_traces", "pagerank",
                "ewma", "tt_config2", "tt_config2_files"):
        assert key not in line, key
    ref = native.finalize(native.edge_aggregate(host))
    assert sorted(p.name for p in out.iterdir()) == sorted(f"{k}.npy" for k in COLUMNS)
    for k in COLUMNS:
        a = np.load(out / f"{k}.npy")
        assert a.dtype == np.float64 and np.isfinite(a).all(), k
        want = np.asarray(ref[k], np.float64)
        # an edge without spans has no quantile: NaN in the table, -1 in the file
        np.testing.assert_array_equal(a, np.where(np.isnan(want), -1.0, want), err_msg=k)
    empty = ref["count"] == 0
    assert empty.any() and np.isnan(ref["p50_us"][empty]).all()
    assert (np.load(out / "p50_us.npy")[empty] == -1).all()
    assert int(np.load(out / "count.npy").sum()) == host.n_spans

"""GPU: features(symptom_corr=True) and rank(walk="correlation") on a hand-built
run — entry service a -> b -> c and a -> d, c's latency following a per-window
pattern that b and a contain, d unrelated — against the host models
(edge_windows_ref + series_corr_ref); the metric part on a regular and an
irregular grid; the CLI."""
import json
import shutil
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod.engine import _trace_range
from conftest import PKG_DIR
from edge_windows_ref import edge_windows_ref
from series_corr_ref import BOUND_MAX, correlate_ref

pytestmark = pytest.mark.gpu

SERVICES = ["svc-a", "svc-b", "svc-c", "svc-d"]
A, B, Cc, D = range(4)
T0 = 1_700_000_000_000_000      # epoch microseconds, a multiple of the steps used
STEP_S, N_WIN = 1.0, 40
MIN_COUNT = 5


def build_spans():
    """40 one-second windows of 6 traces (3 in windows 7 and 23: below
    min_count), each a(root) -> b -> c and a -> d.  c lasts 3 ms + 6 ms *
    pattern[w] + jitter, b and a contain it, d is independent of the window."""
    rng = np.random.default_rng(40)
    pattern = rng.random(N_WIN)
    svc, dur, sid, par, start, ptr = [], [], [], [], [], [0]
    for w in range(N_WIN):
        for _ in range(3 if w in (7, 23) else 6):
            t = T0 + w * 1_000_000 + int(rng.integers(0, 500_000))
            c = 3000 + int(6000 * pattern[w]) + int(rng.integers(0, 300))
            b = c + 200 + int(rng.integers(0, 100))
            d = 1000 + int(rng.integers(0, 800))
            a = b + d + 300 + int(rng.integers(0, 100))
            svc += [A, B, Cc, D]
            dur += [a, b, c, d]
            sid += [1, 2, 3, 4]
            par += [0, 1, 2, 1]
            start += [t, t + 100, t + 200, t + 100 + b]
            ptr.append(len(svc))
    n = len(svc)
    sp = anomod.SpanSet(list(SERVICES), np.array(ptr), np.repeat(np.arange(len(ptr) - 1), 4) + 1,
                        np.array(sid), np.array(par), np.array(svc), np.zeros(n), np.array(dur),
                        unique_ids=True, start_us=np.array(start))
    return sp, pattern


def build_metrics(sp, regular=True):
    """30 rows every 2 s from 4 s before the first trace: a copy of the
    front-door series on that grid (svc-c's pod), its negation (svc-b), a
    constant (svc-a), noise (svc-d) and a series of no service."""
    rng = np.random.default_rng(41)
    ts = T0 / 1e6 - 4.0 + 2.0 * np.arange(30)
    if not regular:
        ts[17] += 0.5
    ts_us = np.rint(ts * 1e6).astype(np.int64)
    # rows whose [ts, ts + 2 s) touches the trace starts: 2 .. 21 on the regular grid
    i0, Tm = 2, 20
    ym = edge_windows_ref(sp, int(ts_us[i0]), 2_000_000, Tm).symptom(MIN_COUNT)
    X = rng.standard_normal((30, 5)).astype(np.float32)
    X[i0:i0 + Tm, 0] = np.where(np.isfinite(ym), 3 * ym + 1, 0)
    X[i0:i0 + Tm, 1] = -X[i0:i0 + Tm, 0]
    X[:, 2] = 42.0
    X[5, 3] = np.nan
    keys = [("container_cpu", (("pod", "svc-c-5f7d9"),)), ("container_mem", (("pod", "svc-b-11aa0"),)),
            ("up", (("job", "svc-a"),)), ("container_cpu", (("pod", "svc-d-0c2e4"),)),
            ("node_load1", (("instance", "10.0.0.7:9100"),))]
    return anomod.MetricMatrix(X, ts, keys), (i0, Tm, ym)


@pytest.fixture(scope="module")
def run(ctx):
    sp, pattern = build_spans()
    mm, mref = build_metrics(sp)
    exp = anomod.Experiment("hand_built", sp, mm, "svc-c")
    on = anomod.features(exp, ctx, W=6, trace_step_s=STEP_S, trace_min_count=MIN_COUNT,
                         symptom_corr=True)
    off = anomod.features(exp, ctx, W=6, trace_step_s=STEP_S, trace_min_count=MIN_COUNT)
    return {"sp": sp, "exp": exp, "on": on, "off": off, "mref": mref}


def host_expectation(sp):
    """(keys, model of the columns, per-service max rule) from the host models."""
    t0, step_us, T = _trace_range(sp, STEP_S)
    assert (t0, step_us, T) == (T0, 1_000_000, N_WIN)
    win = edge_windows_ref(sp, t0, step_us, T)
    mm = win.matrix(MIN_COUNT)
    y = win.symptom(MIN_COUNT)
    cols = [j for j, k in enumerate(mm.series) if k[0] != "edge_count"]
    m = correlate_ref(mm.X[:, cols], y, 3)
    keys = [mm.series[j] for j in cols]
    svc = np.zeros(len(SERVICES))
    for key, r in zip(keys, m["r"][0]):
        c = SERVICES.index(dict(key[1])["child"])
        if r > 0:
            svc[c] = max(svc[c], r)
    return y, keys, m, svc


def test_host_models_rank_c_above_d():
    """What the GPU test relies on, from the models alone (no GPU needed, but
    kept beside its user)."""
    sp, _ = build_spans()
    y, keys, m, svc = host_expectation(sp)
    assert np.isnan(y[[7, 23]]).all() and np.isfinite(np.delete(y, [7, 23])).all()
    assert [dict(k[1])["child"] for k in keys] == ["svc-b", "svc-d", "svc-c", "svc-a"]
    assert (m["n"][0] == N_WIN - 2).all() and m["bound"].max() <= BOUND_MAX
    assert svc[Cc] > 0.9 and svc[B] > 0.9 and svc[A] > 0.99 and svc[Cc] > svc[D] + 0.3


def test_trace_columns_within_the_bound(run):
    sc = run["on"].symptom_corr
    y, keys, m, svc = host_expectation(run["sp"])
    np.testing.assert_array_equal(sc.symptom.view(np.uint32), y.view(np.uint32))
    assert sc.keys == keys
    np.testing.assert_array_equal(sc.n, m["n"][0])
    assert not np.isnan(sc.r).any()
    assert (np.abs(sc.r - m["r"][0]) <= m["bound"][0]).all()
    comp = run["on"].params["components"]["symptom_corr"]
    assert comp is sc.service and comp.dtype == np.float64 and comp.shape == (4,)
    # the max rule over the kernel's own r, and the model's within the bound
    want = np.zeros(4)
    for key, r in zip(sc.keys, sc.r):
        c = SERVICES.index(dict(key[1])["child"])
        want[c] = max(want[c], r if r > 0 else 0.0)
    np.testing.assert_array_equal(comp, want)
    assert (np.abs(comp - svc) <= m["bound"].max()).all()
    assert ((comp >= 0) & (comp <= 1)).all() and comp[Cc] > comp[D]
    top = sc.top(3)
    assert len(top) == 3 and abs(top[0]["r"]) >= abs(top[1]["r"]) >= abs(top[2]["r"])


def test_score_and_components_unchanged(run):
    on, off = run["on"], run["off"]
    assert off.symptom_corr is None and "symptom_corr" not in off.params["components"]
    assert "metric_corr_grid" not in off.params
    np.testing.assert_array_equal(on.service_scores.view(np.uint64),
                                  off.service_scores.view(np.uint64))
    for k, v in off.params["components"].items():
        np.testing.assert_array_equal(on.params["components"][k], v, err_msg=k)
    assert set(on.params["components"]) - set(off.params["components"]) == {
        "symptom_corr", "metric_corr"}
    np.testing.assert_array_equal(on.trace_window_scores, off.trace_window_scores)
    np.testing.assert_array_equal(on.window_scores, off.window_scores)


def test_correlation_walk_is_pagerank_on_walk_graph(ctx, run):
    on = run["on"]
    calls = anomod.rank(on, ctx=ctx)
    assert calls == anomod.rank(on, walk="calls", ctx=ctx) == anomod.rank(run["off"], ctx=ctx)
    got = anomod.rank(on, walk="correlation", rho=0.3, ctx=ctx)
    row_ptr, col, w = anomod.walk_graph(on.edges, on.symptom_corr.service, 0.3)
    p = np.asarray(on.service_scores, np.float64)
    p = np.where(np.isfinite(p), p, 0.0)
    if p.sum() <= 0:
        p = np.ones(4)
    p = p + 1e-9 * p.sum()
    x, _ = ctx.pagerank(row_ptr, col, w, p, alpha=0.85, iters=100, tol=1e-10)
    order = np.argsort(-x, kind="stable")
    assert got == [(SERVICES[i], float(x[i])) for i in order]
    assert got != calls
    with pytest.raises(ValueError):
        anomod.rank(run["off"], walk="correlation", ctx=ctx)


def test_metric_matrix_on_a_regular_grid(run):
    on, sc = run["on"], run["on"].symptom_corr
    i0, Tm, ym = run["mref"]
    assert on.params["metric_corr_grid"] == sc.metric_grid == "regular"
    assert sc.metric_rows == (i0, i0 + Tm - 1)
    np.testing.assert_array_equal(sc.metric_symptom.view(np.uint32), ym.view(np.uint32))
    m = correlate_ref(run["exp"].metrics.X[i0:i0 + Tm], ym, 3)
    np.testing.assert_array_equal(sc.metric_n, m["n"][0])
    np.testing.assert_array_equal(np.isnan(sc.metric_r), np.isnan(m["r"][0]))
    have = ~np.isnan(m["r"][0])
    assert m["bound"][0][have].max() <= BOUND_MAX
    assert (np.abs(sc.metric_r - m["r"][0])[have] <= m["bound"][0][have]).all()
    assert sc.metric_keys == run["exp"].metrics.series
    assert abs(sc.metric_r[0] - 1) < 1e-6 and abs(sc.metric_r[1] + 1) < 1e-6   # the copies
    assert np.isnan(sc.metric_r[2]) and sc.metric_n[2] == sc.metric_n[0]       # the constant
    mc = on.params["components"]["metric_corr"]
    want = np.array([0.0, abs(sc.metric_r[1]), abs(sc.metric_r[0]), abs(sc.metric_r[3])])
    np.testing.assert_array_equal(mc, want)      # |r|; the constant and the unmapped series add nothing
    assert abs(sc.top(1)[0]["r"]) >= 1 - 1e-6
    assert {"metric", "trace"} == {t["kind"] for t in sc.top(20)}


def test_metric_matrix_on_an_irregular_grid(ctx, run):
    mm, _ = build_metrics(run["sp"], regular=False)
    exp = anomod.Experiment("hand_built", run["sp"], mm, "svc-c")
    f = anomod.features(exp, ctx, W=6, trace_step_s=STEP_S, trace_min_count=MIN_COUNT,
                        symptom_corr=True)
    sc = f.symptom_corr
    assert f.params["metric_corr_grid"] == sc.metric_grid == "irregular"
    assert "metric_corr" not in f.params["components"]
    assert sc.metric_r is None and sc.metric_service is None and sc.metric_symptom is None
    np.testing.assert_array_equal(sc.r, run["on"].symptom_corr.r)     # the trace part is as before
    exp0 = anomod.Experiment("hand_built", run["sp"], None, "svc-c")
    f0 = anomod.features(exp0, ctx, trace_step_s=STEP_S, trace_min_count=MIN_COUNT,
                         symptom_corr=True)
    assert f0.params["metric_corr_grid"] == "none" and f0.symptom_corr.metric_r is None


def _cli(args):
    return subprocess.run([sys.executable, "-m", "anomod", "features"] + args, cwd=PKG_DIR,
                          capture_output=True, text=True, timeout=300)


def test_cli(golden, tmp_path):
    d = tmp_path / "trace_data" / "Svc_Kill_Media_20251103_230000_traces_2025-11-03_23-10-00"
    d.mkdir(parents=True)
    shutil.copy(golden / "jaeger_small.json", d / "all_traces.json")
    out = tmp_path / "features.json"
    r = _cli([str(d), "--trace-step", "60", "--symptom-corr", "--walk", "correlation",
              "--out", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(out.read_text())
    assert set(doc["symptom_corr"]) == set(doc["services"])
    assert all(0.0 <= v <= 1.0 for v in doc["symptom_corr"].values())
    assert isinstance(doc["symptom_correlates"], list) and len(doc["symptom_correlates"]) <= 10
    for row in doc["symptom_correlates"]:
        assert set(row) == {"kind", "name", "labels", "r", "n"} and -1 <= row["r"] <= 1
    assert len(doc["ranking"]) == len(doc["services"])
    for bad in ([str(d), "--symptom-corr"],
                [str(d), "--trace-step", "60", "--walk", "correlation"]):
        r = _cli(bad)
        assert r.returncode == 2 and "error:" in r.stderr, r.stderr[-500:]

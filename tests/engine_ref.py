"""Plain model of the composition between the kernels' tables and the ranking
(anomod.features / anomod.rank), and a CPU context that lets both run without
a GPU (a plain helper, not a conftest).

The model restates the rules of the docstrings in Python loops over services,
edge rows and columns; it takes tables as arrays (an Inputs record) and
returns every component and the score.

  column score    the mean of a column's top k = max(1, n // 20) window
                  scores.  The trace and load series drop their first window
                  (the EWMA variance starts at 0 there), the metric series
                  keeps it.  A column holding a NaN window scores NaN.  The
                  trace and load means are taken in f64; the metric mean in
                  the precision of the window scores handed over (f32 from
                  the kernels and the C oracle): summed in ascending order,
                  then divided.
  squashing       s(x) = x / (1 + x), s(+inf) = 1; a NaN column score is
                  skipped: it contributes nothing to its service.
  series          a metric series belongs to the service with the longest
                  name contained in one of its label values (the first in
                  service order on ties), to none when no name is contained.
                  A trace / load column belongs to the child service of its
                  edge row (row % S; ROOT and ORPHAN rows included); the
                  columns are those of the active rows in ascending order, 2
                  (3 with a quantile) per row for the trace series, 1 for the
                  load series.  A service takes the max over its columns.
  error term      errors / calls summed over the rows a service is the child
                  of; with error origins the origin spans instead of errors.
  latency term    max over a service's incoming edges of max(0, log2(p99 /
                  baseline p99)), the baseline edge found by the NAMES of
                  parent and child, both sides holding >= min_count calls and
                  finite p99 (baseline > 0); from the critical-path tables
                  when both runs have them, else the self-time tables, else
                  the inclusive ones.
  score           err + lat + 0.25 * (metric + spectrum Ochiai + shape
                  novelty + trace + load), each term present with its switch
                  and prerequisites, added in that order.
  personalization p + 1e-9 * sum(p) (a non-finite p counts as 0); ones when
                  sum(p) <= 0.

RefContext answers the Context calls features() and rank() make from the
references the suite already holds the kernels to (oracle.native, the *_ref
helpers, ewma_ref), each as the product's own result dataclass."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import anomod
from anomod.decode import MetricMatrix
from anomod.spans import (CriticalPath, EdgeTable, ErrorOrigins, TraceShapes, TraceSpectrum)
from oracle import native

import ewma_ref
from critical_path_ref import cp_table_ref, critical_path_ref
from edge_exemplars_ref import exemplars_ref
from edge_load_ref import edge_load_ref
from edge_window_quantiles_ref import edge_window_quantiles_ref
from edge_windows_ref import edge_windows_ref, formula_starts
from error_origins_ref import origins_ref
from self_time_ref import as_edge_table, self_table_ref
from spectrum_ref import spectrum_ref
from trace_shapes_ref import census_ref, path_hash_ref, shapes_ref

NAN = float("nan")
INF = float("inf")


# ----------------------------------------------------------------- the rules
def column_score(col, drop_first: bool, f32: bool = False) -> float | None:
    """Score of one column of window scores; None when no window is left."""
    vals = [float(v) for v in col]
    if drop_first:
        vals = vals[1:]
    n = len(vals)
    if n == 0:
        return None
    k = max(1, n // 20)
    if any(v != v for v in vals):
        return NAN
    top = sorted(vals)[n - k:]
    if f32:
        with np.errstate(over="ignore"):
            acc = np.float32(top[0])
            for v in top[1:]:
                acc = np.float32(acc + np.float32(v))
            return float(np.float32(acc / np.float32(k)))
    acc = top[0]
    for v in top[1:]:
        acc = acc + v
    return acc / k


def squash(x: float) -> float:
    return 1.0 if x == INF else x / (1.0 + x)


def series_service(key, services) -> int | None:
    best = None
    labels = key[1] if len(key) > 1 else ()
    for _, value in labels:
        text = str(value)
        for i, name in enumerate(services):
            if not name or name not in text:
                continue
            if best is None or len(name) > len(services[best]) or (
                    len(name) == len(services[best]) and i < best):
                best = i
    return best


def max_per_service(S: int, owners, scores) -> list:
    """Per service the largest score of the columns it owns, from 0; a column
    without an owner or with a NaN score is skipped."""
    out = [0.0] * S
    for owner, sc in zip(owners, scores):
        if owner is None or sc is None or sc != sc:
            continue
        if sc > out[owner]:
            out[owner] = sc
    return out


def z_term(S: int, Z, owners, drop_first: bool, f32: bool = False) -> tuple[list, list]:
    """(raw per-service score, squashed term) of a window score matrix Z [n,
    columns] whose column j belongs to service owners[j]."""
    if Z is None:
        return [0.0] * S, [0.0] * S
    Z = np.asarray(Z)
    assert Z.shape[1] == len(owners), (Z.shape, len(owners))
    scores = [column_score(Z[:, j].tolist(), drop_first, f32) for j in range(Z.shape[1])]
    raw = max_per_service(S, owners, scores)
    return raw, [squash(x) for x in raw]


def active_rows(*tables) -> list:
    """Edge rows with a non-zero cell in one of the [T, E] tables, ascending."""
    E = tables[0].shape[1]
    return [r for r in range(E) if any(bool(t[:, r].any()) for t in tables)]


def per_child(S: int, table) -> list:
    """An [E] integer table summed over the S + 2 parent rows of every child."""
    t = [int(v) for v in table]
    return [sum(t[p * S + c] for p in range(S + 2)) for c in range(S)]


def rate(num, den) -> list:
    return [a / b if b > 0 else 0.0 for a, b in zip(num, den)]


@dataclass
class Latency:
    """One run's latency table: count and p99 per edge row over `services`."""
    services: list
    count: np.ndarray
    p99: np.ndarray

    @staticmethod
    def of(t: EdgeTable | None) -> "Latency | None":
        return None if t is None else Latency(list(t.services), t.count, t.p99_us)


def latency_term(cur: Latency, base: Latency, min_count: int = 10) -> list:
    S, Sb = len(cur.services), len(base.services)
    names = list(cur.services) + ["ROOT", "ORPHAN"]
    brow = {name: i for i, name in enumerate(list(base.services))}
    out = [0.0] * S
    for c in range(S):
        if cur.services[c] not in brow:
            continue
        for p in range(S + 2):
            # ROOT / ORPHAN are rows, not names: a service that happens to be
            # called so still matches only itself
            if p < S:
                if names[p] not in brow:
                    continue
                pb = brow[names[p]]
            else:
                pb = Sb + (p - S)
            r, rb = p * S + c, pb * Sb + brow[cur.services[c]]
            a, b = float(cur.p99[r]), float(base.p99[rb])
            if int(cur.count[r]) < min_count or int(base.count[rb]) < min_count:
                continue
            if not (math.isfinite(a) and math.isfinite(b) and b > 0):
                continue
            if a > 0:
                out[c] = max(out[c], max(0.0, math.log2(a / b)))
    return out


def ochiai(ef: int, ep: int, F: int) -> float:
    den = math.sqrt(float(F) * (float(ef) + float(ep)))
    return ef / den if den > 0 else 0.0


def shape_novelty(S: int, shape, count, first_trace, trace_ptr, svc, base_shape) -> list:
    have = set(int(v) for v in base_shape)
    num, den = [0] * S, [0] * S
    for v, c, t in zip(shape.tolist(), count.tolist(), first_trace.tolist()):
        for s in set(svc[int(trace_ptr[t]):int(trace_ptr[t + 1])].tolist()):
            den[s] += c
            if v not in have:
                num[s] += c
    return rate(num, den)


def personalization(scores) -> list:
    p = [float(v) if math.isfinite(v) else 0.0 for v in scores]
    if sum(p) <= 0:
        p = [1.0] * len(p)
    total = sum(p)
    return [v + 1e-9 * total for v in p]


# ----------------------------------------------------------------- the model
@dataclass
class Inputs:
    """What the composition reads, as arrays.  A table of a switch that is off
    is None; base_* are the baseline run's (None without a baseline, or when
    that run lacks the table)."""
    services: list
    count: np.ndarray                    # u64 [E]
    errors: np.ndarray                   # u64 [E]
    inclusive: Latency = None
    metric_Z: np.ndarray | None = None   # [n, series]
    metric_series: list | None = None
    self_time: bool = False
    self_lat: Latency | None = None
    critical_path: bool = False
    cp_lat: Latency | None = None
    origin: np.ndarray | None = None     # u64 [E] (error_origins)
    spectrum: tuple | None = None        # (svc_traces u64 [2, S], abnormal traces)
    shapes: tuple | None = None          # (shape, count, first_trace, trace_ptr, svc)
    trace_Z: np.ndarray | None = None    # [n, cols_per_edge * active rows]
    trace_on: bool = False
    trace_count: np.ndarray | None = None  # u64 [T, E]: EdgeWindows.count
    cols_per_edge: int = 2
    load_Z: np.ndarray | None = None     # [n, active rows]
    load_on: bool = False
    load_busy: np.ndarray | None = None  # u64 [T, E]
    load_carried: np.ndarray | None = None
    has_baseline: bool = False
    base_inclusive: Latency | None = None
    base_self: Latency | None = None
    base_cp: Latency | None = None
    base_shape: np.ndarray | None = None


def model(x: Inputs) -> dict:
    """Every component and the score, as lists of Python floats."""
    S = len(x.services)
    out: dict = {}
    # metric term: first window kept
    owners = [series_service(k, x.services) for k in (x.metric_series or [])]
    f32 = x.metric_Z is not None and np.asarray(x.metric_Z).dtype == np.float32
    _, out["metric"] = z_term(S, x.metric_Z, owners, drop_first=False, f32=f32)
    # error term
    calls = per_child(S, x.count)
    if x.origin is not None:
        out["error_rate"] = rate(per_child(S, x.origin), calls)
        out["error_kind"] = "origin"
    else:
        out["error_rate"] = rate(per_child(S, x.errors), calls)
    # latency term
    if x.critical_path and x.cp_lat is not None and x.base_cp is not None:
        kind, lat = "critical", latency_term(x.cp_lat, x.base_cp)
    elif x.self_time and x.self_lat is not None and x.base_self is not None:
        kind, lat = "self", latency_term(x.self_lat, x.base_self)
    elif x.has_baseline:
        kind, lat = "inclusive", latency_term(x.inclusive, x.base_inclusive)
    else:
        kind, lat = "inclusive", [0.0] * S
    out["latency"] = lat
    if x.self_time or x.critical_path:
        out["latency_kind"] = kind
    score = [e + l + 0.25 * m for e, l, m in zip(out["error_rate"], lat, out["metric"])]
    if x.spectrum is not None:
        svc_traces, F = x.spectrum
        out["spectrum"] = [ochiai(int(svc_traces[1][s]), int(svc_traces[0][s]), int(F))
                           for s in range(S)]
        score = [a + 0.25 * b for a, b in zip(score, out["spectrum"])]
    if x.shapes is not None and x.base_shape is not None:
        out["shape_novelty"] = shape_novelty(S, *x.shapes, x.base_shape)
        score = [a + 0.25 * b for a, b in zip(score, out["shape_novelty"])]
    if x.trace_on:
        rows = active_rows(x.trace_count)
        owners = [r % S for r in rows for _ in range(x.cols_per_edge)]
        out["trace_raw"], out["trace"] = z_term(S, x.trace_Z, owners, drop_first=True)
        score = [a + 0.25 * b for a, b in zip(score, out["trace"])]
    if x.load_on:
        rows = active_rows(x.load_busy, x.load_carried)
        owners = [r % S for r in rows]
        _, out["load"] = z_term(S, x.load_Z, owners, drop_first=True)
        score = [a + 0.25 * b for a, b in zip(score, out["load"])]
    out["score"] = score
    out["personalization"] = personalization(score)
    return out


COMPONENTS = ("error_rate", "latency", "metric", "spectrum", "shape_novelty", "trace", "load")


def inputs_of(exp, f, baseline=None, zs: dict | None = None) -> Inputs:
    """The Inputs of a features() result f of experiment exp against the
    features `baseline`; zs: the window scores {"metric" | "trace" | "load":
    Z} (default: f.window_scores for the metric term, none for the others)."""
    zs = dict(zs or {})
    p = f.params
    x = Inputs(list(f.edges.services), f.edges.count, f.edges.errors, Latency.of(f.edges))
    x.metric_Z = zs.get("metric", f.window_scores)
    x.metric_series = f.series if x.metric_Z is not None else None
    x.self_time, x.self_lat = f.self_edges is not None, Latency.of(f.self_edges)
    x.critical_path, x.cp_lat = f.cp_edges is not None, Latency.of(f.cp_edges)
    if f.error_origins is not None:
        x.origin = f.error_origins.origin
    if f.spectrum is not None:
        x.spectrum = (f.spectrum.svc_traces, int(f.spectrum.n_traces[1]))
    if f.shapes is not None:
        x.shapes = (f.shapes.shape, f.shapes.count, f.shapes.first_trace, exp.spans.trace_ptr,
                    exp.spans.svc)
    if f.edge_windows is not None:
        x.trace_on, x.trace_count = True, f.edge_windows.count
        x.cols_per_edge = 3 if "trace_quantile" in p else 2
        x.trace_Z = zs.get("trace")
    if f.edge_load is not None:
        x.load_on = True
        x.load_busy, x.load_carried = f.edge_load.busy_us, f.edge_load.carried
        x.load_Z = zs.get("load")
    if baseline is not None:
        x.has_baseline = True
        x.base_inclusive = Latency.of(baseline.edges)
        x.base_self = Latency.of(baseline.self_edges)
        x.base_cp = Latency.of(baseline.cp_edges)
        x.base_shape = None if baseline.shapes is None else baseline.shapes.shape
    return x


def assert_model_equals(f, m: dict, rtol=1e-12):
    """features() result f against the model's output m."""
    comp = f.params["components"]
    for k in COMPONENTS:
        assert (k in comp) == (k in m), k
        if k in m:
            np.testing.assert_allclose(comp[k], m[k], rtol=rtol, atol=0, err_msg=k)
    for k in ("latency_kind", "error_kind"):
        assert comp.get(k) == m.get(k), k
    np.testing.assert_allclose(f.service_scores, m["score"], rtol=rtol, atol=0, err_msg="score")


# --------------------------------------------------------------- the context
class RefContext:
    """The Context calls of features() / rank(), answered on the CPU.

    ewma: "oracle" — the C oracle's f32 window scores; "dd" — the
    double-double reference's f64 scores plus shift * its error bound
    (ewma_ref.window_bound), clipped at 0 and rounded outward to f32 when
    shift != 0: the ends of the interval a kernel within the bound lies in.
    z_hook(name, Z) -> Z edits the window scores of a call ("metric", "trace"
    or "load": the table asked for before it says which).  log holds (name, X,
    alpha, W, eps, Z) of every EWMA call.  Tables are cached per span set in
    `cache`, which contexts may share; nobody writes to them."""

    handle = "ref"

    def __init__(self, ewma: str = "oracle", shift: float = 0.0, z_hook=None, cache=None):
        assert ewma in ("oracle", "dd")
        self.ewma, self.shift, self.z_hook = ewma, float(shift), z_hook
        self.cache = {} if cache is None else cache
        self.log: list = []
        self._next = "metric"

    def _memo(self, name, spans, args, make):
        key = (name, id(spans), args)
        hit = self.cache.get(key)
        if hit is None or hit[0] is not spans:
            hit = (spans, make())
            self.cache[key] = hit
        return hit[1]

    # -- tables
    def edge_aggregate(self, spans, with_hist=True) -> EdgeTable:
        self._next = "metric"   # features() starts here; its first EWMA call is the metrics'
        t = self._memo("edges", spans, (), lambda: native.finalize(native.edge_aggregate(spans)))
        tab = as_edge_table(t, spans.services)
        if not with_hist:
            tab.hist = None
        return tab

    def self_time(self, spans, with_hist=True) -> EdgeTable:
        t = self._memo("self", spans, (), lambda: self_table_ref(spans))
        return as_edge_table(t, spans.services)

    def critical_path(self, spans, with_hist=True) -> CriticalPath:
        def make():
            cp, on, _ = critical_path_ref(spans)
            return cp_table_ref(spans, cp, on), cp, on
        t, cp, on = self._memo("cp", spans, (), make)
        return CriticalPath(as_edge_table(t, spans.services), cp, on)

    def error_origins(self, spans) -> ErrorOrigins:
        r = self._memo("origins", spans, (), lambda: origins_ref(spans))
        return ErrorOrigins(list(spans.services), r.origin, r.propagated, r.stopped, r.surfaced,
                            r.absorbers, r.hops_sum, r.hops_max, r.error_spans, r.loop_spans)

    def trace_spectrum(self, spans, thr_us=None) -> TraceSpectrum:
        thr = None if thr_us is None else np.ascontiguousarray(thr_us, np.uint32)
        r = spectrum_ref(spans, thr)
        return TraceSpectrum(list(spans.services), r["n_traces"], r["svc_traces"],
                             r["edge_traces"], r["bad_spans"], r["trace_abnormal"], thr, True)

    def trace_shapes(self, spans, trace_class=None) -> TraceShapes:
        def make():
            P, on = path_hash_ref(spans)
            lo, hi = int(spans.trace_ptr[0]), int(spans.trace_ptr[-1])
            return shapes_ref(spans, P, on), int((~on[lo:hi]).sum())
        shape, off = self._memo("shapes", spans, (), make)
        c = census_ref(shape, trace_class)
        return TraceShapes(list(spans.services), c.shape, c.count, c.abnormal, c.first_trace,
                           int(c.shape.shape[0]), off)

    def edge_windows(self, spans, t0_us, step_us, n_windows):
        self._next = "trace"
        return self._memo("windows", spans, (t0_us, step_us, n_windows),
                          lambda: edge_windows_ref(spans, t0_us, step_us, n_windows))

    def edge_window_quantiles(self, spans, t0_us, step_us, n_windows, q_pct=(50, 99)):
        qs = tuple(int(q) for q in q_pct)
        self._next = "trace"

        def make():
            base = edge_windows_ref(spans, t0_us, step_us, n_windows)
            cnt, q_us, outside = edge_window_quantiles_ref(spans, t0_us, step_us, n_windows, qs)
            base.q_pct, base.q_us, base.q_count, base.outside = qs, q_us, cnt, outside
            return base
        return self._memo("quantiles", spans, (t0_us, step_us, n_windows, qs), make)

    def edge_load(self, spans, t0_us, step_us, n_windows):
        self._next = "load"
        return self._memo("load", spans, (t0_us, step_us, n_windows),
                          lambda: edge_load_ref(spans, t0_us, step_us, n_windows))

    def edge_exemplars(self, spans, k=8, errors_only=False):
        which = 1 if errors_only else 0
        return self._memo("exemplars", spans, (int(k), which),
                          lambda: exemplars_ref(spans, int(k), which))

    # -- window scores
    def ewma_z(self, X, alpha, W, eps=1e-12):
        X = np.ascontiguousarray(X, np.float32)
        if X.shape[0] % W:
            raise ValueError(f"T={X.shape[0]} must be a multiple of W={W}")
        name = self._next   # the series of the table asked for last
        if self.ewma == "oracle":
            Z = native.ewma_z(X, alpha, W, eps)
        else:
            Z = dd_scores(X, alpha, W, eps, self.shift)
        if self.z_hook is not None:
            Z = self.z_hook(name, Z)
        self.log.append((name, X, alpha, W, eps, Z))
        return Z

    # -- ranking
    def pagerank(self, row_ptr, col, w, p, alpha=0.85, iters=100, tol=1e-10):
        return native.pagerank(row_ptr, col, w, p, alpha, iters, tol)


def dd_scores(X, alpha, W, eps, shift: float = 0.0) -> np.ndarray:
    """Window scores of the double-double reference, moved by shift * the
    kernels' bound; with a shift, clipped at 0 and rounded outward to an f32
    value (kept as f64 where shift == 0)."""
    ref = ewma_ref.ewma_ref(X, alpha, W, eps)
    if shift == 0.0:
        return ref.Z
    with np.errstate(all="ignore"):
        z = np.maximum(ref.Z + shift * ewma_ref.window_bound(ref), 0.0)
        z32 = z.astype(np.float32)
        wrong = (z32 > z) if shift < 0 else (z32 < z)
        z32 = np.where(wrong, np.nextafter(z32, np.float32(-np.inf if shift < 0 else np.inf)), z32)
    return np.where(np.isfinite(z), z32, z).astype(np.float32)


def run(exp, ctx: RefContext, baseline=None, **kw):
    """(features(exp, ctx, baseline=baseline, **kw), its window scores by name)."""
    ctx.log.clear()
    f = anomod.features(exp, ctx, baseline=baseline, **kw)
    zs = {call[0]: call[5] for call in ctx.log}
    assert len(zs) == len(ctx.log)
    return f, zs


# ------------------------------------------------------------- shared inputs
T0 = 1_762_000_005_000_000   # a multiple of 15 s
STEP_S = 15.0
N_WINDOWS = 48

CASES = {
    # name: (topology, traces, seed, baseline seed, fault service)
    "SN": ("SN", 2000, 11, 12, "home-timeline-service"),
    "TT": ("TT", 300, 21, 22, "ts-order-service"),
}
ALL_ON = dict(trace_step_s=STEP_S, self_time=True, spectrum=True, critical_path=True,
              trace_quantile=90, shapes=True, error_origins=True, trace_load=True, exemplars=4)
# The points features() runs at on the GPU.  Besides all switches together, the
# single-switch points are those at which no two services of the case come
# closer than 100 x the enclosure's width (the TT services without errors or
# latency growth tie in the trace terms down to the 1e-9 their metric terms
# differ by): test_engine_model_host.py asserts that from the references alone.
GPU_POINTS = {"SN": ("all", "trace", "trace_load", "trace_quantile"),
              "TT": ("all", "spectrum", "critical_path", "error_origins")}


def gpu_point(point: str) -> dict:
    return dict({"all": ALL_ON, "trace": dict(trace_step_s=STEP_S),
                 "trace_load": dict(trace_step_s=STEP_S, trace_load=True),
                 "trace_quantile": dict(trace_step_s=STEP_S, trace_quantile=90),
                 "spectrum": dict(spectrum=True), "critical_path": dict(critical_path=True),
                 "error_origins": dict(error_origins=True)}[point])


def synth_experiment(topology, n_traces, seed, fault=None, metric_steps=240,
                     series_per_service=3, n_windows=N_WINDOWS):
    """load_experiment(SynthSpec) with a start column: the traces spread in
    order over n_windows windows of STEP_S, 50 us between a trace's spans."""
    exp = anomod.load_experiment(anomod.SynthSpec(topology, seed=seed, fault_service=fault),
                                 n_traces=n_traces, metric_steps=metric_steps,
                                 series_per_service=series_per_service)
    exp.spans.start_us = formula_starts(exp.spans, T0, int(n_windows * STEP_S * 1e6), 50)
    return exp


def with_bad_series(exp, kind):
    """exp with one more series of its last service, holding a bad sample."""
    mm = exp.metrics
    T = mm.T
    rng = np.random.default_rng(99)
    x = (100 + rng.standard_normal(T)).astype(np.float32)
    if kind == "inf":
        x[T - 1] = np.inf                 # the last step: an infinite score in the last window
    elif kind == "nan":
        x[:] = np.nan
    elif kind == "f32_range":
        x[:] = 100.0                      # v = 0: z = d / sqrt(eps) leaves the f32 range
        x[T - 1] = 3e38
    victim = exp.services[-1]
    X = np.concatenate([mm.X, x[:, None]], axis=1)
    series = list(mm.series) + [("bad_metric", (("service", victim),))]
    return anomod.Experiment(exp.name, exp.spans, MetricMatrix(X, mm.timestamps, series), exp.label)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(faulty experiment, fault-free baseline experiment) of CASES[name]."""
    topo, n, seed, bseed, fault = CASES[name]
    return synth_experiment(topo, n, seed, fault), synth_experiment(topo, n, bseed)


def score_interval(exp, f, baseline, calls) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(low, mid, high) service scores of the model over the tables of f with
    the window scores of the double-double reference at -bound, 0, +bound;
    calls: [(name, X, alpha, W, eps)] of the EWMA calls.  Every z-term is
    monotone non-decreasing in each window score, so a kernel within the
    bound scores inside [low, high]."""
    out = []
    for shift in (-1.0, 0.0, 1.0):
        zs = {n: dd_scores(X, a, W, e, shift) for n, X, a, W, e in calls}
        out.append(np.asarray(model(inputs_of(exp, f, baseline, zs))["score"]))
    return tuple(out)


def smallest_gap(scores) -> float:
    s = sorted(float(v) for v in scores)
    gaps = [b - a for a, b in zip(s, s[1:]) if b > a]
    return min(gaps)


def integer_tables(f) -> dict:
    """Every integer array / count held by a Features, by dotted name (the
    edge tables' p50 / p99, functions of the histogram, ride along)."""
    out = {}

    def walk(prefix, obj):
        for k, v in vars(obj).items():
            if k.startswith("_") or k in ("services", "params", "series"):
                continue
            name = f"{prefix}.{k}" if prefix else k
            if isinstance(v, np.ndarray):
                if v.dtype.kind in "ui" or k in ("p50_us", "p99_us"):
                    out[name] = v
            elif isinstance(v, (int, tuple)) and not isinstance(v, bool):
                out[name] = np.asarray(v)
            elif hasattr(v, "__dataclass_fields__"):
                walk(name, v)
    walk("", f)
    return out


def assert_integer_tables_equal(got, ref):
    a, b = integer_tables(got), integer_tables(ref)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)   # NaNs compare equal

"""load_experiment -> features -> rank: the engine's call surface.

The reference produces one experiment's telemetry with bash + Python
collectors (SURVEY.md §3 call stacks A-C) and stops at files; this module
reads those files (or a synthetic equivalent) and computes the RCA features
on the GPU:

* edge table: libanomod edge aggregation (HIP), per-edge histogram, counts,
  errors, p50/p99;
* window scores: libanomod EWMA/z kernel over the metric matrix;
* ranking: libanomod personalized PageRank over the caller -> callee graph,
  seeded by per-service anomaly scores;
* symptom correlation: libanomod series correlation of the per-edge trace
  series and the metric series against the front-door latency series, which
  can weight the walk (rank(walk="correlation")).
"""
from __future__ import annotations

import math
import re
import threading
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from . import decode
from .device import Context, SynthSpec, synth_generate_host
from .spans import (CallRepeats, CallTransit, EdgeExemplars, EdgeLoad, EdgeTable, EdgeWindows, ErrorOrigins, SpanSet,
                    TraceShapes, TraceSpectrum, edge_rows, spectrum_thresholds)

# --------------------------------------------------------------------------
# Ground-truth labels (experiment name -> faulty service), SURVEY.md §2:
# SN automated_multimodal_collection.sh:904-916 / :323-496;
# TT chaos-experiments/*.yaml target_service and run_experiment.sh:299-345.
# --------------------------------------------------------------------------
_SN_LABELS = {
    "Svc_Kill_Media": "media-service",
    "Svc_Kill_SocialGraph": "social-graph-service",
    "Svc_Kill_UserTimeline": "user-timeline-service",
    "Code_Stop_MediaService": "media-service",
    "Code_Stop_TextService": "text-service",
    "Code_Stop_UserService": "user-service",
    "DB_Redis_CacheLimit_HomeTimeline": "home-timeline-service",
    "DB_Redis_CacheLimit_SocialGraph": "social-graph-service",
    "DB_Redis_CacheLimit_UserTimeline": "user-timeline-service",
}


def fault_target(experiment_name: str) -> str | None:
    """Faulty service named by an experiment directory, if the name encodes one."""
    for key, svc in _SN_LABELS.items():
        if experiment_name.startswith(key):
            return svc
    m = re.search(r"(ts-[a-z0-9-]+-service)", experiment_name)
    if m:
        return m.group(1)
    return None


@dataclass
class Experiment:
    name: str
    spans: SpanSet | None
    metrics: decode.MetricMatrix | None = None
    label: str | None = None
    meta: dict = field(default_factory=dict)

    @property
    def services(self) -> list[str]:
        return self.spans.services if self.spans is not None else []


def _synthetic_metrics(services: list[str], T: int, series_per_service: int, seed: int,
                       fault: str | None) -> decode.MetricMatrix:
    rng = np.random.default_rng(seed)
    keys, cols = [], []
    for s in services:
        for k in range(series_per_service):
            mu, sd = rng.uniform(10, 1000), rng.uniform(0.5, 5)
            x = mu + sd * rng.standard_normal(T)
            if fault is not None and s == fault:
                x[T // 2:] += 8 * sd  # level shift at the fault
            keys.append((f"synthetic_metric_{k}", (("service", s),)))
            cols.append(x.astype(np.float32))
    X = np.stack(cols, axis=1) if cols else np.zeros((T, 0), np.float32)
    return decode.MetricMatrix(X, np.arange(T, dtype=np.float64) * 15.0, keys)


def load_experiment(source, *, metrics=None, name: str | None = None,
                    services: list[str] | None = None, n_traces: int | None = None,
                    metric_steps: int = 480, series_per_service: int = 4) -> Experiment:
    """Load one experiment.

    ``source`` is one of
      * a :class:`SynthSpec` — synthetic SN/TT spans (``n_traces`` traces,
        default 600 = 50 per SN service as collect_trace.sh:18/:49 scrapes)
        over the services they name, plus a synthetic metric matrix;
      * a Jaeger dump (``all_traces.json``) or its directory
        (SN_data/trace_data/<exp>_traces_<ts>/);
      * a SkyWalking payload JSON (TT_data/trace_data/<exp>/*.json) or its
        directory;
    ``metrics`` optionally names an SN metric directory (one CSV per query)
    or a TT long-format metric CSV.
    """
    if isinstance(source, SynthSpec):
        nt = 600 if n_traces is None else n_traces
        spans = synth_generate_host(source, nt)
        fault = source.fault_service
        if isinstance(fault, int):
            fault = spans.services[fault]
        # the services the traces name, as a collector payload lists them
        # (services_discovered, trace_collector.py:572): the same experiment
        # read back from its files has the same service list
        spans = spans.observed_services()
        X = _synthetic_metrics(spans.services, metric_steps, series_per_service,
                               source.seed ^ 0x5EED, fault) if metric_steps else None
        return Experiment(name or f"synthetic_{source.topology}", spans, X, fault,
                          {"synthetic": True})

    path = Path(source)
    exp_name = name or (path.name if path.is_dir() else path.parent.name)
    doc_path = path
    if path.is_dir():
        if (path / "all_traces.json").exists():
            doc_path = path / "all_traces.json"
        else:
            cands = sorted(path.glob("*skywalking_traces_*.json")) or sorted(path.glob("*.json"))
            if not cands:
                raise FileNotFoundError(f"no trace JSON under {path}")
            doc_path = cands[-1]
    # the metric file decodes on a second host thread while the trace file
    # decodes here: both decoders are native and release the GIL, and each
    # has a serial stretch the other's threads fill
    got: dict = {}
    worker = None
    if metrics is not None:
        mp = Path(metrics)

        def _metrics():
            try:
                got["m"] = (decode.decode_prometheus_csv_dir_native(mp) if mp.is_dir()
                            else decode.decode_metric_long_csv_native(mp))
            except BaseException as e:  # noqa: BLE001 (re-raised below)
                got["e"] = e

        worker = threading.Thread(target=_metrics, name="anomod-metrics-decode")
        worker.start()
    try:
        spans = decode.load_trace_file(doc_path, services)
    finally:
        if worker is not None:
            worker.join()
    if "e" in got:
        raise got["e"]
    return Experiment(exp_name, spans, got.get("m"), fault_target(exp_name),
                      {"trace_file": str(doc_path)})


@dataclass
class SymptomCorrelation:
    """features(symptom_corr=True): how every trace series and every metric
    series moves with the front-door latency (EdgeWindows.symptom).  r is the
    Pearson correlation over the windows where both are present (n of them;
    NaN below min_pairs or for a constant side: Context.correlate)."""

    services: list[str]
    symptom: np.ndarray                    # f32 [T] on the trace windows
    keys: list                             # the correlated columns of win.matrix()
    r: np.ndarray                          # f64 [len(keys)]
    n: np.ndarray                          # u32 [len(keys)]
    service: np.ndarray                    # f64 [S] in [0, 1]: max r over incoming edges
    # the metric part: "regular" (computed), "irregular" or "none" (skipped)
    metric_grid: str = "none"
    metric_rows: tuple[int, int] | None = None   # metric rows [i0, i1] it covers
    metric_symptom: np.ndarray | None = None     # f32 on those rows
    metric_keys: list | None = None              # the metric series
    metric_r: np.ndarray | None = None
    metric_n: np.ndarray | None = None
    metric_service: np.ndarray | None = None     # f64 [S]: max |r| over a service's series

    def top(self, k: int = 10) -> list[dict]:
        """The k columns / series of largest |r| (NaN left out; ties by
        position, trace columns first): {"kind": "trace" | "metric", "key",
        "r", "n"}."""
        rows = [("trace", key, float(r), int(n)) for key, r, n in zip(self.keys, self.r, self.n)]
        if self.metric_keys is not None:
            rows += [("metric", key, float(r), int(n))
                     for key, r, n in zip(self.metric_keys, self.metric_r, self.metric_n)]
        rows = [row for row in rows if row[2] == row[2]]
        rows.sort(key=lambda row: -abs(row[2]))
        return [{"kind": kind, "key": key, "r": r, "n": n} for kind, key, r, n in rows[:max(0, k)]]


@dataclass
class Features:
    experiment: str
    edges: EdgeTable
    window_scores: np.ndarray | None      # [T/W, S] max |z| per window
    series: list | None
    service_scores: np.ndarray             # [n_services] anomaly score
    params: dict = field(default_factory=dict)
    # features(trace_step_s=...): the per-window edge table and the per-service
    # trace anomaly scores taken from it
    edge_windows: EdgeWindows | None = None
    trace_window_scores: np.ndarray | None = None
    # features(self_time=True): the self-time (exclusive latency) edge table
    self_edges: EdgeTable | None = None
    # features(spectrum=True): abnormal / normal trace labels and coverage
    spectrum: TraceSpectrum | None = None
    # features(critical_path=True): the critical-path edge table
    cp_edges: EdgeTable | None = None
    # features(shapes=True): the trace shape census
    shapes: TraceShapes | None = None
    # features(error_origins=True): where failures started and how far they travelled
    error_origins: ErrorOrigins | None = None
    # features(repeats=True): repeated and retried calls per edge
    repeats: CallRepeats | None = None
    # features(transit=True): request and response gaps per edge
    transit: CallTransit | None = None
    # features(trace_load=True): per-window busy time and carried calls of every edge
    edge_load: EdgeLoad | None = None
    # features(exemplars=K): the K slowest calls of every edge, and the K
    # slowest error-flagged ones
    exemplars: EdgeExemplars | None = None
    error_exemplars: EdgeExemplars | None = None
    # features(symptom_corr=True): correlation with the front-door latency
    symptom_corr: SymptomCorrelation | None = None


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None or _default_ctx.handle is None:
        _default_ctx = Context(0)
    return _default_ctx


def _series_service(key, services: list[str], memo: dict | None = None) -> int | None:
    """Map a metric series to a service by its label values (pod, container,
    service, job ... carry the service name in both datasets): the longest
    service name contained in a label value, the first such in `services`
    order on ties.  Service names hold no spaces, so this is decided value by
    value; `memo` (one per call site) keeps each distinct value's answer."""
    labels = key[1] if len(key) > 1 else ()
    best = None
    for _, v in labels:
        v = str(v)
        hit = memo.get(v, -2) if memo is not None else -2
        if hit == -2:
            hit = -1
            for i, s in enumerate(services):
                if s and s in v and (hit < 0 or len(s) > len(services[hit])):
                    hit = i
            if memo is not None:
                memo[v] = hit
        if hit >= 0 and (best is None or len(services[hit]) > len(services[best])
                         or (len(services[hit]) == len(services[best]) and hit < best)):
            best = hit
    return best


def _latency_shift(cur: EdgeTable, base: EdgeTable, min_count: int = 10) -> np.ndarray:
    """Per service: largest log2 growth of an incoming edge's GPU p99 over
    the same edge — matched by service NAMES (the two runs may have seen
    different service sets: services_discovered lists only the services a
    run's traces name, trace_collector.py:572) — in a baseline run (edges
    with >= min_count spans on both sides)."""
    S, Sb = cur.n_services, base.n_services
    out = np.zeros(S)
    pos = {s: i for i, s in enumerate(base.services)}
    m = np.array([pos.get(s, -1) for s in cur.services] + [Sb, Sb + 1], np.int64)  # + ROOT, ORPHAN
    p_cur = np.repeat(np.arange(S + 2), S)
    c_cur = np.tile(np.arange(S), S + 2)
    pb, cb = m[p_cur], m[c_cur]
    have = (pb >= 0) & (cb >= 0)
    rows = np.where(have, pb * Sb + np.where(cb >= 0, cb, 0), 0)
    bc = np.where(have, base.count[rows], 0)
    bp = np.where(have, base.p99_us[rows], np.nan)
    ok = ((cur.count >= min_count) & (bc >= min_count) & np.isfinite(cur.p99_us)
          & np.isfinite(bp) & (bp > 0))
    ratio = np.zeros(cur.count.shape[0])
    ratio[ok] = np.maximum(0.0, np.log2(cur.p99_us[ok] / bp[ok]))
    return ratio.reshape(S + 2, S).max(axis=0)


def _repeat_components(rep: CallRepeats, min_groups: int = 10) -> tuple[np.ndarray, np.ndarray]:
    """Per service (amplification, retry_rate): over the incoming rows with >=
    min_groups groups the largest row amplification minus 1 (0 without such a
    row), and retried / groups, both summed over the incoming rows (0 where
    the service has no group)."""
    S = len(rep.services)
    amp = np.where(rep.groups >= min_groups, rep.amplification() - 1.0, 0.0)
    g = rep.per_service("groups").astype(np.float64)
    rate = np.divide(rep.per_service("retried").astype(np.float64), g, out=np.zeros(S),
                     where=g > 0)
    return amp.reshape(S + 2, S).max(axis=0), rate


def _repeat_shift(cur: CallRepeats, base: CallRepeats, min_groups: int = 10) -> np.ndarray:
    """Per service: largest log2 growth of an incoming edge's call
    amplification over the same edge — matched by service NAMES, as
    _latency_shift matches them — in a baseline run (rows with >= min_groups
    groups on both sides); never below 0."""
    S, Sb = len(cur.services), len(base.services)
    pos = {s: i for i, s in enumerate(base.services)}
    m = np.array([pos.get(s, -1) for s in cur.services] + [Sb, Sb + 1], np.int64)  # + ROOT, ORPHAN
    p_cur = np.repeat(np.arange(S + 2), S)
    c_cur = np.tile(np.arange(S), S + 2)
    pb, cb = m[p_cur], m[c_cur]
    have = (pb >= 0) & (cb >= 0)
    rows = np.where(have, pb * Sb + np.where(cb >= 0, cb, 0), 0)
    bg = np.where(have, base.groups[rows], 0)
    ba = base.amplification()[rows]
    ok = have & (cur.groups >= min_groups) & (bg >= min_groups)
    shift = np.zeros(cur.groups.shape[0])
    shift[ok] = np.maximum(0.0, np.log2(cur.amplification()[ok] / ba[ok]))
    return shift.reshape(S + 2, S).max(axis=0)


def _transit_shift(cur: CallTransit, base: CallTransit, min_count: int = 10) -> np.ndarray:
    """Per service: largest log2 growth of the p99 of an incoming
    cross-service row (p < S, p != c: a handler's gap to its own client span
    is work, not transit) of the request or the response table over the same
    row — matched by service NAMES, as _latency_shift matches them — in a
    baseline run (>= min_count records on both sides in the table in question,
    a finite baseline p99 > 0); never below 0."""
    S, Sb = len(cur.services), len(base.services)
    pos = {s: i for i, s in enumerate(base.services)}
    m = np.array([pos.get(s, -1) for s in cur.services], np.int64)
    p_cur = np.repeat(np.arange(S), S)
    c_cur = np.tile(np.arange(S), S)
    pb, cb = m[p_cur], m[c_cur]
    have = (pb >= 0) & (cb >= 0) & (p_cur != c_cur)
    rows = np.where(have, pb * Sb + np.where(cb >= 0, cb, 0), 0)
    out = np.zeros(S)
    for tc, tb in ((cur.request, base.request), (cur.response, base.response)):
        cc, cp = tc.count[:S * S], tc.p99_us[:S * S]
        bc = np.where(have, tb.count[rows], 0)
        bp = np.where(have, tb.p99_us[rows], np.nan)
        ok = (have & (cc >= min_count) & (bc >= min_count) & np.isfinite(cp) & np.isfinite(bp)
              & (bp > 0))
        shift = np.zeros(S * S)
        shift[ok] = np.maximum(0.0, np.log2(cp[ok] / bp[ok]))
        out = np.maximum(out, shift.reshape(S, S).max(axis=0))
    return out


def _squash(x: np.ndarray) -> np.ndarray:
    """x / (1 + x), z into [0, 1], with its limit 1 at +inf (inf / inf is NaN)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isposinf(x), 1.0, x / (1.0 + x))


def trace_window_scores(Z: np.ndarray, win: EdgeWindows, S: int,
                        cols_per_edge: int = 2) -> np.ndarray:
    """Per-service trace anomaly score from the window scores Z [n,
    cols_per_edge * active edges] of win.matrix() (3 columns an edge with its
    quantile column): the first score window is dropped (the EWMA variance
    starts at 0 there), a column scores the mean of its top k =
    max(1, n_left // 20) windows, and a service takes the max over the columns
    of the edges it is the child of (row % S; ROOT and ORPHAN rows included);
    a column whose score is NaN is skipped."""
    out = np.zeros(S)
    Z = np.asarray(Z, np.float64)[1:]
    if Z.shape[0] == 0 or Z.shape[1] == 0:
        return out
    k = max(1, Z.shape[0] // 20)
    top = np.sort(Z, axis=0)[-k:].mean(axis=0)
    active = np.nonzero(win.count.sum(axis=0))[0]
    child = np.repeat(active % S, int(cols_per_edge))
    np.fmax.at(out, child, top[: child.shape[0]])
    return out


def load_window_scores(Z: np.ndarray, load: EdgeLoad, S: int) -> np.ndarray:
    """Per-service load score from the window scores Z [n, active edges] of
    load.matrix(), by the rule of trace_window_scores: the first score window
    is dropped, a column scores the mean of its top k = max(1, n_left // 20)
    windows, and a service takes the max over the edges it is the child of
    (a column whose score is NaN is skipped)."""
    out = np.zeros(S)
    Z = np.asarray(Z, np.float64)[1:]
    if Z.shape[0] == 0 or Z.shape[1] == 0:
        return out
    k = max(1, Z.shape[0] // 20)
    top = np.sort(Z, axis=0)[-k:].mean(axis=0)
    child = load.active_rows() % S
    np.fmax.at(out, child, top[: child.shape[0]])
    return out


MAX_TRACE_WINDOWS = 65536          # anomod_edge_windows: T <= 65536, T * E <= 2^24
MAX_TRACE_CELLS = 1 << 24


def _trace_range(spans: SpanSet, step_s: float) -> tuple[int, int, int]:
    """(t0_us, step_us, n_windows) of the window range the trace series use:
    from the step-aligned smallest non-zero start to the largest."""
    if spans.start_us is None:
        raise ValueError("features(trace_step_s=...): the span set has no start_us column")
    step_us = max(1, int(round(step_s * 1e6)))
    S = spans.n_services
    nz = spans.start_us[spans.start_us != 0]
    t0 = int(nz.min()) // step_us * step_us if nz.size else 0
    T = (int(nz.max()) - t0) // step_us + 1 if nz.size else 1
    T = max(1, min(T, MAX_TRACE_WINDOWS, MAX_TRACE_CELLS // max(1, edge_rows(S))))
    return t0, step_us, T


def _trace_load(spans: SpanSet, ctx: Context, step_s: float, W: int, eps: float
                ) -> tuple[EdgeLoad, np.ndarray]:
    """The edge-load table over the range of _trace_windows (the two tables
    line up) and its per-service score."""
    t0, step_us, T = _trace_range(spans, step_s)
    S = spans.n_services
    load = ctx.edge_load(spans, t0, step_us, T)
    mm = load.matrix().pad_to_multiple(W)
    if mm.S == 0 or mm.T == 0:
        return load, np.zeros(S)
    Z = ctx.ewma_z(mm.X, 2.0 / (W + 1), W, eps)
    return load, load_window_scores(Z, load, S)


def _trace_windows(spans: SpanSet, ctx: Context, step_s: float, W: int, eps: float,
                   min_count: int, quantile: int | None = None
                   ) -> tuple[EdgeWindows, np.ndarray, decode.MetricMatrix]:
    """The per-window edge table, its per-service score and win.matrix() (not
    padded) the score was taken from."""
    t0, step_us, T = _trace_range(spans, step_s)
    S = spans.n_services
    if quantile is None:
        win = ctx.edge_windows(spans, t0, step_us, T)
        mm0 = win.matrix(min_count)
    else:
        win = ctx.edge_window_quantiles(spans, t0, step_us, T, q_pct=(int(quantile),))
        mm0 = win.matrix(min_count, quantile=int(quantile))
    mm = mm0.pad_to_multiple(W)
    if mm.S == 0 or mm.T == 0:
        return win, np.zeros(S), mm0
    Z = ctx.ewma_z(mm.X, 2.0 / (W + 1), W, eps)
    return win, trace_window_scores(Z, win, S, 2 if quantile is None else 3), mm0


def _labels_service(series: list, services: list[str]) -> np.ndarray:
    """Service index of every series (-1: none) by _series_service, decided
    once per distinct label set (a TT matrix holds ~6 k series over ~50 label
    sets)."""
    memo: dict = {}
    labs = [k[1] if len(k) > 1 else () for k in series]
    if not all(isinstance(lb, tuple) for lb in labs):  # a caller's lists of pairs
        labs = [lb if isinstance(lb, tuple) else tuple(tuple(kv) for kv in lb) for lb in labs]
    by_labels = {}
    for lb in dict.fromkeys(labs):
        i = _series_service(("", lb), services, memo)
        by_labels[lb] = -1 if i is None else i
    return np.fromiter(map(by_labels.__getitem__, labs), np.int64, len(labs))


def _metric_grid(metrics: "decode.MetricMatrix | None") -> str:
    """"regular" when the metric matrix has T >= 2 rows whose consecutive
    timestamp differences are all equal and positive, "irregular" when it has
    rows that are not, "none" without a matrix."""
    if metrics is None or metrics.S == 0 or metrics.T == 0:
        return "none"
    d = np.diff(np.asarray(metrics.timestamps, np.float64))
    return "regular" if d.size >= 1 and d[0] > 0 and bool((d == d[0]).all()) else "irregular"


def _symptom_correlation(exp: Experiment, ctx: Context, win: EdgeWindows,
                         mm0: "decode.MetricMatrix", min_count: int, min_pairs: int
                         ) -> SymptomCorrelation:
    spans, services = exp.spans, win.services
    S = len(services)
    y = win.symptom(min_count)
    per_edge = 3 if any(k[0].startswith("edge_p") for k in mm0.series) else 2
    cols = np.array([j for j, k in enumerate(mm0.series) if k[0] != "edge_count"], np.int64)
    keys = [mm0.series[j] for j in cols.tolist()]
    svc = np.zeros(S)
    if cols.size and y.shape[0]:
        r, n = ctx.correlate(mm0.X[:, cols], y, min_pairs)
        r, n = r[0], n[0]
        # the rule of trace_window_scores: a service takes the max over the
        # columns of the edges it is the child of; NaN and negative r count as 0
        active = np.nonzero(win.count.sum(axis=0))[0]
        child = (active % S)[cols // per_edge]
        np.fmax.at(svc, child, np.where(r > 0, r, 0.0))
    else:
        r, n = np.zeros(0), np.zeros(0, np.uint32)
    sc = SymptomCorrelation(list(services), y, keys, r, n, svc, _metric_grid(exp.metrics))
    if sc.metric_grid != "regular":
        return sc
    # the front-door series again, on the metric grid: metric row i covers
    # [ts[i], ts[i] + step); the rows that touch the trace start range
    ts = np.asarray(exp.metrics.timestamps, np.float64)
    step_us = max(1, int(round((ts[1] - ts[0]) * 1e6)))
    ts_us = np.rint(ts * 1e6).astype(np.int64)
    nz = spans.start_us[spans.start_us != 0]
    sc.metric_keys = list(exp.metrics.series)
    sc.metric_r = np.full(exp.metrics.S, np.nan)
    sc.metric_n = np.zeros(exp.metrics.S, np.uint32)
    sc.metric_service = np.zeros(S)
    hit = (np.nonzero((ts_us + step_us > int(nz.min())) & (ts_us <= int(nz.max())))[0]
           if nz.size else np.zeros(0, np.int64))
    if hit.size == 0:
        return sc
    i0 = int(hit[0])
    Tm = min(int(hit[-1]) - i0 + 1, MAX_TRACE_WINDOWS, MAX_TRACE_CELLS // max(1, edge_rows(S)))
    if Tm < 1:
        return sc
    win_m = ctx.edge_windows(spans, int(ts_us[i0]), step_us, Tm)
    ym = win_m.symptom(min_count)
    rm, nm = ctx.correlate(exp.metrics.X[i0:i0 + Tm], ym, min_pairs)
    sc.metric_rows, sc.metric_symptom, sc.metric_r, sc.metric_n = (i0, i0 + Tm - 1), ym, rm[0], nm[0]
    idx = _labels_service(sc.metric_keys, services)
    ok = idx >= 0
    np.fmax.at(sc.metric_service, idx[ok], np.abs(rm[0])[ok])  # a metric's sign is arbitrary
    return sc


def features(exp: Experiment, ctx: Context | None = None, *, W: int = 60,
             alpha: float | None = None, eps: float = 1e-12, with_hist: bool = True,
             baseline: "Features | None" = None, trace_step_s: float | None = None,
             trace_W: int = 6, trace_eps: float = 1e-2, trace_min_count: int = 5,
             self_time: bool = False, spectrum: bool = False,
             spectrum_rows: str = "root", critical_path: bool = False,
             trace_quantile: int | None = None, shapes: bool = False,
             error_origins: bool = False, trace_load: bool = False,
             exemplars: int | None = None, symptom_corr: bool = False,
             corr_min_pairs: int = 3, repeats: bool = False,
             transit: bool = False) -> Features:
    """GPU features of one experiment (SURVEY.md §3 stack D steps 4-7).  With
    trace_step_s (seconds; the span set needs start_us) the spans also go
    through the per-window edge table -> EWMA/z -> trace_window_scores, and
    the score gains 0.25 * ts / (1 + ts); trace_quantile=q (a percentage in
    [0, 99]; needs trace_step_s) adds the exact per-window latency quantile of
    every edge (Context.edge_window_quantiles) as a third scored series, so a
    fault that slows a fraction of an edge's calls shows in the tail series
    where the per-window mean dilutes it.  With self_time the result also
    holds the self-time edge table (Context.self_time), and the latency term
    against a baseline that has one is the p99 growth of self time instead of
    the inclusive duration (components["latency_kind"] says which), so a slow
    service no longer raises the term of its callers.  With spectrum the
    traces are labelled abnormal / normal (Context.trace_spectrum: latency
    thresholds from baseline.edges by spectrum_thresholds(rows=spectrum_rows)
    when a baseline is given, else error flags alone —
    components["spectrum_thresholds"] says which) and the score gains 0.25 *
    the per-service Ochiai coefficient of the trace coverage.  With
    critical_path (the span set needs start_us) the result also holds the
    critical-path edge table (Context.critical_path), and against a baseline
    that has one the latency term is the p99 growth of the time spans add on
    the critical path (latency_kind "critical", ahead of "self" and
    "inclusive"): a span that merely runs beside a longer sibling no longer
    raises it, and a fan-out parent's own work does.  With shapes the result
    also holds the trace shape census (Context.trace_shapes, service keys by
    name; the counts are split by the spectrum's trace labels when spectrum
    is on), and against a baseline that has one the score gains 0.25 * the
    shape novelty (TraceShapes.novelty: per service, the share of the traces
    — among those whose shape's exemplar holds the service — whose shape the
    baseline run does not have; components["shape_novelty"]).  With
    error_origins the result also holds the error origins
    (Context.error_origins) and the score's error term is the origin rate —
    the failures that started in a service over the spans it served — instead
    of the inclusive error rate, which also fires for every caller that merely
    relayed a callee's failure: components["error_rate"] then holds the origin
    rate and components["error_kind"] is "origin".  No baseline is involved.
    With trace_load (needs trace_step_s) the spans also go through the edge
    load table (Context.edge_load, over the same window range as the trace
    series) -> EWMA/z at trace_W / trace_eps -> load_window_scores, and the
    score gains 0.25 * ls / (1 + ls) (components["load"]): calls that stay
    open pile up busy time in every window they last through, which the
    start-window series above cannot see — a hung call is one cell of their
    latency sum, and none at all on an edge below trace_min_count.  With
    exemplars=K (1..64) the result also holds the K slowest calls of every
    edge and the K slowest error-flagged ones (Context.edge_exemplars:
    Features.exemplars / .error_exemplars) — the way from a ranked service
    back to the traces that show it; no score or component changes.
    With symptom_corr (needs trace_step_s) every trace series of win.matrix()
    except the call counts is correlated (Context.correlate, at least
    corr_min_pairs common windows) with the front-door latency series
    (EdgeWindows.symptom(trace_min_count)); a service takes the max over the
    columns of the edges it is the child of, NaN and negative r as 0
    (components["symptom_corr"], in [0, 1]).  With a metric matrix on a
    regular grid (params["metric_corr_grid"] = "regular"; "irregular" and
    "none" skip this part) the front-door series is taken again on the metric
    rows that touch the trace start range, every metric series is correlated
    with it and a service takes the max |r| of its series
    (components["metric_corr"]).  Features.symptom_corr holds both with the
    per-column r and n; rank(walk="correlation") walks by them.  No score or
    other component changes.
    With repeats the result also holds the call repeats (Context.call_repeats:
    how often one parent span called the same callee more than once) with
    components["amplification"] — per service, over the incoming edge rows
    with >= 10 groups, the largest spans-per-logical-call minus 1 — and
    components["retry_rate"] — retried / groups over the incoming rows.
    Against a baseline that has repeats the score gains 0.25 * the squashed
    components["repeat_shift"]: the largest log2 growth of an incoming row's
    amplification over the same row of the baseline (rows matched by service
    names, >= 10 groups on both sides); without a baseline no score changes.
    With transit (the span set needs start_us) the result also holds the call
    transit (Context.call_transit: for every call whose parent span made no
    other call, the request gap from the caller's client span to the callee
    and the response gap back) with components["abandoned_rate"] — per callee
    service over the cross-service incoming rows, the share of the timed
    calls whose caller ended first — and components["skew_rate"] — the share
    that start before their caller.  Against a baseline that has transit the
    score gains 0.25 * the squashed components["transit_shift"], added after
    every other term: the largest log2 growth of the request or response p99
    of a cross-service incoming row over the same row of the baseline (rows
    matched by service names, >= 10 records on both sides): time lost between
    two services, which leaves the callee's duration and self time where they
    were; without a baseline no score changes.
    Non-finite window scores: a column whose score is NaN is skipped, +inf
    squashes to 1, so service_scores stays finite."""
    if trace_load and trace_step_s is None:
        raise ValueError("features(trace_load=True) needs trace_step_s")
    if trace_quantile is not None and trace_step_s is None:
        raise ValueError("features(trace_quantile=...) needs trace_step_s")
    if symptom_corr and trace_step_s is None:
        raise ValueError("features(symptom_corr=True) needs trace_step_s")
    if trace_quantile is not None and not 0 <= int(trace_quantile) <= 99:
        raise ValueError(f"features(trace_quantile={trace_quantile}): a percentage in [0, 99]")
    if transit and getattr(exp.spans, "start_us", None) is None:
        raise ValueError("features(transit=True) needs a span set with start_us")
    ctx = ctx or default_context()
    edges = ctx.edge_aggregate(exp.spans, with_hist=with_hist)
    self_edges = ctx.self_time(exp.spans, with_hist=with_hist) if self_time else None
    cp_edges = (ctx.critical_path(exp.spans, with_hist=with_hist).edges if critical_path
                else None)
    S = edges.n_services
    alpha = 2.0 / (W + 1) if alpha is None else alpha
    Z = None
    series = None
    metric_score = np.zeros(S)
    if exp.metrics is not None and exp.metrics.S > 0 and exp.metrics.T > 0:
        mm = exp.metrics.pad_to_multiple(W)
        Z = ctx.ewma_z(mm.X, alpha, W, eps)
        series = mm.series
        # score a series by the mean of its top-5 % window scores (robust to
        # a single spike), then take the max over the series of a service
        k = max(1, Z.shape[0] // 20)
        top = np.sort(Z, axis=0)[-k:].mean(axis=0) if Z.shape[0] else np.zeros(Z.shape[1])
        # series -> service, then one scatter-max
        idx = _labels_service(series, edges.services)
        ok = idx >= 0
        np.fmax.at(metric_score, idx[ok], np.asarray(top, np.float64)[ok])  # skips NaN
    # error rate of the calls each service serves
    cnt = edges.count.reshape(S + 2, S).sum(axis=0).astype(np.float64)
    err = edges.errors.reshape(S + 2, S).sum(axis=0).astype(np.float64)
    err_rate = np.divide(err, cnt, out=np.zeros(S), where=cnt > 0)
    origins = None
    if error_origins:
        origins = ctx.error_origins(exp.spans)
        err_rate = origins.origin_rate(edges.count)
    lat = np.zeros(S)
    use_self = self_edges is not None and baseline is not None and baseline.self_edges is not None
    use_cp = cp_edges is not None and baseline is not None and baseline.cp_edges is not None
    if use_cp:
        lat = _latency_shift(cp_edges, baseline.cp_edges)
    elif use_self:
        lat = _latency_shift(self_edges, baseline.self_edges)
    elif baseline is not None:
        lat = _latency_shift(edges, baseline.edges)
    ms = _squash(metric_score)  # squash z into [0, 1]
    score = err_rate + lat + 0.25 * ms
    params = {"W": W, "alpha": alpha, "eps": eps,
              "components": {"error_rate": err_rate, "latency": lat, "metric": ms}}
    if self_time or critical_path:
        params["components"]["latency_kind"] = ("critical" if use_cp else
                                                "self" if use_self else "inclusive")
    if error_origins:
        params["components"]["error_kind"] = "origin"
    spec = None
    if spectrum:
        thr = (spectrum_thresholds(baseline.edges, edges.services, rows=spectrum_rows)
               if baseline is not None else None)
        spec = ctx.trace_spectrum(exp.spans, thr_us=thr)
        och = spec.ochiai()
        params["components"]["spectrum"] = och
        params["components"]["spectrum_thresholds"] = "baseline" if thr is not None else "errors-only"
        score = score + 0.25 * och
    census = None
    if shapes:
        census = ctx.trace_shapes(exp.spans,
                                  trace_class=spec.trace_abnormal if spec is not None else None)
        if baseline is not None and baseline.shapes is not None:
            nov = census.novelty(exp.spans, baseline.shapes)
            params["components"]["shape_novelty"] = nov
            score = score + 0.25 * nov
    rep_table, rep_term = None, None
    if repeats:
        rep_table = ctx.call_repeats(exp.spans)
        amp, retry_rate = _repeat_components(rep_table)
        params["components"]["amplification"] = amp
        params["components"]["retry_rate"] = retry_rate
        if baseline is not None and baseline.repeats is not None:
            shift = _repeat_shift(rep_table, baseline.repeats)
            params["components"]["repeat_shift"] = shift
            rep_term = 0.25 * _squash(shift)   # added last: the other terms sum as without it
    tr_table, tr_term = None, None
    if transit:
        tr_table = ctx.call_transit(exp.spans, with_hist=with_hist)
        params["components"]["abandoned_rate"] = tr_table.abandoned_rate()
        params["components"]["skew_rate"] = tr_table.skew_rate()
        if baseline is not None and baseline.transit is not None:
            shift = _transit_shift(tr_table, baseline.transit)
            params["components"]["transit_shift"] = shift
            tr_term = 0.25 * _squash(shift)   # added after every other term, the repeat term included
    ex = err_ex = None
    if exemplars is not None:
        ex = ctx.edge_exemplars(exp.spans, int(exemplars))
        err_ex = ctx.edge_exemplars(exp.spans, int(exemplars), errors_only=True)
    if trace_step_s is None:
        if rep_term is not None:
            score = score + rep_term
        if tr_term is not None:
            score = score + tr_term
        return Features(exp.name, edges, Z, series, score, params, self_edges=self_edges,
                        spectrum=spec, cp_edges=cp_edges, shapes=census, error_origins=origins,
                        exemplars=ex, error_exemplars=err_ex, repeats=rep_table,
                        transit=tr_table)
    win, ts, mm0 = _trace_windows(exp.spans, ctx, trace_step_s, trace_W, trace_eps,
                                  trace_min_count, trace_quantile)
    tsq = _squash(ts)  # the metric term's squashing
    params["components"]["trace"] = tsq
    params.update(trace_step_s=trace_step_s, trace_W=trace_W, trace_eps=trace_eps,
                  trace_min_count=trace_min_count)
    if trace_quantile is not None:
        params["trace_quantile"] = int(trace_quantile)
    score = score + 0.25 * tsq
    load = None
    if trace_load:
        load, ls = _trace_load(exp.spans, ctx, trace_step_s, trace_W, trace_eps)
        lsq = _squash(ls)
        params["components"]["load"] = lsq
        params["trace_load"] = True
        score = score + 0.25 * lsq
    sc = None
    if symptom_corr:
        sc = _symptom_correlation(exp, ctx, win, mm0, trace_min_count, corr_min_pairs)
        params["components"]["symptom_corr"] = sc.service
        params["metric_corr_grid"] = sc.metric_grid
        if sc.metric_grid == "regular":
            params["components"]["metric_corr"] = sc.metric_service
    if rep_term is not None:
        score = score + rep_term
    if tr_term is not None:
        score = score + tr_term
    return Features(exp.name, edges, Z, series, score, params, symptom_corr=sc,
                    edge_windows=win, trace_window_scores=ts, self_edges=self_edges,
                    spectrum=spec, cp_edges=cp_edges, shapes=census, error_origins=origins,
                    edge_load=load, exemplars=ex, error_exemplars=err_ex, repeats=rep_table,
                    transit=tr_table)


def walk_graph(edges: EdgeTable, corr: np.ndarray, rho: float = 0.2
               ) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The correlation-weighted walk graph (the MonitorRank / MicroRCA family)
    as a CSR (row_ptr u32, col u32 ascending per row, w f32).  With c = corr +
    0.01, every cross-service pair i != j with count[i -> j] > 0 gives a
    forward edge i -> j of weight c[j] — the walk moves to the callees that
    follow the symptom — and a backward edge j -> i of weight rho * c[i];
    weights of coinciding edges are added.  Every node i gets a self edge of
    weight max(0, c[i] - max c[j] over its callees j), c[i] when it calls
    nobody — the walk stays where the correlation stops rising — dropped when
    its weight is 0."""
    S = edges.n_services
    c = np.asarray(corr, np.float64) + 0.01
    if c.shape != (S,):
        raise ValueError(f"walk_graph: corr of shape {c.shape} for {S} services")
    if not rho >= 0:
        raise ValueError(f"walk_graph: rho={rho} must be >= 0")
    calls = edges.count[: S * S].reshape(S, S) > 0
    calls[np.arange(S), np.arange(S)] = False
    w = np.zeros((S, S))
    has = calls | calls.T
    w += np.where(calls, c[None, :], 0.0)              # i -> j: c[j]
    w += np.where(calls.T, rho * c[None, :], 0.0)      # j -> i: rho * c[i]
    for i in range(S):
        out = np.nonzero(calls[i])[0]
        self_w = max(0.0, c[i] - c[out].max()) if out.size else c[i]
        if self_w > 0:
            has[i, i] = True
            w[i, i] = self_w
    row_ptr = np.zeros(S + 1, np.uint32)
    row_ptr[1:] = np.cumsum(has.sum(axis=1))
    rows, cols = np.nonzero(has)  # row-major: ascending columns per row
    return row_ptr, cols.astype(np.uint32), w[rows, cols].astype(np.float32)


def rank(feats: Features, *, walk: str = "calls", rho: float = 0.2, alpha: float = 0.85,
         iters: int = 100, tol: float = 1e-10,
         ctx: Context | None = None) -> list[tuple[str, float]]:
    """Root-cause ranking: personalized PageRank over the caller -> callee
    graph (weights = call counts), personalization = service anomaly scores
    (a non-finite score counts as 0; the uniform vector only when nothing
    positive remains).  walk="correlation" (needs features(symptom_corr=True))
    walks walk_graph(edges, symptom correlation per service, rho) instead: a
    busy but healthy callee no longer collects walk mass for its call count."""
    if walk not in ("calls", "correlation"):
        raise ValueError(f"rank(walk={walk!r}): \"calls\" or \"correlation\"")
    if walk == "correlation" and feats.symptom_corr is None:
        raise ValueError("rank(walk=\"correlation\") needs features(symptom_corr=True)")
    ctx = ctx or default_context()
    services = feats.edges.services
    if walk == "correlation":
        row_ptr, col, w = walk_graph(feats.edges, feats.symptom_corr.service, rho)
    else:
        row_ptr, col, w = feats.edges.call_graph()
    p = np.asarray(feats.service_scores, np.float64).copy()
    p = np.where(np.isfinite(p), p, 0.0)
    if p.sum() <= 0:
        p = np.ones(len(services))
    p = p + 1e-9 * p.sum()  # every node reachable by the restart
    x, _ = ctx.pagerank(row_ptr, col, w, p, alpha=alpha, iters=iters, tol=tol)
    order = np.argsort(-x, kind="stable")
    return [(services[i], float(x[i])) for i in order]


def hit_at(ranking: list[tuple[str, float]], target: str | None, k: int) -> float | math.nan:
    if target is None:
        return math.nan
    return 1.0 if target in [s for s, _ in ranking[:k]] else 0.0

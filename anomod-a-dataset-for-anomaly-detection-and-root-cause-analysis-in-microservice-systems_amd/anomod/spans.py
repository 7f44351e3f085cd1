"""Host containers: span sets (struct-of-arrays) and edge tables.

A :class:`SpanSet` is the columnar form of the spans the reference collectors
write one dict (or CSV row) at a time — jaeger_to_csv.py:76-90 for SN,
trace_collector.py:86-123 (SpanRecord.to_dict) for TT.  Spans are grouped by
trace: trace t owns rows [trace_ptr[t], trace_ptr[t+1]).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L


@dataclass
class SpanSet:
    services: list[str]
    trace_ptr: np.ndarray      # u64 [n_traces + 1]
    trace_hash: np.ndarray     # u64 [n_spans]
    span_id: np.ndarray        # u64 [n_spans]
    parent_span_id: np.ndarray  # u64 [n_spans]; 0 = no parent reference
    svc: np.ndarray            # u16 [n_spans]
    flags: np.ndarray          # u16 [n_spans]
    dur_us: np.ndarray         # u32 [n_spans]
    trace_ids: list[str] | None = None
    # span ids unique within every trace (the producer's declaration, or
    # check_unique_ids()): lets the GPU parent lookups scan from both ends
    unique_ids: bool = False
    # performance hints the library learns on the device at a set's first
    # aggregation (include/anomod.h anomod_spans_hints): parent-scan order
    # (1 collector order / 0 shuffled / -1 unknown) and histogram form (0 pair
    # / 1 compact / -1 unknown).  Context.upload hands them to every upload
    # and edge_aggregate keeps what was learned, so a host set that is
    # uploaded per call (features()) learns them once.  Results never depend
    # on them.
    scan_order: int = field(default=-1, compare=False)
    hist_form: int = field(default=-1, compare=False)
    _keep: list = field(default_factory=list, repr=False, compare=False)
    # span start times, epoch microseconds (0 = none recorded), or None: the
    # time axis of Context.edge_windows
    start_us: np.ndarray | None = field(default=None, compare=False)

    def __post_init__(self):
        self.trace_ptr = np.ascontiguousarray(self.trace_ptr, dtype=np.uint64)
        self.trace_hash = np.ascontiguousarray(self.trace_hash, dtype=np.uint64)
        self.span_id = np.ascontiguousarray(self.span_id, dtype=np.uint64)
        self.parent_span_id = np.ascontiguousarray(self.parent_span_id, dtype=np.uint64)
        self.svc = np.ascontiguousarray(self.svc, dtype=np.uint16)
        self.flags = np.ascontiguousarray(self.flags, dtype=np.uint16)
        self.dur_us = np.ascontiguousarray(self.dur_us, dtype=np.uint32)
        n = self.span_id.shape[0]
        for name in ("trace_hash", "parent_span_id", "svc", "flags", "dur_us"):
            if getattr(self, name).shape[0] != n:
                raise ValueError(f"SpanSet column {name} has {getattr(self, name).shape[0]} rows, "
                                 f"expected {n}")
        if self.trace_ptr.shape[0] < 1:
            raise ValueError("trace_ptr needs at least one entry")
        if self.start_us is not None:
            self.start_us = np.ascontiguousarray(self.start_us, dtype=np.uint64)
            if self.start_us.shape != (n,):
                raise ValueError(f"SpanSet column start_us has shape {self.start_us.shape}, "
                                 f"expected ({n},)")

    @property
    def n_spans(self) -> int:
        return int(self.span_id.shape[0])

    @property
    def n_traces(self) -> int:
        return int(self.trace_ptr.shape[0] - 1)

    @property
    def n_services(self) -> int:
        return len(self.services)

    def soa(self) -> L.SpanSoA:
        return L.SpanSoA(
            L.ptr(self.trace_hash, C.c_uint64), L.ptr(self.span_id, C.c_uint64),
            L.ptr(self.parent_span_id, C.c_uint64), L.ptr(self.svc, C.c_uint16),
            L.ptr(self.flags, C.c_uint16), L.ptr(self.dur_us, C.c_uint32))

    def check_unique_ids(self) -> bool:
        """Exact: no trace holds a span id twice (sets and returns
        unique_ids)."""
        if self.n_spans:
            t = self.trace_of_span()
            order = np.lexsort((self.span_id, t))
            ts, ids = t[order], self.span_id[order]
            self.unique_ids = not bool(np.any((ts[1:] == ts[:-1]) & (ids[1:] == ids[:-1])))
        else:
            self.unique_ids = True
        return self.unique_ids

    def trace_of_span(self) -> np.ndarray:
        """Trace index of every span (host helper)."""
        lens = np.diff(self.trace_ptr).astype(np.int64)
        return np.repeat(np.arange(self.n_traces, dtype=np.int64), lens)

    def select_traces(self, mask: np.ndarray) -> "SpanSet":
        """Sub-set of whole traces (trace order preserved)."""
        mask = np.asarray(mask, dtype=bool)
        lens = np.diff(self.trace_ptr).astype(np.int64)
        span_mask = np.repeat(mask, lens)
        new_ptr = np.zeros(int(mask.sum()) + 1, dtype=np.uint64)
        np.cumsum(lens[mask], out=new_ptr[1:])
        ids = None
        if self.trace_ids is not None:
            ids = [t for t, m in zip(self.trace_ids, mask) if m]
        return SpanSet(list(self.services), new_ptr, self.trace_hash[span_mask],
                       self.span_id[span_mask], self.parent_span_id[span_mask],
                       self.svc[span_mask], self.flags[span_mask], self.dur_us[span_mask], ids,
                       self.unique_ids,
                       start_us=None if self.start_us is None else self.start_us[span_mask])

    def shard(self, nshards: int, rank: int) -> "SpanSet":
        """Traces whose trace_hash % nshards == rank."""
        if self.n_traces == 0:
            return self.select_traces(np.zeros(0, dtype=bool))
        first = self.trace_ptr[:-1].astype(np.int64)
        lens = np.diff(self.trace_ptr).astype(np.int64)
        h = np.zeros(self.n_traces, dtype=np.uint64)
        nz = lens > 0
        h[nz] = self.trace_hash[first[nz]]
        return self.select_traces((h % np.uint64(nshards)) == np.uint64(rank))

    def observed_services(self) -> "SpanSet":
        """The same spans over only the services they name (names stay sorted,
        ids renumbered) — what a collector payload records as
        metadata.services_discovered = sorted(union of observed services),
        trace_collector.py:572."""
        used = np.unique(self.svc)
        if used.shape[0] == len(self.services):
            return self
        remap = np.zeros(len(self.services), np.uint16)
        remap[used] = np.arange(used.shape[0], dtype=np.uint16)
        return SpanSet([self.services[i] for i in used.tolist()], self.trace_ptr, self.trace_hash,
                       self.span_id, self.parent_span_id, remap[self.svc], self.flags,
                       self.dur_us, self.trace_ids, self.unique_ids, start_us=self.start_us)

    def take(self, order: np.ndarray, trace_ptr: np.ndarray) -> "SpanSet":
        """The spans in `order`, split into traces by `trace_ptr`."""
        return SpanSet(self.services, trace_ptr, self.trace_hash[order], self.span_id[order],
                       self.parent_span_id[order], self.svc[order], self.flags[order],
                       self.dur_us[order],
                       start_us=None if self.start_us is None else self.start_us[order])

    @staticmethod
    def concat(sets: list["SpanSet"]) -> "SpanSet":
        if not sets:
            raise ValueError("concat of no span sets")
        services = sets[0].services
        for s in sets[1:]:
            if s.services != services:
                raise ValueError("span sets with different service lists")
        lens = np.concatenate([np.diff(s.trace_ptr) for s in sets]).astype(np.uint64)
        ptr = np.zeros(lens.shape[0] + 1, dtype=np.uint64)
        np.cumsum(lens, out=ptr[1:])
        cat = lambda name: np.concatenate([getattr(s, name) for s in sets])  # noqa: E731
        ids = None
        if all(s.trace_ids is not None for s in sets):
            ids = [t for s in sets for t in s.trace_ids]
        return SpanSet(list(services), ptr, cat("trace_hash"), cat("span_id"),
                       cat("parent_span_id"), cat("svc"), cat("flags"), cat("dur_us"), ids,
                       all(s.unique_ids for s in sets),
                       start_us=(cat("start_us") if all(s.start_us is not None for s in sets)
                                 else None))


def edge_rows(n_services: int) -> int:
    return (n_services + L.ROOT_ROWS) * n_services


@dataclass
class EdgeTable:
    """Per (parent service -> child service) edge aggregate.

    Row r = p * S + c; p == S is ROOT (no parent reference), p == S + 1 is
    ORPHAN (parent reference not found in the trace)."""

    services: list[str]
    count: np.ndarray    # u64 [E]
    errors: np.ndarray   # u64 [E]
    sum_us: np.ndarray   # u64 [E]
    min_us: np.ndarray   # u32 [E]
    max_us: np.ndarray   # u32 [E]
    p50_us: np.ndarray   # f64 [E]
    p99_us: np.ndarray   # f64 [E]
    hist: np.ndarray | None = None  # u64 [E, HIST_BINS]

    @property
    def n_services(self) -> int:
        return len(self.services)

    @staticmethod
    def empty(services: list[str], with_hist: bool = True) -> "EdgeTable":
        E = edge_rows(len(services))
        return EdgeTable(list(services), np.zeros(E, np.uint64), np.zeros(E, np.uint64),
                         np.zeros(E, np.uint64), np.full(E, 0xFFFFFFFF, np.uint32),
                         np.zeros(E, np.uint32), np.full(E, np.nan), np.full(E, np.nan),
                         np.zeros((E, L.HIST_BINS), np.uint64) if with_hist else None)

    def c_struct(self) -> L.EdgeTableC:
        return L.EdgeTableC(
            self.n_services, L.HIST_BINS, L.ptr(self.count, C.c_uint64),
            L.ptr(self.errors, C.c_uint64), L.ptr(self.sum_us, C.c_uint64),
            L.ptr(self.min_us, C.c_uint32), L.ptr(self.max_us, C.c_uint32),
            L.ptr(self.hist, C.c_uint64), L.ptr(self.p50_us, C.c_double),
            L.ptr(self.p99_us, C.c_double))

    def parent_name(self, p: int) -> str:
        S = self.n_services
        return "ROOT" if p == S else "ORPHAN" if p == S + 1 else self.services[p]

    def records(self) -> list[dict]:
        """Non-empty edges as dicts (parent, child, count, errors, mean/p50/p99)."""
        S = self.n_services
        out = []
        for r in np.nonzero(self.count)[0]:
            p, c = divmod(int(r), S)
            n = int(self.count[r])
            out.append({
                "parent": self.parent_name(p), "child": self.services[c], "count": n,
                "errors": int(self.errors[r]), "mean_us": int(self.sum_us[r]) / n,
                "min_us": int(self.min_us[r]), "max_us": int(self.max_us[r]),
                "p50_us": float(self.p50_us[r]), "p99_us": float(self.p99_us[r]),
            })
        return out

    def call_graph(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Cross-service caller -> callee CSR (self edges, ROOT, ORPHAN dropped);
        weight = call count."""
        S = self.n_services
        cnt = self.count[: S * S].reshape(S, S).astype(np.float64)
        np.fill_diagonal(cnt, 0.0)
        row_ptr = np.zeros(S + 1, dtype=np.uint32)
        cols, ws = [], []
        for p in range(S):
            nz = np.nonzero(cnt[p])[0]
            cols.extend(nz.tolist())
            ws.extend(cnt[p, nz].tolist())
            row_ptr[p + 1] = len(cols)
        return row_ptr, np.asarray(cols, dtype=np.uint32), np.asarray(ws, dtype=np.float32)


@dataclass
class EdgeWindows:
    """Per-window edge table of a span set with start times
    (anomod_edge_windows_spans): window w covers starts in
    [t0_us + w * step_us, t0_us + (w + 1) * step_us); rows as in EdgeTable."""

    services: list[str]
    t0_us: int
    step_us: int
    count: np.ndarray    # u64 [T, E]
    errors: np.ndarray   # u64 [T, E]
    sum_us: np.ndarray   # u64 [T, E]
    max_us: np.ndarray   # u32 [T, E]; 0 for an empty cell
    outside: int = 0     # spans that start before t0_us or at / after the last window's end
    # Context.edge_window_quantiles: the exact per-cell order statistics
    # sorted(x)[int(c * q / 100)] and the cell counts they were taken over
    q_pct: tuple | None = None
    q_us: np.ndarray | None = None      # u32 [T, E, nq]; 0 for an empty cell
    q_count: np.ndarray | None = None   # u64 [T, E]

    @property
    def n_windows(self) -> int:
        return int(self.count.shape[0])

    @staticmethod
    def empty(services: list[str], t0_us: int, step_us: int, n_windows: int) -> "EdgeWindows":
        shape = (n_windows, edge_rows(len(services)))
        return EdgeWindows(list(services), int(t0_us), int(step_us), np.zeros(shape, np.uint64),
                           np.zeros(shape, np.uint64), np.zeros(shape, np.uint64),
                           np.zeros(shape, np.uint32))

    def matrix(self, min_count: int = 5, quantile: int | None = None):
        """The table as a time-major series matrix for the EWMA/z kernels: the
        active edges (non-zero total count, ascending row) give two f32
        columns each, log2(1 + count) and log2(1 + sum_us / count) (NaN where
        the window holds fewer than min_count spans of the edge), computed in
        f64.  Series keys: ("edge_count" | "edge_mean_us", (("parent", name),
        ("child", name))); timestamps are the window starts in epoch seconds.
        With quantile=q (a percentage of q_pct: Context.edge_window_quantiles)
        every active edge gets a third column, log2(1 + q_us) of that
        percentage (NaN where the cell holds fewer than min_count spans), key
        ("edge_p<q>_us", labels)."""
        from .decode import MetricMatrix

        S = len(self.services)
        T = self.n_windows
        cols = 2
        if quantile is not None:
            if self.q_pct is None or self.q_us is None or self.q_count is None:
                raise ValueError("matrix(quantile=...): the table holds no quantiles "
                                 "(Context.edge_window_quantiles)")
            if int(quantile) not in [int(q) for q in self.q_pct]:
                raise ValueError(f"matrix(quantile={quantile}): not among q_pct={self.q_pct}")
            kq = [int(q) for q in self.q_pct].index(int(quantile))
            cols = 3
        active = np.nonzero(self.count.sum(axis=0))[0]
        cnt = self.count[:, active].astype(np.float64)
        tot = self.sum_us[:, active].astype(np.float64)
        X = np.empty((T, cols * active.shape[0]), np.float32)
        X[:, 0::cols] = np.log2(1.0 + cnt)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(self.count[:, active] >= max(int(min_count), 1),
                            np.log2(1.0 + tot / cnt), np.nan)
        X[:, 1::cols] = mean
        if cols == 3:
            X[:, 2::3] = np.where(self.q_count[:, active] >= max(int(min_count), 1),
                                  np.log2(1.0 + self.q_us[:, active, kq].astype(np.float64)),
                                  np.nan)
        series = []
        for r in active.tolist():
            p, c = divmod(r, S)
            name = "ROOT" if p == S else "ORPHAN" if p == S + 1 else self.services[p]
            labels = (("parent", name), ("child", self.services[c]))
            series += [("edge_count", labels), ("edge_mean_us", labels)]
            if cols == 3:
                series.append((f"edge_p{int(quantile)}_us", labels))
        ts = (self.t0_us + np.arange(T, dtype=np.float64) * self.step_us) / 1e6
        return MetricMatrix(X, ts, series)

    def symptom(self, min_count: int = 5) -> np.ndarray:
        """The front-door latency series, f32 [T]: per window log2(1 + sum of
        sum_us / sum of count) over the ROOT rows (parent index S: the spans
        that entered the system), computed in f64; NaN where the window holds
        fewer than max(min_count, 1) such spans."""
        S = len(self.services)
        cnt = self.count[:, S * S:S * S + S].sum(axis=1)
        tot = self.sum_us[:, S * S:S * S + S].sum(axis=1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.where(cnt >= max(int(min_count), 1),
                         np.log2(1.0 + tot / cnt.astype(np.float64)), np.nan)
        return y.astype(np.float32)


@dataclass
class EdgeLoad:
    """Per-window edge load of a span set with start times
    (anomod_edge_load_spans): for window w = [t0_us + w * step_us, t0_us +
    (w + 1) * step_us) and an edge row, busy_us is the time the edge's calls
    were open inside the window (busy_us / step_us = the mean number in
    flight) and carried the calls still open when the window opens.  A call is
    followed for as long as it lasts, where EdgeWindows books it in the window
    it starts in only.  Rows as in EdgeTable."""

    services: list[str]
    t0_us: int
    step_us: int
    busy_us: np.ndarray   # u64 [T, E]
    carried: np.ndarray   # u64 [T, E]
    outside: int = 0      # spans in traces that touch no window: dur 0, or wholly before / after

    @property
    def n_windows(self) -> int:
        return int(self.busy_us.shape[0])

    @staticmethod
    def empty(services: list[str], t0_us: int, step_us: int, n_windows: int) -> "EdgeLoad":
        shape = (n_windows, edge_rows(len(services)))
        return EdgeLoad(list(services), int(t0_us), int(step_us), np.zeros(shape, np.uint64),
                        np.zeros(shape, np.uint64))

    def active_rows(self) -> np.ndarray:
        """The edge rows with a non-zero busy or carried total, ascending."""
        return np.nonzero((self.busy_us != 0).any(axis=0) | (self.carried != 0).any(axis=0))[0]

    def matrix(self):
        """The table as a time-major series matrix for the EWMA/z kernels: one
        f32 column per active edge (active_rows), log2(1 + busy_us) computed
        in f64.  No NaNs: an idle window is a 0, which is information here.
        Series keys: ("edge_busy_us", (("parent", name), ("child", name)));
        timestamps are the window starts in epoch seconds."""
        from .decode import MetricMatrix

        S = len(self.services)
        T = self.n_windows
        active = self.active_rows()
        X = np.log2(1.0 + self.busy_us[:, active].astype(np.float64)).astype(np.float32)
        series = []
        for r in active.tolist():
            p, c = divmod(r, S)
            name = "ROOT" if p == S else "ORPHAN" if p == S + 1 else self.services[p]
            series.append(("edge_busy_us", (("parent", name), ("child", self.services[c]))))
        ts = (self.t0_us + np.arange(T, dtype=np.float64) * self.step_us) / 1e6
        return MetricMatrix(X, ts, series)


U64_MAX = 0xFFFFFFFFFFFFFFFF


@dataclass
class EdgeExemplars:
    """The k slowest calls of every edge row (anomod_edge_exemplars_spans),
    all spans (which = 0) or the error-flagged ones (which = 1): row r holds
    n_found[r] exemplars in slots [r, 0 .. n_found[r]), ordered by dur_us
    descending, then span position ascending — ties go by position, so the
    table is a pure function of the set.  An unused slot holds position and
    trace 2^64 - 1 and zeros elsewhere.  Rows as in EdgeTable."""

    services: list[str]
    k: int
    which: int
    n_found: np.ndarray    # u32 [E]
    position: np.ndarray   # u64 [E, K] span position
    trace: np.ndarray      # u64 [E, K] trace index
    span_id: np.ndarray    # u64 [E, K]
    dur_us: np.ndarray     # u32 [E, K]
    flags: np.ndarray      # u16 [E, K]
    start_us: np.ndarray   # u64 [E, K]; 0 when the set has no start column

    COLUMNS = ("position", "trace", "span_id", "dur_us", "flags", "start_us")

    @staticmethod
    def empty(services: list[str], k: int, which: int = 0) -> "EdgeExemplars":
        """The table of a set without spans: nothing found, every slot unused."""
        shape = (edge_rows(len(services)), int(k))
        return EdgeExemplars(list(services), int(k), int(which),
                             np.zeros(shape[0], np.uint32), np.full(shape, U64_MAX, np.uint64),
                             np.full(shape, U64_MAX, np.uint64), np.zeros(shape, np.uint64),
                             np.zeros(shape, np.uint32), np.zeros(shape, np.uint16),
                             np.zeros(shape, np.uint64))

    def c_struct(self) -> L.EdgeExemplarsC:
        return L.EdgeExemplarsC(
            len(self.services), self.k, self.which, L.ptr(self.n_found, C.c_uint32),
            L.ptr(self.position, C.c_uint64), L.ptr(self.trace, C.c_uint64),
            L.ptr(self.span_id, C.c_uint64), L.ptr(self.dur_us, C.c_uint32),
            L.ptr(self.flags, C.c_uint16), L.ptr(self.start_us, C.c_uint64))

    def row(self, parent: str, child: str) -> int:
        """Edge row of (parent service -> child service) by name; parent
        "ROOT" / "ORPHAN" as EdgeTable.parent_name spells them."""
        S = len(self.services)
        p = S if parent == "ROOT" else S + 1 if parent == "ORPHAN" else self.services.index(parent)
        return p * S + self.services.index(child)

    def trace_indices(self, row: int) -> np.ndarray:
        """Trace index of each exemplar of the row, slowest first (a trace
        that holds several of them appears several times)."""
        return self.trace[row, : int(self.n_found[row])].astype(np.int64)

    def trace_ids(self, spans: SpanSet, row: int) -> list[str]:
        """Trace id of each exemplar of the row: SpanSet.trace_ids when the
        set carries them, else the trace_hash of the trace's first span as 16
        hex digits."""
        idx = self.trace_indices(row).tolist()
        if spans.trace_ids is not None:
            return [spans.trace_ids[t] for t in idx]
        return [f"{int(spans.trace_hash[int(spans.trace_ptr[t])]):016x}" for t in idx]

    def select(self, spans: SpanSet, row: int) -> SpanSet:
        """The exemplar traces of the row as a span set (SpanSet.select_traces:
        whole traces, in trace order)."""
        mask = np.zeros(spans.n_traces, bool)
        mask[self.trace_indices(row)] = True
        return spans.select_traces(mask)


@dataclass
class CriticalPath:
    """Critical path of a span set with start times
    (anomod_edge_critical_path_spans): the edge table of the on-path spans
    over their cp_us (exclusive time on the path) and, when asked for, the
    per-span columns by span position."""

    edges: EdgeTable
    cp_us: np.ndarray | None = None     # u32 [n_spans]
    on_path: np.ndarray | None = None   # u8  [n_spans]

    def service_share(self) -> np.ndarray:
        """Per child service: its share of the critical-path time of the whole
        table (zeros for an empty table)."""
        S = self.edges.n_services
        per = self.edges.sum_us.reshape(S + 2, S).sum(axis=0).astype(np.float64)
        tot = per.sum()
        return per / tot if tot > 0 else np.zeros(S)


U32_MAX = 0xFFFFFFFF


def _ochiai(ef: np.ndarray, ep: np.ndarray, F: int) -> np.ndarray:
    """ef / sqrt(F * (ef + ep)) in float64, 0 where the denominator is 0."""
    ef = ef.astype(np.float64)
    den = np.sqrt(float(F) * (ef + ep.astype(np.float64)))
    return np.divide(ef, den, out=np.zeros(ef.shape[0]), where=den > 0)


@dataclass
class TraceSpectrum:
    """Abnormal / normal trace labels of a span set and the per-class trace
    coverage of services and edge rows (anomod_trace_spectrum_spans): a span
    is bad when dur_us > thr_us[its edge row] or, with use_errors, when it
    carries the error flag; a trace is abnormal (class 1) when any of its
    spans is bad.  Rows as in EdgeTable."""

    services: list[str]
    n_traces: np.ndarray              # u64 [2] traces per class
    svc_traces: np.ndarray            # u64 [2, S] traces of the class holding the service
    edge_traces: np.ndarray           # u64 [2, E] the same per edge row
    bad_spans: np.ndarray             # u64 [E] bad spans per row
    trace_abnormal: np.ndarray | None  # u8 [n_traces] class of each trace
    thr_us: np.ndarray | None         # u32 [E] the thresholds used (None: none)
    use_errors: bool = True

    def ochiai(self) -> np.ndarray:
        """Per service: ef / sqrt(F * (ef + ep)) with ef / ep the abnormal /
        normal traces holding the service and F the abnormal traces."""
        return _ochiai(self.svc_traces[1], self.svc_traces[0], int(self.n_traces[1]))

    def edge_ochiai(self) -> np.ndarray:
        """ochiai() per edge row."""
        return _ochiai(self.edge_traces[1], self.edge_traces[0], int(self.n_traces[1]))


@dataclass
class TraceShapes:
    """Shape census of a span set (anomod_trace_shapes_spans): the distinct
    trace shapes — 64-bit fingerprints of the multiset of labelled
    root-to-span call paths of a trace — by count descending, then value
    ascending.  The arrays hold the first min(cap, n_shapes) shapes."""

    services: list[str]
    shape: np.ndarray                 # u64 [m] the fingerprints
    count: np.ndarray                 # u64 [m] traces with the shape
    abnormal: np.ndarray              # u64 [m] those with trace_class != 0
    first_trace: np.ndarray           # u64 [m] smallest trace index with the shape
    n_shapes: int                     # distinct shapes of the set
    off_tree_spans: int               # spans whose parent chain reaches no head
    trace_shape: np.ndarray | None = None  # u64 [n_traces] (per_trace=True)
    path_hash: np.ndarray | None = None    # u64 [n_spans] (per_span=True)
    use_errors: bool = False

    @property
    def truncated(self) -> bool:
        """The census holds fewer shapes than the set has (cap < n_shapes)."""
        return int(self.shape.shape[0]) < int(self.n_shapes)

    def novel(self, baseline: "TraceShapes") -> np.ndarray:
        """Mask of the shapes absent from baseline.shape.  A truncated
        baseline cannot say that a shape is absent: ValueError."""
        if baseline.truncated:
            raise ValueError("the baseline census is truncated "
                             f"({baseline.shape.shape[0]} of {baseline.n_shapes} shapes)")
        return ~np.isin(self.shape, baseline.shape)

    def service_sets(self, spans: SpanSet) -> np.ndarray:
        """bool [m, S]: the services of each shape's exemplar trace
        (first_trace), over all spans of that trace."""
        S = len(self.services)
        out = np.zeros((self.shape.shape[0], S), bool)
        ptr = spans.trace_ptr
        for k, t in enumerate(self.first_trace.tolist()):
            out[k, spans.svc[int(ptr[t]):int(ptr[t + 1])]] = True
        return out

    def novelty(self, spans: SpanSet, baseline: "TraceShapes") -> np.ndarray:
        """Per service s: the traces of novel shapes whose exemplar holds s
        over the traces of all shapes whose exemplar holds s (0 where no
        exemplar holds s)."""
        holds = self.service_sets(spans).astype(np.float64)
        cnt = self.count.astype(np.float64)
        num = (cnt * self.novel(baseline)) @ holds
        den = cnt @ holds
        return np.divide(num, den, out=np.zeros(holds.shape[1]), where=den > 0)


ERR_CLEAN, ERR_ORIGIN, ERR_PROPAGATED, ERR_ABSORBER = 0, 1, 2, 3
FATE_SURFACED, FATE_CONTAINED, FATE_LOOP = 1, 2, 3


@dataclass
class ErrorOrigins:
    """Error origins of a span set (anomod_error_origins_spans): every
    error-flagged span is the place its failure started (ORIGIN: no failing
    callee) or a place it passed through (PROPAGATED), a span without the flag
    whose callee failed is an ABSORBER; a failure follows its chain of failing
    callers and is SURFACED (the chain ends at a trace head), CONTAINED (it
    ends below a caller that did not fail) or in a LOOP (a reference cycle).
    Rows as in EdgeTable; origin + propagated equals EdgeTable.errors."""

    services: list[str]
    origin: np.ndarray                # u64 [E] ORIGIN spans
    propagated: np.ndarray            # u64 [E] PROPAGATED spans
    stopped: np.ndarray               # u64 [E] error spans at the top of a CONTAINED chain
    surfaced: np.ndarray              # u64 [E] ORIGIN spans of fate SURFACED
    absorbers: np.ndarray             # u64 [E] ABSORBER spans
    hops_sum: np.ndarray              # u64 [E] hops of the ORIGIN spans
    hops_max: np.ndarray              # u32 [E] (0 for a row without an ORIGIN span)
    error_spans: int = 0              # error-flagged spans in traces
    loop_spans: int = 0               # those of fate LOOP
    span_state: np.ndarray | None = None  # u8 [n_spans] class | fate << 2 (per_span=True)
    span_hops: np.ndarray | None = None   # u32 [n_spans] (per_span=True)

    TABLES = ("origin", "propagated", "stopped", "surfaced", "absorbers", "hops_sum", "hops_max")

    @staticmethod
    def empty(services: list[str], n_spans: int | None = None) -> "ErrorOrigins":
        """Zeroed tables over `services`; n_spans: also the per-span columns."""
        E = edge_rows(len(services))
        return ErrorOrigins(list(services), *(np.zeros(E, np.uint64) for _ in range(6)),
                            np.zeros(E, np.uint32), 0, 0,
                            None if n_spans is None else np.zeros(n_spans, np.uint8),
                            None if n_spans is None else np.zeros(n_spans, np.uint32))

    def per_service(self, name: str) -> np.ndarray:
        """A table summed over the parent rows: one value per child service
        (the maximum for hops_max)."""
        S = len(self.services)
        t = getattr(self, name).reshape(S + 2, S)
        return t.max(axis=0) if name == "hops_max" else t.sum(axis=0)

    def origin_rate(self, count: np.ndarray) -> np.ndarray:
        """Per service: the failures that started in it over the spans it
        served — origin summed over the parent rows, divided by the service's
        span count (count: u64 [E] as EdgeTable.count, or [S] per service); 0
        where the count is 0."""
        S = len(self.services)
        cnt = np.asarray(count)
        if cnt.shape == (edge_rows(S),):
            cnt = cnt.reshape(S + 2, S).sum(axis=0)
        elif cnt.shape != (S,):
            raise ValueError(f"count has shape {cnt.shape}, expected ({edge_rows(S)},) or ({S},)")
        cnt = cnt.astype(np.float64)
        return np.divide(self.per_service("origin").astype(np.float64), cnt, out=np.zeros(S),
                         where=cnt > 0)

    def surfaced_share(self) -> np.ndarray:
        """Per service: the share of the failures that started in it and
        reached their trace's entry (surfaced / origin); 0 where origin is 0."""
        S = len(self.services)
        org = self.per_service("origin").astype(np.float64)
        return np.divide(self.per_service("surfaced").astype(np.float64), org, out=np.zeros(S),
                         where=org > 0)

    def mean_hops(self) -> np.ndarray:
        """Per service: the mean number of failing callers above a failure that
        started in it (hops_sum / origin); 0 where origin is 0."""
        S = len(self.services)
        org = self.per_service("origin").astype(np.float64)
        return np.divide(self.per_service("hops_sum").astype(np.float64), org, out=np.zeros(S),
                         where=org > 0)


@dataclass
class CallRepeats:
    """Call repeats of a span set (anomod_call_repeats_spans): a group is one
    parent span's calls to one callee service, n its size and e its
    error-flagged members.  The edge table counts spans; groups counts the
    logical calls behind them, repeats the calls beyond the first of a group.
    Rows as in EdgeTable; only the first S * S rows hold groups (a head has no
    parent), and groups + repeats there equals EdgeTable.count for a set
    without a self-referencing span."""

    services: list[str]
    groups: np.ndarray                # u64 [E] groups (logical calls)
    repeats: np.ndarray               # u64 [E] sum of n - 1
    repeated: np.ndarray              # u64 [E] groups with n >= 2
    retried: np.ndarray               # u64 [E] ... and e >= 1
    recovered: np.ndarray             # u64 [E] ... and 1 <= e < n
    exhausted: np.ndarray             # u64 [E] ... and e == n
    after_error: np.ndarray           # u64 [E] members that started after a failure of their group ended
    size_hist: np.ndarray             # u64 [E, REPEAT_BINS] groups by min(floor(log2 n), 7)
    size_max: np.ndarray              # u32 [E] largest n (0 for a row without a group)
    grouped_spans: int = 0            # spans that have a parent
    max_size: int = 0                 # the largest group of the set
    timed: bool = False               # the set has start times (else after_error is all zero)
    span_group_size: np.ndarray | None = None   # u32 [n_spans] (per_span=True)
    span_after_error: np.ndarray | None = None  # u8 [n_spans] (per_span=True)

    TABLES = ("groups", "repeats", "repeated", "retried", "recovered", "exhausted", "after_error",
              "size_hist", "size_max")

    @staticmethod
    def empty(services: list[str], n_spans: int | None = None) -> "CallRepeats":
        """Zeroed tables over `services`; n_spans: also the per-span columns."""
        E = edge_rows(len(services))
        return CallRepeats(list(services), *(np.zeros(E, np.uint64) for _ in range(7)),
                           np.zeros((E, L.REPEAT_BINS), np.uint64), np.zeros(E, np.uint32), 0, 0,
                           False,
                           None if n_spans is None else np.zeros(n_spans, np.uint32),
                           None if n_spans is None else np.zeros(n_spans, np.uint8))

    def per_service(self, name: str) -> np.ndarray:
        """A table summed over the parent rows: one value per callee service
        (the maximum for size_max; [S, REPEAT_BINS] for size_hist)."""
        S = len(self.services)
        t = getattr(self, name)
        t = t.reshape((S + 2, S) + t.shape[1:])
        return t.max(axis=0) if name == "size_max" else t.sum(axis=0)

    def amplification(self) -> np.ndarray:
        """Per edge row: spans per logical call, (groups + repeats) / groups;
        1 where the row has no group."""
        g = self.groups.astype(np.float64)
        return np.divide(g + self.repeats.astype(np.float64), g, out=np.ones(g.shape[0]),
                         where=g > 0)


@dataclass
class CallTransit:
    """Call transit of a span set (anomod_call_transit_spans): for a call whose
    parent span made no other call (a client / exit span and the callee's
    server / entry span), the request gap from the parent's start to the
    call's start and the response gap from the call's end to the parent's.
    Rows as in EdgeTable; only the first S * S rows hold calls.  A call that
    starts before its parent is early (clock skew), one that ends after it is
    late (abandoned: the caller gave up first); neither leaves a record."""

    services: list[str]
    request: EdgeTable                # the request gaps of the recorded calls
    response: EdgeTable               # the response gaps
    untimed: np.ndarray               # u64 [E] paired calls with a start of 0 on either side
    early: np.ndarray                 # u64 [E] paired, timed calls that start before their parent
    late: np.ndarray                  # u64 [E] paired, timed calls that end after their parent
    early_us: np.ndarray              # u64 [E] by how much, summed (each clamped to 2^32 - 1)
    late_us: np.ndarray               # u64 [E]
    calls: int = 0                    # spans that have a parent
    paired: int = 0                   # ... whose parent made no other call
    span_req_us: np.ndarray | None = None   # u32 [n_spans] (per_span=True)
    span_resp_us: np.ndarray | None = None  # u32 [n_spans] (per_span=True)
    span_state: np.ndarray | None = None    # u8 [n_spans] TRANSIT_* bits (per_span=True)

    TABLES = ("untimed", "early", "late", "early_us", "late_us")

    @staticmethod
    def empty(services: list[str], with_hist: bool = True,
              n_spans: int | None = None) -> "CallTransit":
        """Empty tables over `services`; n_spans: also the per-span columns."""
        E = edge_rows(len(services))
        return CallTransit(list(services), EdgeTable.empty(services, with_hist),
                           EdgeTable.empty(services, with_hist),
                           *(np.zeros(E, np.uint64) for _ in range(5)), 0, 0,
                           None if n_spans is None else np.zeros(n_spans, np.uint32),
                           None if n_spans is None else np.zeros(n_spans, np.uint32),
                           None if n_spans is None else np.zeros(n_spans, np.uint8))

    def paired_rows(self) -> np.ndarray:
        """u64 [E]: the paired calls of every row (request.count + early + untimed)."""
        return self.request.count + self.early + self.untimed

    def per_service(self, name: str) -> np.ndarray:
        """A u64 [E] array summed over the parent rows of the cross-service
        rows (p < S, p != c): one value per callee service.  name: one of
        TABLES, "paired", or a table field as "request.count" /
        "response.sum_us"."""
        S = len(self.services)
        if name == "paired":
            t = self.paired_rows()
        elif "." in name:
            tab, field = name.split(".", 1)
            if tab not in ("request", "response") or field not in ("count", "errors", "sum_us"):
                raise ValueError(f"per_service({name!r}): no such summable table")
            t = getattr(getattr(self, tab), field)
        elif name in self.TABLES:
            t = getattr(self, name)
        else:
            raise ValueError(f"per_service({name!r}): no such summable table")
        t = t[:S * S].reshape(S, S).copy()
        np.fill_diagonal(t, 0)
        return t.sum(axis=0)

    def skew_rate(self) -> np.ndarray:
        """Per callee service over the cross-service rows: early / (request
        records + early), the share of the timed calls into it that start
        before their caller; 0 where there is none."""
        e = self.per_service("early").astype(np.float64)
        d = e + self.per_service("request.count").astype(np.float64)
        return np.divide(e, d, out=np.zeros(len(self.services)), where=d > 0)

    def abandoned_rate(self) -> np.ndarray:
        """Per callee service over the cross-service rows: late / (response
        records + late), the share of the timed calls into it whose caller
        ended first; 0 where there is none."""
        l = self.per_service("late").astype(np.float64)
        d = l + self.per_service("response.count").astype(np.float64)
        return np.divide(l, d, out=np.zeros(len(self.services)), where=d > 0)


def spectrum_thresholds(base: EdgeTable, services: list[str], *, rows: str = "root",
                        min_count: int = 10) -> np.ndarray:
    """Latency thresholds (u32 [E] over `services`) for Context.trace_spectrum
    from a baseline run's edge table: floor(base.p99_us) of the same edge —
    matched by service NAMES, as the latency term matches them — where the
    baseline edge holds >= min_count spans and a finite p99, else UINT32_MAX
    (never fires).  rows="root" sets only the ROOT rows (trace entry spans: their
    duration is the trace's end-to-end latency), rows="all" every row."""
    if rows not in ("root", "all"):
        raise ValueError(f"rows={rows!r}: 'root' or 'all'")
    S, Sb = len(services), base.n_services
    pos = {s: i for i, s in enumerate(base.services)}
    m = np.array([pos.get(s, -1) for s in services] + [Sb, Sb + 1], np.int64)  # + ROOT, ORPHAN
    p_cur = np.repeat(np.arange(S + 2), S)
    pb, cb = m[p_cur], m[np.tile(np.arange(S), S + 2)]
    have = (pb >= 0) & (cb >= 0)
    if rows == "root":
        have &= p_cur == S
    brow = np.where(have, pb * Sb + cb, 0)
    p99 = np.where(have, base.p99_us[brow], np.nan)
    ok = have & (base.count[brow] >= min_count) & np.isfinite(p99)
    thr = np.full(edge_rows(S), U32_MAX, np.uint32)
    thr[ok] = np.minimum(np.floor(p99[ok]), float(U32_MAX)).astype(np.uint32)
    return thr


@dataclass
class TraceStructure:
    """Per-span / per-trace structure of a span set (trace_collector.py:401-481,
    536-547; see anomod_trace_structure in include/anomod.h)."""

    services: list[str]
    parent_pos: np.ndarray   # u32 [n_spans] position of the node's parent in its trace
    depth: np.ndarray        # u32 [n_spans]
    n_children: np.ndarray   # u32 [n_spans]
    span_flags: np.ndarray   # u8  [n_spans] SPAN_ROOT | SPAN_FIRST
    n_roots: np.ndarray      # u32 [n_traces]
    svc_mask: np.ndarray     # u64 [n_traces, ceil(S/64)]

    @staticmethod
    def empty(services: list[str], n_spans: int, n_traces: int) -> "TraceStructure":
        w = (len(services) + 63) // 64
        return TraceStructure(list(services), np.zeros(n_spans, np.uint32),
                              np.zeros(n_spans, np.uint32), np.zeros(n_spans, np.uint32),
                              np.zeros(n_spans, np.uint8), np.zeros(n_traces, np.uint32),
                              np.zeros((n_traces, w), np.uint64))

    def c_struct(self) -> L.TraceStructC:
        return L.TraceStructC(len(self.services), L.ptr(self.parent_pos, C.c_uint32),
                              L.ptr(self.depth, C.c_uint32), L.ptr(self.n_children, C.c_uint32),
                              L.ptr(self.span_flags, C.c_uint8), L.ptr(self.n_roots, C.c_uint32),
                              L.ptr(self.svc_mask, C.c_uint64))

    def services_involved(self, t: int) -> list[str]:
        """Sorted service names of trace t (trace_collector.py:536)."""
        m = self.svc_mask[t]
        return [s for i, s in enumerate(self.services) if (int(m[i // 64]) >> (i % 64)) & 1]

    def root_positions(self, trace_ptr: np.ndarray, t: int) -> list[int]:
        """Trace-local positions of the root nodes of trace t, in first-seen
        order (root_span_node_ids, trace_collector.py:443, 544)."""
        a, b = int(trace_ptr[t]), int(trace_ptr[t + 1])
        fl = self.span_flags[a:b]
        return [k for k in range(b - a) if fl[k] == (L.SPAN_ROOT | L.SPAN_FIRST)]

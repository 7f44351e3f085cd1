"""Device context: one HIP device + stream (+ optional RCCL communicator).

Thin object layer over the C ABI; every compute method runs a hand-written
HIP kernel in libanomod.so.  Nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .spans import (CallRepeats, CallTransit, CriticalPath, EdgeExemplars, EdgeLoad, EdgeTable, EdgeWindows, ErrorOrigins, SpanSet,
                    TraceShapes, TraceSpectrum, TraceStructure, edge_rows)


@dataclass
class SynthSpec:
    """Synthetic workload: topology 'SN' or 'TT' (or 'LONG':
    SN services in traces of 16..4000 spans, the length / depth stress case)."""

    topology: str = "SN"
    seed: int = 20251103
    fault_service: str | int | None = None
    fault_latency_mult: int = 8
    p_error_ppm: int = 5000          # 0.5 % base error rate
    p_fault_error_ppm: int = 200000  # 20 % on the faulty service
    p_orphan_ppm: int = 0

    @property
    def topo_id(self) -> int:
        return {"SN": L.TOPO_SN, "TT": L.TOPO_TT, "LONG": L.TOPO_LONG}[self.topology.upper()]

    def services(self) -> list[str]:
        return synth_services(self.topology)

    def c_struct(self) -> L.SynthSpec:
        fault = 0xFFFFFFFF
        if self.fault_service is not None:
            fault = (self.services().index(self.fault_service)
                     if isinstance(self.fault_service, str) else int(self.fault_service))
        return L.SynthSpec(self.topo_id, fault, self.seed, self.fault_latency_mult,
                           self.p_error_ppm, self.p_fault_error_ppm, self.p_orphan_ppm)


def synth_services(topology: str) -> list[str]:
    lib = L.lib()
    tid = {"SN": L.TOPO_SN, "TT": L.TOPO_TT, "LONG": L.TOPO_LONG}[topology.upper()]
    n = C.c_uint32()
    L.check(lib.anomod_synth_n_services(tid, C.byref(n)))
    return [lib.anomod_synth_service_name(tid, i).decode() for i in range(n.value)]


def synth_generate_host(spec: SynthSpec, n_traces: int, shard: int = 0) -> SpanSet:
    """Generate a synthetic span set on the host (same generator as the GPU)."""
    lib = L.lib()
    cs = spec.c_struct()
    n = C.c_uint64()
    L.check(lib.anomod_synth_count_host(C.byref(cs), shard, n_traces, C.byref(n)))
    ns = n.value
    arr = dict(trace_hash=np.empty(ns, np.uint64), span_id=np.empty(ns, np.uint64),
               parent_span_id=np.empty(ns, np.uint64), svc=np.empty(ns, np.uint16),
               flags=np.empty(ns, np.uint16), dur_us=np.empty(ns, np.uint32))
    ptr = np.empty(n_traces + 1, np.uint64)
    L.check(lib.anomod_synth_generate_host(C.byref(cs), shard, n_traces,
                                           C.byref(_soa_out(arr)), L.ptr(ptr, C.c_uint64)))
    # span ids are injective in the span index (csrc/synth.h synth_span_id)
    return SpanSet(spec.services(), ptr, **arr, unique_ids=True, scan_order=1)


def _soa_out(arr: dict) -> L.SpanSoA:
    return L.SpanSoA(L.ptr(arr["trace_hash"], C.c_uint64), L.ptr(arr["span_id"], C.c_uint64),
                     L.ptr(arr["parent_span_id"], C.c_uint64), L.ptr(arr["svc"], C.c_uint16),
                     L.ptr(arr["flags"], C.c_uint16), L.ptr(arr["dur_us"], C.c_uint32))


def device_count() -> int:
    n = C.c_int()
    L.check(L.lib().anomod_device_count(C.byref(n)))
    return n.value


def device_count_safe() -> int:
    """Number of visible GPUs, 0 when the HIP runtime reports none."""
    n = C.c_int()
    return n.value if L.lib().anomod_device_count(C.byref(n)) == L.OK else 0


class DeviceSpans:
    """A span set resident in HBM (owned by libanomod)."""

    def __init__(self, ctx: "Context", handle: C.c_void_p, services: list[str]):
        self.ctx, self.handle, self.services = ctx, handle, list(services)
        ns, nt, g = C.c_uint64(), C.c_uint64(), C.c_int()
        L.check(L.lib().anomod_spans_info(handle, C.byref(ns), C.byref(nt)))
        L.check(L.lib().anomod_spans_grouped(handle, C.byref(g)))
        self.n_spans, self.n_traces = ns.value, nt.value
        self.grouped = bool(g.value)  # False: arrival order, traces known by trace_hash only

    @property
    def unique_ids(self) -> bool:
        u = C.c_int()
        L.check(L.lib().anomod_spans_unique_ids(self.handle, C.byref(u)))
        return bool(u.value)

    @property
    def scan_order(self) -> int:
        """1 collector order / 0 shuffled inside traces / -1 not probed yet."""
        o = C.c_int()
        L.check(L.lib().anomod_spans_scan_order(self.handle, C.byref(o)))
        return o.value

    @property
    def hist_compact(self) -> bool:
        """True once an aggregation overflowed the pair-form LDS histogram
        (later ones use the compact form)."""
        c = C.c_int()
        L.check(L.lib().anomod_spans_hist_compact(self.handle, C.byref(c)))
        return bool(c.value)

    @unique_ids.setter
    def unique_ids(self, v: bool):
        L.check(L.lib().anomod_spans_set_unique_ids(self.handle, 1 if v else 0))

    @property
    def hints(self) -> tuple[int, int]:
        """(scan_order, hist_form) the library holds for this set."""
        o, f = C.c_int(), C.c_int()
        L.check(L.lib().anomod_spans_hints(self.handle, C.byref(o), C.byref(f)))
        return o.value, f.value

    def set_hints(self, scan_order: int, hist_form: int):
        L.check(L.lib().anomod_spans_set_hints(self.handle, scan_order, hist_form))

    @property
    def has_start_us(self) -> bool:
        h = C.c_int()
        L.check(L.lib().anomod_spans_has_start_us(self.handle, C.byref(h)))
        return bool(h.value)

    def set_start_us(self, start_us):
        """Give the set its start-time column (u64 epoch microseconds, by span
        position)."""
        s = np.ascontiguousarray(start_us, np.uint64)
        if s.shape != (self.n_spans,):
            raise ValueError(f"start_us has shape {s.shape}, expected ({self.n_spans},)")
        L.check(L.lib().anomod_spans_set_start_us(self.ctx.handle, self.handle,
                                                  L.ptr(s, C.c_uint64)), self.ctx.handle)

    def start_us(self) -> np.ndarray:
        """The start-time column (AnomodError ESTATE when the set has none)."""
        out = np.empty(self.n_spans, np.uint64)
        L.check(L.lib().anomod_spans_get_start_us(self.ctx.handle, self.handle,
                                                  L.ptr(out, C.c_uint64)), self.ctx.handle)
        return out

    def fill_start_synthetic(self, t0_us: int, period_us: int, gap_us: int = 0):
        """Start times generated on the device: t0_us + (trace * period_us) //
        n_traces + position_in_trace * gap_us (grouped sets)."""
        L.check(L.lib().anomod_spans_fill_start_synthetic(self.ctx.handle, self.handle, t0_us,
                                                          period_us, gap_us), self.ctx.handle)

    def download(self) -> SpanSet:
        n = self.n_spans
        arr = dict(trace_hash=np.empty(n, np.uint64), span_id=np.empty(n, np.uint64),
                   parent_span_id=np.empty(n, np.uint64), svc=np.empty(n, np.uint16),
                   flags=np.empty(n, np.uint16), dur_us=np.empty(n, np.uint32))
        ptr = np.empty(self.n_traces + 1, np.uint64)
        L.check(L.lib().anomod_spans_download(self.ctx.handle, self.handle,
                                              C.byref(_soa_out(arr)), L.ptr(ptr, C.c_uint64)),
                self.ctx.handle)
        order, form = self.hints
        return SpanSet(self.services, ptr, **arr, unique_ids=self.unique_ids, scan_order=order,
                       hist_form=form, start_us=self.start_us() if self.has_start_us else None)

    def free(self):
        if self.handle:
            L.lib().anomod_spans_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One GPU: ``Context(device)``; use as a context manager or call close()."""

    def __init__(self, device: int = 0):
        self._lib = L.lib()
        h = C.c_void_p()
        L.check(self._lib.anomod_ctx_create(device, C.byref(h)))
        self.handle = h
        self.device = device

    # -- lifecycle
    def close(self):
        if self.handle:
            self._lib.anomod_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status: int):
        L.check(status, self.handle)

    def synchronize(self):
        self._check(self._lib.anomod_ctx_synchronize(self.handle))

    def stage_ms(self, stage: int) -> float:
        v = C.c_double()
        self._check(self._lib.anomod_ctx_stage_ms(self.handle, stage, C.byref(v)))
        return v.value

    def host_ms(self) -> dict:
        """Host wall milliseconds of the last occurrence of each one-off setup
        step / host-side call phase (anomod_ctx_host_ms) and how many times it
        happened: {name: (ms, count)}."""
        out = {}
        for slot, name in enumerate(L.HOST_SLOT_NAMES):
            v, c = C.c_double(), C.c_uint64()
            self._check(self._lib.anomod_ctx_host_ms(self.handle, slot, C.byref(v), C.byref(c)))
            out[name] = (v.value, c.value)
        return out

    def group_info(self) -> dict:
        """How the last grouping ran: path ("bucket" / "join": the bucket
        scatters then the ungrouped aggregation's per-bucket hash join /
        "lsd"),
        scatter levels or radix passes, and the key bits they sorted on."""
        p, lv, b = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.anomod_ctx_group_info(self.handle, C.byref(p), C.byref(lv),
                                                    C.byref(b)))
        return {"path": {1: "bucket", 2: "join"}.get(p.value, "lsd"), "levels": lv.value,
                "bits": b.value}

    # -- multi-GPU
    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * L.UNIQUE_ID_BYTES)()
        L.check(L.lib().anomod_comm_unique_id(buf))
        return bytes(buf)

    def attach_comm(self, unique_id: bytes, nranks: int, rank: int):
        buf = (C.c_uint8 * L.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.anomod_ctx_attach_comm(self.handle, buf, nranks, rank))

    def comm_info(self) -> tuple[int, int]:
        """(nranks, rank) of the attached transport ((1, 0) without one)."""
        n, r = C.c_int(), C.c_int()
        self._check(self._lib.anomod_ctx_comm_info(self.handle, C.byref(n), C.byref(r)))
        return n.value, r.value

    def sort_u64(self, keys, begin_bit: int = 0, end_bit: int = 64) -> tuple[np.ndarray, int]:
        """Stable device radix sort of u64 keys by bits [begin_bit, end_bit)
        (csrc/radix.hip) -> (sorted keys, digit passes run)."""
        k = np.ascontiguousarray(keys, np.uint64)
        out = np.empty_like(k)
        passes = C.c_int()
        self._check(self._lib.anomod_sort_u64(self.handle, L.ptr(k, C.c_uint64), k.size,
                                              begin_bit, end_bit, L.ptr(out, C.c_uint64),
                                              C.byref(passes)))
        return out, passes.value

    def attach_host_comm(self, nranks: int, rank: int, allreduce, allgather):
        """Host collective transport instead of RCCL: ``allreduce(buf, dtype,
        op)`` reduces a numpy array in place over all ranks, ``allgather(buf,
        block)`` fills every rank's ``block``-byte slice of a u8 array (this
        rank's is set); libanomod stages every collective through pinned host
        memory and calls them in the RCCL path's order."""
        dtypes = {L.DTYPE_I32: np.int32, L.DTYPE_U32: np.uint32, L.DTYPE_U64: np.uint64,
                  L.DTYPE_F64: np.float64}

        def _ar(_user, buf, count, dtype, op):
            try:
                dt = np.dtype(dtypes[dtype])
                raw = (C.c_uint8 * (count * dt.itemsize)).from_address(buf)
                allreduce(np.frombuffer(raw, dtype=dt), dtype, op)
                return 0
            except Exception:  # noqa: BLE001 - reported to libanomod as a failed transport
                return 1

        def _ag(_user, buf, block):
            try:
                raw = (C.c_uint8 * (block * nranks)).from_address(buf)
                allgather(np.frombuffer(raw, dtype=np.uint8), block)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        # the ctypes thunks must outlive every call libanomod makes through them
        self._host_comm = (L.HostAllreduceFn(_ar), L.HostAllgatherFn(_ag))
        self._check(self._lib.anomod_ctx_attach_host_comm(
            self.handle, nranks, rank, C.cast(self._host_comm[0], C.c_void_p),
            C.cast(self._host_comm[1], C.c_void_p), None))

    # -- spans
    def upload(self, spans: SpanSet) -> DeviceSpans:
        h = C.c_void_p()
        soa = spans.soa()
        self._check(self._lib.anomod_spans_upload(self.handle, C.byref(soa), spans.n_spans,
                                                  L.ptr(spans.trace_ptr, C.c_uint64),
                                                  spans.n_traces, C.byref(h)))
        d = DeviceSpans(self, h, spans.services)
        d.unique_ids = spans.unique_ids
        d.set_hints(spans.scan_order, spans.hist_form)
        if spans.start_us is not None:
            d.set_start_us(spans.start_us)
        return d

    def upload_ungrouped(self, spans: SpanSet) -> DeviceSpans:
        """Upload spans in arrival order: the trace of a span is its trace_hash
        alone (spans.trace_ptr is ignored)."""
        h = C.c_void_p()
        soa = spans.soa()
        self._check(self._lib.anomod_spans_upload_ungrouped(self.handle, C.byref(soa),
                                                            spans.n_spans, C.byref(h)))
        d = DeviceSpans(self, h, spans.services)
        d.unique_ids = spans.unique_ids
        d.set_hints(spans.scan_order, spans.hist_form)
        self._reserve_for(d)
        return d

    def _reserve_for(self, d: DeviceSpans):
        """Best effort: the workspace for an ungrouped set's first aggregation
        now (a set that fits HBM while its workspace does not still uploads;
        its aggregation then reports the shortage)."""
        try:
            self.reserve_grouping(d.n_spans)
        except L.AnomodError as e:
            if "ENOMEM" not in str(e):
                raise

    def reserve_grouping(self, n_spans: int, both_records: bool = False):
        """Size the context's grouping workspace for an ungrouped set of
        n_spans ahead of its first aggregation (anomod_ctx_reserve_grouping:
        the ~58 B/span of the join path, + 32 B/span with both_records)."""
        self._check(self._lib.anomod_ctx_reserve_grouping(self.handle, n_spans,
                                                          1 if both_records else 0))

    def group(self, spans: DeviceSpans) -> DeviceSpans:
        """Group an ungrouped device span set by trace (segmented radix sort
        on the GPU): traces by mix64(trace_hash), spans in arrival order."""
        h = C.c_void_p()
        self._check(self._lib.anomod_spans_group(self.handle, spans.handle, C.byref(h)))
        return DeviceSpans(self, h, spans.services)

    def shuffle(self, spans: DeviceSpans, seed: int, window_traces: int = 0) -> DeviceSpans:
        """Synthetic arrival order of a grouped set: window_traces = 0 shuffles
        spans inside each trace (stays grouped); W > 0 interleaves the spans
        of every W consecutive traces (ungrouped result)."""
        h = C.c_void_p()
        self._check(self._lib.anomod_spans_shuffle(self.handle, spans.handle, seed, window_traces,
                                                   C.byref(h)))
        d = DeviceSpans(self, h, spans.services)
        if window_traces:  # an ungrouped set: its grouping workspace now, not at the first call
            self._reserve_for(d)
        return d

    def generate(self, spec: SynthSpec, n_traces: int, shard: int = 0) -> DeviceSpans:
        h = C.c_void_p()
        cs = spec.c_struct()
        self._check(self._lib.anomod_spans_generate(self.handle, C.byref(cs), shard, n_traces,
                                                    C.byref(h)))
        return DeviceSpans(self, h, spec.services())

    def edge_aggregate(self, spans: DeviceSpans | SpanSet, with_hist: bool = True) -> EdgeTable:
        """Edge table of a span set.  A host set goes through
        anomod_edge_aggregate_host (pinned staging pipeline into a device set
        the context keeps; the hints learned on the device go back onto the
        host set)."""
        if isinstance(spans, SpanSet):
            table = EdgeTable.empty(spans.services, with_hist)
            cs = table.c_struct()
            soa = spans.soa()
            order, form = C.c_int(spans.scan_order), C.c_int(spans.hist_form)
            self._check(self._lib.anomod_edge_aggregate_host(
                self.handle, C.byref(soa), spans.n_spans, L.ptr(spans.trace_ptr, C.c_uint64),
                spans.n_traces, len(spans.services), 1 if spans.unique_ids else 0,
                C.byref(order), C.byref(form), C.byref(cs)))
            if table.hist is not None:
                table.hist = table.hist.reshape(edge_rows(len(spans.services)), L.HIST_BINS)
            spans.scan_order, spans.hist_form = order.value, form.value
            return table
        # a device set: its hints live on the set itself (libanomod keeps them)
        table = EdgeTable.empty(spans.services, with_hist)
        cs = table.c_struct()
        fn = (self._lib.anomod_edge_aggregate_spans if spans.grouped
              else self._lib.anomod_edge_aggregate_ungrouped)
        self._check(fn(self.handle, spans.handle, len(spans.services), C.byref(cs)))
        if table.hist is not None:
            table.hist = table.hist.reshape(edge_rows(len(spans.services)), L.HIST_BINS)
        return table

    def edge_windows(self, spans: DeviceSpans | SpanSet, t0_us: int, step_us: int,
                     n_windows: int, outputs=("count", "errors", "sum_us", "max_us")
                     ) -> EdgeWindows:
        """Per-window edge table of a grouped set with start times
        (anomod_edge_windows_spans): window w = (start_us - t0_us) // step_us;
        spans outside [0, n_windows) are counted in .outside.  Rank-local.
        `outputs` names the tables to compute (the others stay zero)."""
        tmp = None
        if isinstance(spans, SpanSet):
            if spans.start_us is None:
                raise ValueError("span set has no start_us column")
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            if not 1 <= int(n_windows) <= 65536 or int(n_windows) * edge_rows(S) > 1 << 24:
                raise L.AnomodError(L.EINVAL, f"n_windows={n_windows} outside [1, 65536] or "
                                    f"n_windows * edge rows > 2^24 (n_services={S})")
            win = EdgeWindows.empty(spans.services, t0_us, step_us, n_windows)
            cs = L.EdgeWindowsC(
                S, n_windows, t0_us, step_us,
                L.ptr(win.count if "count" in outputs else None, C.c_uint64),
                L.ptr(win.errors if "errors" in outputs else None, C.c_uint64),
                L.ptr(win.sum_us if "sum_us" in outputs else None, C.c_uint64),
                L.ptr(win.max_us if "max_us" in outputs else None, C.c_uint32), 0)
            self._check(self._lib.anomod_edge_windows_spans(self.handle, spans.handle,
                                                            C.byref(cs)))
            win.outside = int(cs.outside)
            return win
        finally:
            if tmp is not None:
                tmp.free()

    def edge_load(self, spans: DeviceSpans | SpanSet, t0_us: int, step_us: int,
                  n_windows: int, outputs=("busy_us", "carried")) -> EdgeLoad:
        """Per-window edge load of a grouped set with start times
        (anomod_edge_load_spans): the windows and rows of edge_windows;
        .busy_us[w, row] the time the edge's calls were open inside window w,
        .carried[w, row] the calls still open when it opens; spans that touch
        no window are counted in .outside.  A call that starts before t0_us
        and reaches into the range is clipped, not dropped.  Rank-local.
        `outputs` names the tables to compute (the others stay zero).  A
        resident set that has been aggregated is read as one stream (its
        parent rows); a host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            if spans.start_us is None:
                raise ValueError("span set has no start_us column")
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            if not 1 <= int(n_windows) <= 65536 or int(n_windows) * edge_rows(S) > 1 << 24:
                raise L.AnomodError(L.EINVAL, f"n_windows={n_windows} outside [1, 65536] or "
                                    f"n_windows * edge rows > 2^24 (n_services={S})")
            load = EdgeLoad.empty(spans.services, t0_us, step_us, n_windows)
            cs = L.EdgeLoadC(
                S, n_windows, t0_us, step_us,
                L.ptr(load.busy_us if "busy_us" in outputs else None, C.c_uint64),
                L.ptr(load.carried if "carried" in outputs else None, C.c_uint64), 0)
            self._check(self._lib.anomod_edge_load_spans(self.handle, spans.handle, C.byref(cs)))
            load.outside = int(cs.outside)
            return load
        finally:
            if tmp is not None:
                tmp.free()

    def edge_exemplars(self, spans: DeviceSpans | SpanSet, k: int = 8,
                       errors_only: bool = False) -> EdgeExemplars:
        """The k slowest calls of every edge row of a grouped set
        (anomod_edge_exemplars_spans), or with errors_only the k slowest
        error-flagged ones: ordered by dur_us descending, then span position
        ascending.  EdgeExemplars.trace_ids / .select carry a row's exemplars
        back to their traces.  k in [1, 64].  Rank-local.  A resident set
        that has been aggregated is read as one stream (its parent rows); a
        host set is uploaded for the call.  A start column is not needed."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            if not 1 <= int(k) <= 64 or int(k) * edge_rows(S) > 1 << 24:
                raise L.AnomodError(L.EINVAL, f"k={k} outside [1, 64] or k * edge rows > 2^24 "
                                    f"(n_services={S})")
            ex = EdgeExemplars.empty(spans.services, k, 1 if errors_only else 0)
            cs = ex.c_struct()
            self._check(self._lib.anomod_edge_exemplars_spans(self.handle, spans.handle,
                                                              C.byref(cs)))
            return ex
        finally:
            if tmp is not None:
                tmp.free()

    def edge_window_quantiles(self, spans: DeviceSpans | SpanSet, t0_us: int, step_us: int,
                              n_windows: int, q_pct=(50, 99), with_table: bool = True
                              ) -> EdgeWindows:
        """Exact per-window edge latency quantiles of a grouped set with start
        times (anomod_edge_window_quantiles_spans): the windows and rows of
        edge_windows; .q_us[w, row, k] = sorted(x)[int(c * q_pct[k] / 100)]
        over the cell's c latencies (0 for an empty cell), .q_count the cell
        counts.  with_table also fills count / errors / sum_us / max_us by
        edge_windows (else they stay zero).  q_pct: 1..8 percentages in
        [0, 99].  Rank-local.  A host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            if spans.start_us is None:
                raise ValueError("span set has no start_us column")
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            if not 1 <= int(n_windows) <= 65536 or int(n_windows) * edge_rows(S) > 1 << 24:
                raise L.AnomodError(L.EINVAL, f"n_windows={n_windows} outside [1, 65536] or "
                                    f"n_windows * edge rows > 2^24 (n_services={S})")
            qs = [int(q) for q in q_pct]
            if not 1 <= len(qs) <= 8 or any(not 0 <= q <= 99 for q in qs):
                raise L.AnomodError(L.EINVAL, f"q_pct={tuple(q_pct)}: 1..8 percentages in [0, 99]")
            if with_table:
                win = self.edge_windows(spans, t0_us, step_us, n_windows)
            else:
                win = EdgeWindows.empty(spans.services, t0_us, step_us, n_windows)
            q = np.asarray(qs, np.uint32)
            E = edge_rows(S)
            win.q_pct = tuple(qs)
            win.q_us = np.zeros((n_windows, E, len(qs)), np.uint32)
            win.q_count = np.zeros((n_windows, E), np.uint64)
            cs = L.EdgeWindowQuantilesC(S, n_windows, t0_us, step_us, len(qs),
                                        L.ptr(q, C.c_uint32), L.ptr(win.q_count, C.c_uint64),
                                        L.ptr(win.q_us, C.c_uint32), 0)
            self._check(self._lib.anomod_edge_window_quantiles_spans(self.handle, spans.handle,
                                                                     C.byref(cs)))
            win.outside = int(cs.outside)
            return win
        finally:
            if tmp is not None:
                tmp.free()

    def self_time(self, spans: DeviceSpans | SpanSet, with_hist: bool = True,
                  per_span: bool = False):
        """Self-time (exclusive latency) edge table of a grouped set
        (anomod_edge_self_time_spans): the rows, counts and errors of
        edge_aggregate, the latency fields over self_us = dur_us - min(dur_us,
        sum of the direct children's dur_us).  per_span=True also returns the
        u32 self_us column by span position (rank-local).  A host set is
        uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            table = EdgeTable.empty(spans.services, with_hist)
            cs = table.c_struct()
            self_us = np.zeros(spans.n_spans, np.uint32) if per_span else None
            self._check(self._lib.anomod_edge_self_time_spans(
                self.handle, spans.handle, S, C.byref(cs), L.ptr(self_us, C.c_uint32)))
            if table.hist is not None:
                table.hist = table.hist.reshape(edge_rows(S), L.HIST_BINS)
            return (table, self_us) if per_span else table
        finally:
            if tmp is not None:
                tmp.free()

    def critical_path(self, spans: DeviceSpans | SpanSet, with_hist: bool = True,
                      per_span: bool = False) -> CriticalPath:
        """Critical path of a grouped set with start times
        (anomod_edge_critical_path_spans): which spans determined their
        trace's end-to-end latency (walking back from each parent's end
        through its last-finishing, non-overlapping children) and the
        exclusive time each added; the edge table counts the on-path spans
        and takes its latency fields over their cp_us.  per_span=True also
        returns the u32 cp_us and u8 on_path columns by span position
        (rank-local).  A host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            if spans.start_us is None:
                raise ValueError("span set has no start_us column")
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            table = EdgeTable.empty(spans.services, with_hist)
            cs = table.c_struct()
            cp_us = np.zeros(spans.n_spans, np.uint32) if per_span else None
            on_path = np.zeros(spans.n_spans, np.uint8) if per_span else None
            self._check(self._lib.anomod_edge_critical_path_spans(
                self.handle, spans.handle, S, C.byref(cs), L.ptr(cp_us, C.c_uint32),
                L.ptr(on_path, C.c_uint8)))
            if table.hist is not None:
                table.hist = table.hist.reshape(edge_rows(S), L.HIST_BINS)
            return CriticalPath(table, cp_us, on_path)
        finally:
            if tmp is not None:
                tmp.free()

    def trace_spectrum(self, spans: DeviceSpans | SpanSet, thr_us=None, use_errors: bool = True,
                       per_trace: bool = True) -> TraceSpectrum:
        """Abnormal / normal trace labels and the per-class trace coverage of
        services and edge rows (anomod_trace_spectrum_spans).  thr_us: u32 [E]
        latency thresholds by edge row (spectrum_thresholds; None: none, only
        error flags label traces).  per_trace=False skips the per-trace class
        column.  Rank-local.  A host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            E = edge_rows(S)
            thr = None
            if thr_us is not None:
                thr = np.ascontiguousarray(thr_us, np.uint32)
                if thr.shape != (E,):
                    raise ValueError(f"thr_us has shape {thr.shape}, expected ({E},)")
            sp = TraceSpectrum(list(spans.services), np.zeros(2, np.uint64),
                               np.zeros((2, S), np.uint64), np.zeros((2, E), np.uint64),
                               np.zeros(E, np.uint64),
                               np.zeros(spans.n_traces, np.uint8) if per_trace else None, thr,
                               bool(use_errors))
            cs = L.TraceSpectrumC(S, 1 if use_errors else 0, L.ptr(thr, C.c_uint32), (0, 0),
                                  L.ptr(sp.svc_traces, C.c_uint64),
                                  L.ptr(sp.edge_traces, C.c_uint64),
                                  L.ptr(sp.bad_spans, C.c_uint64),
                                  L.ptr(sp.trace_abnormal, C.c_uint8))
            self._check(self._lib.anomod_trace_spectrum_spans(self.handle, spans.handle,
                                                              C.byref(cs)))
            sp.n_traces[:] = (cs.n_traces[0], cs.n_traces[1])
            return sp
        finally:
            if tmp is not None:
                tmp.free()

    def trace_shapes(self, spans: DeviceSpans | SpanSet, trace_class=None,
                     use_errors: bool = False, cap: int | None = None, per_trace: bool = False,
                     per_span: bool = False, svc_key="names") -> TraceShapes:
        """Shape census of a grouped set (anomod_trace_shapes_spans): the
        distinct trace shapes — fingerprints of the multiset of labelled
        root-to-span call paths — with their counts, by count descending.
        trace_class: u8 [n_traces] (e.g. TraceSpectrum.trace_abnormal) splits
        the counts into .abnormal.  use_errors makes the error flag part of a
        span's label.  cap: the most shapes to return (None: all — a second
        call follows when the set has more than 65,536).  svc_key: "names" keys the services by the hash of
        their names (decode.hash64), so shapes compare across runs with
        different service lists; None keys them by index.
        per_trace / per_span also return trace_shape / path_hash.  Rank-local.
        A host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            nt, n = int(spans.n_traces), int(spans.n_spans)
            keys = None
            if svc_key is not None:
                if svc_key != "names":
                    raise ValueError(f"svc_key={svc_key!r}: 'names' or None")
                from .decode import hash64
                keys = np.array([hash64(s) for s in spans.services], np.uint64)
            cls = None
            if trace_class is not None:
                cls = np.ascontiguousarray(trace_class, np.uint8)
                if cls.shape != (nt,):
                    raise ValueError(f"trace_class has shape {cls.shape}, expected ({nt},)")
            tshape = np.zeros(nt, np.uint64) if per_trace else None
            phash = np.zeros(n, np.uint64) if per_span else None

            def call(m, with_cols):
                arrs = [np.zeros(m, np.uint64) for _ in range(4)]
                cs = L.TraceShapesC(S, 1 if use_errors else 0, L.ptr(keys, C.c_uint64),
                                    L.ptr(cls, C.c_uint8), m, 0, 0,
                                    *(L.ptr(a if m else None, C.c_uint64) for a in arrs),
                                    L.ptr(tshape if with_cols else None, C.c_uint64),
                                    L.ptr(phash if with_cols else None, C.c_uint64))
                self._check(self._lib.anomod_trace_shapes_spans(self.handle, spans.handle,
                                                                C.byref(cs)))
                return cs, arrs

            if cap is not None and int(cap) < 0:
                raise ValueError(f"cap={cap}: a count of shapes")
            m = min(nt, 1 << 16) if cap is None else int(cap)
            cs, arrs = call(m, True)
            if cap is None and int(cs.n_shapes) > m:
                m = int(cs.n_shapes)
                cs, arrs = call(m, True)
            k = min(m, int(cs.n_shapes))
            return TraceShapes(list(spans.services), *(a[:k] for a in arrs), int(cs.n_shapes),
                               int(cs.off_tree_spans), tshape, phash, bool(use_errors))
        finally:
            if tmp is not None:
                tmp.free()

    def error_origins(self, spans: DeviceSpans | SpanSet, per_span: bool = False) -> ErrorOrigins:
        """Error origins of a grouped set (anomod_error_origins_spans): per
        edge row the error-flagged spans whose failure started there (origin)
        or passed through (propagated), where failures were stopped, how many
        reached their trace's entry (surfaced), the spans that absorbed a
        callee's failure and the hops the failures travelled.  per_span=True
        also returns span_state (class | fate << 2) and span_hops by span
        position.  Rank-local.  A host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            eo = ErrorOrigins.empty(spans.services, int(spans.n_spans) if per_span else None)
            cs = L.ErrorOriginsC(len(spans.services), 0, 0,
                                 *(L.ptr(getattr(eo, k), C.c_uint64) for k in eo.TABLES[:6]),
                                 L.ptr(eo.hops_max, C.c_uint32), L.ptr(eo.span_state, C.c_uint8),
                                 L.ptr(eo.span_hops, C.c_uint32))
            self._check(self._lib.anomod_error_origins_spans(self.handle, spans.handle,
                                                             C.byref(cs)))
            eo.error_spans, eo.loop_spans = int(cs.error_spans), int(cs.loop_spans)
            return eo
        finally:
            if tmp is not None:
                tmp.free()

    def call_repeats(self, spans: DeviceSpans | SpanSet, per_span: bool = False) -> CallRepeats:
        """Call repeats of a grouped set (anomod_call_repeats_spans): per edge
        row the groups — one parent span's calls to one callee service — the
        calls beyond the first of a group, the groups that repeated, those
        that repeated around a failure (retried = recovered + exhausted), the
        group-size histogram and maximum, and, for a set with start times, the
        members that started after a failure of their group had ended.
        per_span=True also returns span_group_size and span_after_error by
        span position.  Rank-local.  A host set is uploaded for the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            cr = CallRepeats.empty(spans.services, int(spans.n_spans) if per_span else None)
            cs = L.CallRepeatsC(len(spans.services), 0, 0, 0,
                                *(L.ptr(getattr(cr, k), C.c_uint64) for k in cr.TABLES[:8]),
                                L.ptr(cr.size_max, C.c_uint32),
                                L.ptr(cr.span_group_size, C.c_uint32),
                                L.ptr(cr.span_after_error, C.c_uint8))
            self._check(self._lib.anomod_call_repeats_spans(self.handle, spans.handle,
                                                            C.byref(cs)))
            cr.grouped_spans, cr.max_size = int(cs.grouped_spans), int(cs.max_size)
            cr.timed = bool(cs.timed)
            return cr
        finally:
            if tmp is not None:
                tmp.free()

    def call_transit(self, spans: DeviceSpans | SpanSet, with_hist: bool = True,
                     per_span: bool = False) -> CallTransit:
        """Call transit of a grouped set with start times
        (anomod_call_transit_spans): for every call whose parent span made no
        other call, the request gap (parent's start to the call's start) and
        the response gap (the call's end to the parent's end) as two edge
        tables, and per edge row the calls that start before their parent
        (early: clock skew), end after it (late: abandoned by the caller) or
        have no start time (untimed).  per_span=True also returns
        span_req_us, span_resp_us and span_state (TRANSIT_* bits) by span
        position.  With a communicator attached the two tables are merged over
        the ranks; everything else is rank-local.  A host set is uploaded for
        the call."""
        tmp = None
        if isinstance(spans, SpanSet):
            if spans.start_us is None:
                raise ValueError("span set has no start_us column")
            tmp = spans = self.upload(spans)
        try:
            S = len(spans.services)
            tr = CallTransit.empty(spans.services, with_hist,
                                   int(spans.n_spans) if per_span else None)
            req, resp = tr.request.c_struct(), tr.response.c_struct()
            cs = L.CallTransitC(S, 0, 0, C.pointer(req), C.pointer(resp),
                                *(L.ptr(getattr(tr, k), C.c_uint64) for k in tr.TABLES),
                                L.ptr(tr.span_req_us, C.c_uint32),
                                L.ptr(tr.span_resp_us, C.c_uint32),
                                L.ptr(tr.span_state, C.c_uint8))
            self._check(self._lib.anomod_call_transit_spans(self.handle, spans.handle,
                                                            C.byref(cs)))
            tr.calls, tr.paired = int(cs.calls), int(cs.paired)
            for t in (tr.request, tr.response):
                if t.hist is not None:
                    t.hist = t.hist.reshape(edge_rows(S), L.HIST_BINS)
            return tr
        finally:
            if tmp is not None:
                tmp.free()

    def edge_quantiles_exact(self, spans: DeviceSpans | SpanSet, q_pct=(50, 99)):
        """Exact per-edge order statistics x[(c*q)//100] of the sorted edge
        latencies ([E, len(q_pct)], NaN for empty edges) and the per-edge
        counts: the cross-check of the histogram quantiles (§8a a11)."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            q = np.ascontiguousarray(q_pct, np.uint32)
            S = len(spans.services)
            E = edge_rows(S)
            out = np.empty((E, q.shape[0]), np.float64)
            cnt = np.empty(E, np.uint64)
            self._check(self._lib.anomod_edge_quantiles_exact(
                self.handle, spans.handle, S, L.ptr(q, C.c_uint32), q.shape[0],
                L.ptr(out, C.c_double), L.ptr(cnt, C.c_uint64)))
            return out, cnt
        finally:
            if tmp is not None:
                tmp.free()

    def trace_structure(self, spans: DeviceSpans | SpanSet,
                        download: bool = True) -> TraceStructure | None:
        """Per-span parent/depth/children and per-trace roots/services
        (the trace-structure HIP kernel).  download=False runs the kernel
        without copying the outputs back (timing)."""
        tmp = None
        if isinstance(spans, SpanSet):
            tmp = spans = self.upload(spans)
        try:
            if not download:
                cs = L.TraceStructC(len(spans.services))
                self._check(self._lib.anomod_trace_structure_spans(self.handle, spans.handle,
                                                                   C.byref(cs)))
                return None
            ts = TraceStructure.empty(spans.services, spans.n_spans, spans.n_traces)
            cs = ts.c_struct()
            self._check(self._lib.anomod_trace_structure_spans(self.handle, spans.handle,
                                                               C.byref(cs)))
            return ts
        finally:
            if tmp is not None:
                tmp.free()

    def segment_summary(self, seg) -> dict:
        """analyze_trace_patterns over a SegmentSet (segment-summary kernel)."""
        from .segments import segment_summary
        return segment_summary(self, seg)

    # -- metric series
    def ewma_z(self, X: np.ndarray, alpha: float, W: int, eps: float = 1e-12) -> np.ndarray:
        X = np.ascontiguousarray(X, dtype=np.float32)
        T, S = X.shape
        if T % W:
            raise ValueError(f"T={T} must be a multiple of W={W}")
        Z = np.empty((T // W, S), np.float32)
        if T == 0 or S == 0:
            return Z
        self._check(self._lib.anomod_ewma_z(self.handle, L.ptr(X, C.c_float), T, S, alpha, W,
                                            eps, L.ptr(Z, C.c_float)))
        return Z

    def correlate(self, X: np.ndarray, Y: np.ndarray, min_pairs: int = 3
                  ) -> tuple[np.ndarray, np.ndarray]:
        """Pearson correlation of every column of X [T, S] against the target
        columns Y [T, K] (a 1-D Y is one target; K <= 8), pairwise-complete
        over non-finite samples (anomod_correlate; the contract is in
        include/anomod.h).  Returns (r f64 [K, S], n u32 [K, S]): r is NaN
        where fewer than max(min_pairs, 2) pairs exist or a side is constant."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        Y = _targets(Y, X.shape[0])
        T, S = X.shape
        K = Y.shape[1]
        r = np.full((K, S), np.nan, np.float64)
        n = np.zeros((K, S), np.uint32)
        self._check(self._lib.anomod_correlate(self.handle, L.ptr(X, C.c_float), T, S,
                                               L.ptr(Y, C.c_float), K, int(min_pairs),
                                               L.ptr(r, C.c_double), L.ptr(n, C.c_uint32)))
        return r, n

    # -- ranking
    def pagerank(self, row_ptr, col, w, p, alpha=0.85, iters=100, tol=1e-10):
        row_ptr = np.ascontiguousarray(row_ptr, np.uint32)
        col = np.ascontiguousarray(col, np.uint32)
        w = np.ascontiguousarray(w, np.float32)
        p = np.ascontiguousarray(p, np.float64)
        N = row_ptr.shape[0] - 1
        x = np.empty(N, np.float64)
        done = C.c_uint32()
        if col.size == 0:  # keep the pointers valid for an edgeless graph
            col, w = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        self._check(self._lib.anomod_pagerank(self.handle, L.ptr(row_ptr, C.c_uint32),
                                              L.ptr(col, C.c_uint32), L.ptr(w, C.c_float), N,
                                              L.ptr(p, C.c_double), alpha, iters, tol,
                                              L.ptr(x, C.c_double), C.byref(done)))
        return x, done.value


def _targets(Y, T: int) -> np.ndarray:
    """Correlation targets as a C-contiguous f32 [T, K] (a 1-D Y is K = 1)."""
    Y = np.asarray(Y, dtype=np.float32)
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.ndim != 2 or Y.shape[0] != T:
        raise ValueError(f"correlate: Y of shape {Y.shape} does not hold T={T} rows")
    return np.ascontiguousarray(Y)


def synth_graph_csr(N: int, mean_degree: int = 10, seed: int = 11):
    """Host CSR (row_ptr u32, col u32, w f32) of the synthetic config-5 graph
    DeviceGraph(synthetic=(N, mean_degree, seed)) solves."""
    lib = L.lib()
    nnz = C.c_uint64()
    nul32 = C.cast(None, C.POINTER(C.c_uint32))
    L.check(lib.anomod_graph_synthetic_csr(N, mean_degree, seed, nul32, nul32,
                                           C.cast(None, C.POINTER(C.c_float)), 0, C.byref(nnz)))
    row_ptr = np.empty(N + 1, np.uint32)
    col = np.empty(max(1, nnz.value), np.uint32)
    w = np.empty(max(1, nnz.value), np.float32)
    L.check(lib.anomod_graph_synthetic_csr(N, mean_degree, seed, L.ptr(row_ptr, C.c_uint32),
                                           L.ptr(col, C.c_uint32), L.ptr(w, C.c_float),
                                           col.shape[0], C.byref(nnz)))
    return row_ptr, col[:nnz.value], w[:nnz.value]


class DeviceGraph:
    """A CSR graph resident in HBM for repeated PageRank solves."""

    def __init__(self, ctx: Context, row_ptr=None, col=None, w=None, *, synthetic=None):
        self.ctx = ctx
        h = C.c_void_p()
        lib = L.lib()
        if synthetic is not None:
            N, deg, seed = synthetic
            ctx._check(lib.anomod_graph_synthetic(ctx.handle, N, deg, seed, C.byref(h)))
        else:
            row_ptr = np.ascontiguousarray(row_ptr, np.uint32)
            col = np.ascontiguousarray(col, np.uint32)
            w = np.ascontiguousarray(w, np.float32)
            if col.size == 0:  # keep the pointers valid for an edgeless graph
                col, w = np.zeros(1, np.uint32), np.zeros(1, np.float32)
            ctx._check(lib.anomod_graph_create(ctx.handle, L.ptr(row_ptr, C.c_uint32),
                                               L.ptr(col, C.c_uint32), L.ptr(w, C.c_float),
                                               row_ptr.shape[0] - 1, C.byref(h)))
        self.handle = h
        n, nnz = C.c_uint32(), C.c_uint64()
        L.check(lib.anomod_graph_info(h, C.byref(n), C.byref(nnz)))
        self.N, self.nnz = n.value, nnz.value

    def pagerank(self, p, alpha=0.85, iters=100, tol=0.0):
        p = np.ascontiguousarray(p, np.float64)
        x = np.empty(self.N, np.float64)
        done = C.c_uint32()
        self.ctx._check(L.lib().anomod_graph_pagerank(self.ctx.handle, self.handle,
                                                      L.ptr(p, C.c_double), alpha, iters, tol,
                                                      L.ptr(x, C.c_double), C.byref(done)))
        return x, done.value

    PATHS = {1: "graph", 2: "readback", 3: "persistent"}

    def last_solve(self) -> tuple[str, int]:
        """(path of the last pagerank() / pagerank_batch() solve, persistent-
        launch fallbacks so far); the path is "graph" / "readback" /
        "persistent" (a per-launch batch reports "graph" for fixed iterations,
        "readback" in tolerance mode), with a
        "fallback:" prefix when a persistent launch timed out at its grid
        barrier and the solve was rerun per launch."""
        path, fb = C.c_uint32(), C.c_uint32()
        L.check(L.lib().anomod_graph_last_solve(self.handle, C.byref(path), C.byref(fb)))
        name = self.PATHS.get(path.value & 3, "none")
        return ("fallback:" + name if path.value & 4 else name), fb.value

    def pagerank_sharded(self, p, alpha=0.85, iters=100, tol=0.0, virtual_shards=0):
        """Row-sharded solve: over the ranks of the attached RCCL communicator,
        or over ``virtual_shards`` row shards on this device when none is
        attached.  Returns the whole vector on every rank."""
        p = np.ascontiguousarray(p, np.float64)
        x = np.empty(self.N, np.float64)
        done = C.c_uint32()
        self.ctx._check(L.lib().anomod_graph_pagerank_sharded(
            self.ctx.handle, self.handle, L.ptr(p, C.c_double), alpha, iters, tol,
            virtual_shards, L.ptr(x, C.c_double), C.byref(done)))
        return x, done.value

    def pagerank_batch(self, P, alpha=0.85, iters=100, tol=0.0):
        """K personalizations ([K, N]) in one batched solve -> x [K, N]."""
        P = np.ascontiguousarray(np.atleast_2d(P), np.float64)
        K = P.shape[0]
        X = np.empty((K, self.N), np.float64)
        done = C.c_uint32()
        self.ctx._check(L.lib().anomod_graph_pagerank_batch(
            self.ctx.handle, self.handle, L.ptr(P, C.c_double), K, alpha, iters, tol,
            L.ptr(X, C.c_double), C.byref(done)))
        return X, done.value

    def free(self):
        if self.handle:
            L.lib().anomod_graph_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceSeries:
    """A [T][S] metric matrix resident in HBM with carried EWMA state."""

    def __init__(self, ctx: Context, T: int, S: int):
        self.ctx, self.T, self.S = ctx, T, S
        h = C.c_void_p()
        ctx._check(L.lib().anomod_series_create(ctx.handle, T, S, C.byref(h)))
        self.handle = h

    def upload(self, X: np.ndarray):
        X = np.ascontiguousarray(X, np.float32)
        assert X.shape == (self.T, self.S)
        self.ctx._check(L.lib().anomod_series_upload(self.ctx.handle, self.handle,
                                                     L.ptr(X, C.c_float)))

    def fill_synthetic(self, seed: int, t0: int = 0):
        self.ctx._check(L.lib().anomod_series_fill_synthetic(self.ctx.handle, self.handle,
                                                             seed, t0))

    def reset_state(self):
        self.ctx._check(L.lib().anomod_series_reset_state(self.ctx.handle, self.handle))

    def download(self) -> np.ndarray:
        """The resident matrix as host rows X[T][S]."""
        X = np.empty((self.T, self.S), np.float32)
        self.ctx._check(L.lib().anomod_series_download(self.ctx.handle, self.handle,
                                                       L.ptr(X, C.c_float)))
        return X

    def ewma_z(self, alpha: float, W: int, eps: float = 1e-12, download: bool = True):
        Z = np.empty((self.T // W, self.S), np.float32) if download else None
        self.ctx._check(L.lib().anomod_series_ewma_z(
            self.ctx.handle, self.handle, alpha, W, eps,
            L.ptr(Z, C.c_float) if Z is not None else C.cast(None, C.POINTER(C.c_float))))
        return Z

    def correlate(self, Y: np.ndarray, min_pairs: int = 3) -> tuple[np.ndarray, np.ndarray]:
        """Context.correlate of the resident matrix (anomod_series_correlate):
        reads it in the layout it has and leaves it and the EWMA state alone."""
        Y = _targets(Y, self.T)
        K = Y.shape[1]
        r = np.full((K, self.S), np.nan, np.float64)
        n = np.zeros((K, self.S), np.uint32)
        self.ctx._check(L.lib().anomod_series_correlate(
            self.ctx.handle, self.handle, L.ptr(Y, C.c_float), K, int(min_pairs),
            L.ptr(r, C.c_double), L.ptr(n, C.c_uint32)))
        return r, n

    def free(self):
        if self.handle:
            L.lib().anomod_series_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

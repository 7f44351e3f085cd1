"""Reference for the edge load table (a plain helper, not a conftest).

Edge rows come from the C oracle (oracle.native.span_edges: the first-match
parent rule of the aggregation), as edge_windows_ref.py takes them.  Two forms
of the definition of include/anomod.h (anomod_edge_load_spans):

  edge_load_brute  the definition itself in Python integers, a loop over spans
                   x windows (T <= 512)
  edge_load_ref    the difference-table form in numpy u64 with cumsum, O(1) a
                   span (any T) — what the kernels do, restated

Every result is an integer table: results are compared bit for bit."""
import numpy as np

from anomod.spans import EdgeLoad, edge_rows
from oracle import native

U64 = 2**64
FIELDS = ("busy_us", "carried")


def _rows(sp):
    """(edge row, in-trace flag) per span position."""
    S = len(sp.services)
    edges = native.span_edges(sp, S).astype(np.int64) if sp.n_spans else np.zeros(0, np.int64)
    pos = np.arange(sp.n_spans)
    lo, hi = (int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])) if len(sp.trace_ptr) else (0, 0)
    return edges, (pos >= lo) & (pos < hi)


def edge_load_brute(sp, t0_us, step_us, T, start_us=None) -> EdgeLoad:
    assert T <= 512
    E = edge_rows(len(sp.services))
    ref = EdgeLoad.empty(sp.services, t0_us, step_us, T)
    start = sp.start_us if start_us is None else start_us
    edges, in_trace = _rows(sp)
    busy = [[0] * E for _ in range(T)]
    car = [[0] * E for _ in range(T)]
    outside = 0
    for i in range(sp.n_spans):
        if not in_trace[i]:
            continue
        s = int(start[i])
        e = min(s + int(sp.dur_us[i]), U64 - 1)
        r = int(edges[i])
        hit = False
        for w in range(T):
            lo, hi = t0_us + w * step_us, t0_us + (w + 1) * step_us
            ov = max(0, min(e, hi) - max(s, lo))
            if ov:
                busy[w][r] += ov
                hit = True
            if s < lo < e:
                car[w][r] += 1
                hit = True
        outside += not hit
        # the closed form of `outside`
        assert hit == (not (e == s or e <= t0_us or s >= t0_us + T * step_us))
    ref.busy_us[:] = np.asarray(busy, np.uint64).reshape(T, E)
    ref.carried[:] = np.asarray(car, np.uint64).reshape(T, E)
    ref.outside = outside
    return ref


def edge_load_ref(sp, t0_us, step_us, T, start_us=None) -> EdgeLoad:
    E = edge_rows(len(sp.services))
    ref = EdgeLoad.empty(sp.services, t0_us, step_us, T)
    start = sp.start_us if start_us is None else start_us
    edges, in_trace = _rows(sp)
    busy = ref.busy_us.reshape(-1)
    full = np.zeros(T * E, np.uint64)   # differences, negatives wrapped
    car = np.zeros(T * E, np.uint64)
    one, minus = np.uint64(1), np.uint64(U64 - 1)
    outside = 0
    end = t0_us + T * step_us           # (a Python integer: may pass 2^64)
    with np.errstate(over="ignore"):
        for i in np.nonzero(in_trace)[0].tolist():
            s = int(start[i])
            e = min(s + int(sp.dur_us[i]), U64 - 1)
            r = int(edges[i])
            if e == s or e <= t0_us or s >= end:
                outside += 1
                continue
            cs, ce = max(s, t0_us), min(e, end)          # clipped to the range
            a, b = (cs - t0_us) // step_us, (ce - 1 - t0_us) // step_us
            if a == b:
                busy[a * E + r] += np.uint64(ce - cs)
            else:
                busy[a * E + r] += np.uint64(t0_us + (a + 1) * step_us - cs)
                busy[b * E + r] += np.uint64(ce - (t0_us + b * step_us))
                full[(a + 1) * E + r] += one
                full[b * E + r] += minus
            f = 0 if s < t0_us else a + 1
            if f <= b:
                car[f * E + r] += one
                if b + 1 < T:
                    car[(b + 1) * E + r] += minus
        fullp = np.cumsum(full.reshape(T, E), axis=0, dtype=np.uint64)
        ref.busy_us += fullp * np.uint64(step_us)
        ref.carried[:] = np.cumsum(car.reshape(T, E), axis=0, dtype=np.uint64)
    ref.outside = outside
    return ref


def assert_load_equal(got: EdgeLoad, ref: EdgeLoad, fields=FIELDS):
    for k in fields:
        assert getattr(got, k).dtype == np.uint64 and getattr(got, k).shape == getattr(ref, k).shape
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    assert got.outside == ref.outside

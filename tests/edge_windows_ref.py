"""Reference for the windowed edge table (a plain helper, not a conftest).

Edge rows come from the C oracle (oracle.native.span_edges: the first-match
parent rule of the aggregation); the window rule is restated in Python
integers; the cells are filled with np.add.at / np.maximum.at.  Every result is
an integer table: GPU results are compared to it bit for bit."""
import numpy as np

from anomod.spans import EdgeWindows, edge_rows
from oracle import native

FIELDS = ("count", "errors", "sum_us", "max_us")


def formula_starts(sp, t0_us, period_us, gap_us):
    """start = t0 + (trace * period) // n_traces + pos_in_trace * gap (u64)."""
    lens = np.diff(sp.trace_ptr).astype(np.int64)
    trace = np.repeat(np.arange(sp.n_traces, dtype=np.uint64), lens)
    pos = np.arange(sp.n_spans, dtype=np.uint64) - np.repeat(sp.trace_ptr[:-1], lens)
    n_traces = np.uint64(max(sp.n_traces, 1))
    return (np.uint64(t0_us) + (trace * np.uint64(period_us)) // n_traces
            + pos * np.uint64(gap_us))


def windows_of(start_us, t0_us, step_us, T):
    """Window index per span, -1 for a span outside [0, T) (Python integers:
    start < t0 is tested before the subtraction, w against T, not end times)."""
    out = np.empty(len(start_us), np.int64)
    for i, s in enumerate(np.asarray(start_us, np.uint64).tolist()):
        w = (s - t0_us) // step_us if s >= t0_us else -1
        out[i] = w if 0 <= w < T else -1
    return out


def edge_windows_ref(sp, t0_us, step_us, T, start_us=None) -> EdgeWindows:
    S = len(sp.services)
    E = edge_rows(S)
    start = sp.start_us if start_us is None else start_us
    ref = EdgeWindows.empty(sp.services, t0_us, step_us, T)
    if sp.n_spans == 0:
        return ref
    edges = native.span_edges(sp, S).astype(np.int64)
    w = windows_of(start, t0_us, step_us, T)
    pos = np.arange(sp.n_spans)
    in_trace = (pos >= int(sp.trace_ptr[0])) & (pos < int(sp.trace_ptr[-1]))
    w[~in_trace] = -2            # spans outside every trace: in no cell, not in `outside`
    ok = w >= 0
    cell = w[ok] * E + edges[ok]
    dur = sp.dur_us[ok]
    np.add.at(ref.count.reshape(-1), cell, np.uint64(1))
    np.add.at(ref.errors.reshape(-1), cell, (sp.flags[ok] & 1).astype(np.uint64))
    np.add.at(ref.sum_us.reshape(-1), cell, dur.astype(np.uint64))
    np.maximum.at(ref.max_us.reshape(-1), cell, dur)
    ref.outside = int((w == -1).sum())
    return ref


def assert_windows_equal(got: EdgeWindows, ref: EdgeWindows, fields=FIELDS):
    for k in fields:
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    assert got.outside == ref.outside

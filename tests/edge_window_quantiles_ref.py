"""Reference for the per-window edge latency quantiles (a plain helper, not a
conftest).

Edge rows come from the C oracle (oracle.native.span_edges), windows from
edge_windows_ref.windows_of; per cell the durations are sorted with numpy and
the pick index is restated in Python: int(c * (q / 100.0)).  Every result is an
integer table: GPU results are compared to it bit for bit."""
import numpy as np

from anomod.spans import edge_rows
from oracle import native

from edge_windows_ref import windows_of


def pick_index(c: int, q: int) -> int:
    """The reference's int(n * q) with q the double q_pct / 100."""
    return int(c * (q / 100.0))


def edge_window_quantiles_ref(sp, t0_us, step_us, T, q_pct=(50, 99), start_us=None):
    """(count u64 [T, E], q_us u32 [T, E, nq], outside)."""
    S = len(sp.services)
    E = edge_rows(S)
    nq = len(q_pct)
    count = np.zeros((T, E), np.uint64)
    q_us = np.zeros((T, E, nq), np.uint32)
    if sp.n_spans == 0:
        return count, q_us, 0
    start = sp.start_us if start_us is None else start_us
    edges = native.span_edges(sp, S).astype(np.int64)
    w = windows_of(start, t0_us, step_us, T)
    pos = np.arange(sp.n_spans)
    in_trace = (pos >= int(sp.trace_ptr[0])) & (pos < int(sp.trace_ptr[-1]))
    w[~in_trace] = -2            # spans outside every trace: in no cell, not in `outside`
    ok = w >= 0
    cell = w[ok] * E + edges[ok]
    dur = sp.dur_us[ok]
    order = np.lexsort((dur, cell))
    cell, dur = cell[order], dur[order]
    cells, first, cnt = np.unique(cell, return_index=True, return_counts=True)
    cflat, qflat = count.reshape(-1), q_us.reshape(-1, nq)
    for c_id, b, c in zip(cells.tolist(), first.tolist(), cnt.tolist()):
        cflat[c_id] = c
        x = dur[b:b + c]
        for k, q in enumerate(q_pct):
            qflat[c_id, k] = x[pick_index(c, int(q))]
    return count, q_us, int((w == -1).sum())


def assert_quantiles_equal(got, ref):
    """got: an EdgeWindows of Context.edge_window_quantiles; ref: the helper's triple."""
    count, q_us, outside = ref
    assert got.q_us.dtype == np.uint32 and got.q_count.dtype == np.uint64
    np.testing.assert_array_equal(got.q_count, count, err_msg="count")
    np.testing.assert_array_equal(got.q_us, q_us, err_msg="q_us")
    assert got.outside == outside

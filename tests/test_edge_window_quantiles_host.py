"""Per-window edge latency quantiles, host side (no GPU): the reference helper
against two independent restatements, the pick-index rule, the third column
of EdgeWindows.matrix, trace_window_scores over three columns an edge, the ABI
symbol, and the evidence set — one call in ten to one service slowed in the
second half of a run — scored on the CPU restatement end to end."""
import re

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import EdgeTable, EdgeWindows, edge_rows
from conftest import ROOT
from oracle import native

from edge_window_quantiles_ref import edge_window_quantiles_ref, pick_index
from edge_windows_ref import edge_windows_ref, formula_starts, windows_of
from test_edge_windows_host import FAULT, STEP, T, T0

SLOW_TRACES = 12000   # per half: ~75 spans a (window, edge) cell on average
SLOW_EVERY = 10       # one call in ten to FAULT, in the second half
SLOW_MULT = 4         # its latency multiplied by this
TRACE_W = 6


def slow_set(n_traces=SLOW_TRACES, every=SLOW_EVERY, mult=SLOW_MULT):
    """Two normal halves spread in order over T windows; in the second half
    every `every`-th span served by FAULT takes `mult` times as long.  Chosen
    on the CPU (this file): with ~75 spans a cell the per-window mean of the
    faulted edges moves by 30 % while their p99 moves by 4x."""
    sp = anomod.SpanSet.concat([
        anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1), n_traces),
        anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1), n_traces, shard=1)])
    sp.start_us = formula_starts(sp, T0, T * STEP, 50)
    k = sp.services.index(FAULT)
    half = int(sp.trace_ptr[n_traces])
    hit = np.nonzero(sp.svc[half:] == k)[0][::every] + half
    d = sp.dur_us.astype(np.uint64)
    d[hit] *= np.uint64(mult)
    assert int(d.max()) < 2**32
    sp.dur_us = d.astype(np.uint32)
    return sp


def ref_windows(sp, t0, step, n_windows, q_pct):
    """The restated table with the helper's quantiles attached."""
    win = edge_windows_ref(sp, t0, step, n_windows)
    cnt, q_us, outside = edge_window_quantiles_ref(sp, t0, step, n_windows, q_pct)
    assert outside == win.outside
    win.q_pct, win.q_us, win.q_count = tuple(q_pct), q_us, cnt
    return win


def ref_scores(win, S, quantile):
    mm = win.matrix(5, quantile=quantile).pad_to_multiple(TRACE_W)
    Z = native.ewma_z(mm.X, 2.0 / (TRACE_W + 1), TRACE_W, eps=1e-2)
    return anomod.trace_window_scores(Z, win, S, 2 if quantile is None else 3)


@pytest.fixture(scope="module")
def small_set():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=3, p_orphan_ppm=20000), 400)
    sp.start_us = formula_starts(sp, T0, 8 * 1_000_000, 50)
    return sp


# ------------------------------------------------------------------ the helper
def test_helper_equals_dict_of_lists(small_set):
    sp = small_set
    S, E = sp.n_services, edge_rows(sp.n_services)
    q_pct = (0, 50, 95, 99)
    t0, step, n_windows = T0 + 1_500_000, 900_000, 6   # spans outside on both sides
    count, q_us, outside = edge_window_quantiles_ref(sp, t0, step, n_windows, q_pct)
    rows = native.span_edges(sp, S).tolist()
    cells: dict = {}
    n_out = 0
    for i, (s, d) in enumerate(zip(sp.start_us.tolist(), sp.dur_us.tolist())):
        w = (s - t0) // step if s >= t0 else -1
        if not 0 <= w < n_windows:
            n_out += 1
            continue
        cells.setdefault((w, rows[i]), []).append(d)
    assert 0 < n_out == outside < sp.n_spans
    assert count.shape == (n_windows, E) and q_us.shape == (n_windows, E, 4)
    assert q_us.dtype == np.uint32 and count.dtype == np.uint64
    assert int(np.count_nonzero(count)) == len(cells)
    for (w, r), x in cells.items():
        assert int(count[w, r]) == len(x)
        for k, q in enumerate(q_pct):
            assert int(q_us[w, r, k]) == sorted(x)[int(len(x) * q / 100.0)], (w, r, q)
    assert not q_us[count == 0].any()


def test_one_window_equals_the_exact_edge_quantiles(small_set):
    sp = small_set
    q_pct = (50, 90, 99)
    count, q_us, outside = edge_window_quantiles_ref(sp, 0, 2**62, 1, q_pct)
    assert outside == 0 and int(count.sum()) == sp.n_spans
    want = native.exact_quantiles(sp, q_pct)
    nz = count[0] > 0
    assert np.isnan(want[~nz]).all()
    np.testing.assert_array_equal(q_us[0][nz].astype(np.float64), want[nz])


def test_helper_count_equals_the_windowed_table(small_set):
    sp = small_set
    for t0, step, n_windows in ((T0, 1_000_000, 8), (T0 + 1_500_000, 900_000, 6)):
        count, _, outside = edge_window_quantiles_ref(sp, t0, step, n_windows, (50,))
        ref = edge_windows_ref(sp, t0, step, n_windows)
        np.testing.assert_array_equal(count, ref.count)
        assert outside == ref.outside


def test_pick_index_rule():
    """(u64)((double)c * ((double)q / 100.0)) == Python's int(c * (q / 100.0))
    and stays inside the cell, for every c in 1..1000 and q in 0..99."""
    c = np.arange(1, 1001, dtype=np.float64)
    for q in range(100):
        idx = (c * (np.float64(q) / np.float64(100.0))).astype(np.uint64)
        want = [pick_index(int(n), q) for n in range(1, 1001)]
        assert idx.tolist() == want, q
        assert (idx < c.astype(np.uint64)).all(), q
    assert pick_index(100, 99) == 99 and pick_index(101, 99) == 99 and pick_index(1, 99) == 0
    assert pick_index(2, 50) == 1 and pick_index(100, 0) == 0


# ------------------------------------------------------------------ matrix
def _hand_made():
    svcs = ["a", "b"]
    S = 2
    win = EdgeWindows.empty(svcs, 3_000_000, 500_000, 3)
    a_b, root_b = 0 * S + 1, S * S + 1
    win.count[:, a_b] = [7, 4, 0]
    win.sum_us[:, a_b] = [700, 400, 0]
    win.count[:, root_b] = [5, 0, 1]
    win.sum_us[:, root_b] = [15, 0, 9]
    win.q_pct = (50, 99)
    win.q_count = win.count.copy()
    win.q_us = np.zeros((3, edge_rows(S), 2), np.uint32)
    win.q_us[:, a_b, 0] = [90, 80, 0]
    win.q_us[:, a_b, 1] = [255, 300, 0]
    win.q_us[:, root_b, 0] = [3, 0, 9]
    win.q_us[:, root_b, 1] = [0, 0, 9]       # a cell whose p99 is 0: count tells it from empty
    return win


def test_matrix_without_quantile_is_unchanged():
    win = _hand_made()
    bare = EdgeWindows(win.services, win.t0_us, win.step_us, win.count, win.errors, win.sum_us,
                       win.max_us)   # positional construction, no quantile fields
    assert bare.q_pct is None and bare.q_us is None and bare.q_count is None
    for mc in (1, 5):
        a, b, c = bare.matrix(mc), win.matrix(mc), win.matrix(mc, quantile=None)
        assert a.X.tobytes() == b.X.tobytes() == c.X.tobytes()
        assert a.X.dtype == c.X.dtype == np.float32 and a.X.shape == c.X.shape
        assert a.series == b.series == c.series
        np.testing.assert_array_equal(a.timestamps, c.timestamps)
    with pytest.raises(ValueError):
        bare.matrix(quantile=99)


def test_matrix_third_column():
    win = _hand_made()
    mm = win.matrix(min_count=5, quantile=99)
    assert mm.X.dtype == np.float32 and mm.X.shape == (3, 6)
    lab = lambda p, c: (("parent", p), ("child", c))  # noqa: E731
    assert mm.series == [("edge_count", lab("a", "b")), ("edge_mean_us", lab("a", "b")),
                         ("edge_p99_us", lab("a", "b")),
                         ("edge_count", lab("ROOT", "b")), ("edge_mean_us", lab("ROOT", "b")),
                         ("edge_p99_us", lab("ROOT", "b"))]
    nan = np.nan
    want = np.array([
        [np.log2(8.0), np.log2(101.0), np.log2(256.0), np.log2(6.0), np.log2(4.0), 0.0],
        [np.log2(5.0), nan, nan, 0.0, nan, nan],
        [0.0, nan, nan, 1.0, nan, nan]], np.float64)
    np.testing.assert_array_equal(mm.X, want.astype(np.float32))
    two = win.matrix(min_count=5)
    np.testing.assert_array_equal(mm.X[:, 0::3], two.X[:, 0::2])
    np.testing.assert_array_equal(mm.X[:, 1::3], two.X[:, 1::2])
    # the other percentage, and min_count moving the NaN threshold
    m50 = win.matrix(min_count=1, quantile=50)
    assert m50.series[2] == ("edge_p50_us", lab("a", "b"))
    np.testing.assert_array_equal(
        m50.X[:, 2], np.array([np.log2(91.0), np.log2(81.0), nan]).astype(np.float32))
    np.testing.assert_array_equal(
        m50.X[:, 5], np.array([2.0, nan, np.log2(10.0)]).astype(np.float32))
    with pytest.raises(ValueError):
        win.matrix(quantile=95)   # not among q_pct
    # u32 extremes survive the f64 log
    win.q_us[0, 1, 1] = 2**32 - 1
    assert win.matrix(5, quantile=99).X[0, 2] == np.float32(32.0)


def test_trace_window_scores_three_columns():
    svcs = ["a", "b", "c"]
    S = 3
    win = EdgeWindows.empty(svcs, 0, 1, 4)
    rows = [0 * S + 1, 1 * S + 2, S * S + 1]   # a->b, b->c, ROOT->b
    for r in rows:
        win.count[0, r] = 1
    Z = np.zeros((41, 9), np.float32)
    Z[0] = 1e6                    # the first score window is dropped
    Z[5, 0], Z[9, 0] = 4.0, 2.0   # a->b count column: top-2 mean = 3
    Z[7, 5] = 8.0                 # b->c quantile column: top-2 mean = 4
    Z[3, 8], Z[4, 8] = 10.0, 6.0  # ROOT->b quantile column: 8 > 3
    got = anomod.trace_window_scores(Z, win, S, cols_per_edge=3)
    np.testing.assert_allclose(got, [0.0, 8.0, 4.0])
    # the default still reads two columns an edge: column 5 is ROOT->b's mean
    got2 = anomod.trace_window_scores(Z[:, :6], win, S)
    np.testing.assert_allclose(got2, [0.0, 4.0, 0.0])
    np.testing.assert_array_equal(got2, anomod.trace_window_scores(Z[:, :6], win, S, 2))


# ------------------------------------------------------------------ features
class HostContext:
    """Stand-in for Context built on the CPU references: what features() calls."""

    def __init__(self):
        self.calls = []

    def edge_aggregate(self, spans, with_hist=True):
        ref = native.finalize(native.edge_aggregate(spans))
        return EdgeTable(list(spans.services), ref["count"], ref["errors"], ref["sum_us"],
                         ref["min_us"], ref["max_us"], ref["p50_us"], ref["p99_us"],
                         ref["hist"] if with_hist else None)

    def edge_windows(self, spans, t0_us, step_us, n_windows):
        self.calls.append("edge_windows")
        return edge_windows_ref(spans, t0_us, step_us, n_windows)

    def edge_window_quantiles(self, spans, t0_us, step_us, n_windows, q_pct=(50, 99),
                              with_table=True):
        self.calls.append(("edge_window_quantiles", tuple(q_pct)))
        return ref_windows(spans, t0_us, step_us, n_windows, q_pct)

    def ewma_z(self, X, alpha, W, eps):
        return native.ewma_z(X, alpha, W, eps)


def test_features_trace_quantile_on_the_host(small_set):
    exp = anomod.Experiment("host", small_set, None, None, {})
    with pytest.raises(ValueError):
        anomod.features(exp, HostContext(), trace_quantile=99)   # needs trace_step_s
    with pytest.raises(ValueError):
        anomod.features(exp, HostContext(), trace_step_s=1.0, trace_quantile=100)
    c0, c1, c2 = HostContext(), HostContext(), HostContext()
    f0 = anomod.features(exp, c0, trace_step_s=1.0, trace_W=2)
    f1 = anomod.features(exp, c1, trace_step_s=1.0, trace_W=2, trace_quantile=None)
    f2 = anomod.features(exp, c2, trace_step_s=1.0, trace_W=2, trace_quantile=90)
    assert c0.calls == c1.calls == ["edge_windows"]
    assert c2.calls == [("edge_window_quantiles", (90,))]
    np.testing.assert_array_equal(f0.service_scores, f1.service_scores)
    assert "trace_quantile" not in f0.params and "trace_quantile" not in f1.params
    assert f2.params["trace_quantile"] == 90
    win = f2.edge_windows
    assert win.q_pct == (90,) and win.q_us.shape == win.count.shape + (1,)
    want = anomod.trace_window_scores(
        native.ewma_z(win.matrix(5, quantile=90).pad_to_multiple(2).X, 2.0 / 3, 2, eps=1e-2),
        win, small_set.n_services, 3)
    np.testing.assert_array_equal(f2.trace_window_scores, want)
    comp = f2.params["components"]
    np.testing.assert_array_equal(comp["trace"], want / (1 + want))


# ------------------------------------------------------------------ ABI
def test_abi_symbol_is_exported_and_listed():
    name = "anomod_edge_window_quantiles_spans"
    assert name in L.EXPORTED_SYMBOLS
    assert hasattr(anomod.lib(), name)
    text = (ROOT / "include" / "anomod.h").read_text()
    assert re.search(r"\bint " + name + r"\(anomod_ctx\*", text)
    assert "#define ANOMOD_ABI_VERSION 2" in text and L.ABI_VERSION == 2
    fields = [f for f, _ in L.EdgeWindowQuantilesC._fields_]
    assert fields == ["n_services", "n_windows", "t0_us", "step_us", "nq", "q_pct", "count",
                      "q_us", "outside"]


# ------------------------------------------------------------------ evidence
def test_slowed_tail_ranks_the_target_first():
    """The evidence set through the restatement: helper quantiles -> matrix ->
    oracle EWMA/z (eps 1e-2) -> trace_window_scores.  By the three-column score
    the target leads the runner-up by 1.5x at least (2.09x on this set: 11.76
    against 5.62; the two-column score gives 6.22 against 5.22)."""
    sp = slow_set()
    S = sp.n_services
    k = sp.services.index(FAULT)
    win = ref_windows(sp, T0, STEP, T, (99,))
    assert win.outside == 0 and int(win.q_count.sum()) == sp.n_spans
    np.testing.assert_array_equal(win.q_count, win.count)
    assert windows_of(sp.start_us[[0, -1]], T0, STEP, T).tolist() == [0, T - 1]
    two, three = ref_scores(win, S, None), ref_scores(win, S, 99)
    for name, ts in (("two-column", two), ("three-column", three)):
        order = np.argsort(-ts)
        print(f"{name}: target {ts[k]:.2f} (rank {int(np.nonzero(order == k)[0][0])}), "
              f"best other {sp.services[[i for i in order if i != k][0]]} "
              f"{max(ts[i] for i in range(S) if i != k):.2f}")
    order = np.argsort(-three)
    assert sp.services[order[0]] == FAULT
    assert three[order[0]] >= 1.5 * three[order[1]]
    assert three[k] > two[k]   # the tail series carries the lead

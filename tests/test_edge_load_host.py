"""Edge load, host side (no GPU): the two restatements of the definition
against each other, EdgeLoad.matrix, the load score rule, and the score term
end to end on the reference tables for a fault the start-window series cannot
see (calls of a quiet edge that hang for tens of windows)."""
import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import EdgeLoad, edge_rows
from oracle import native

from edge_load_ref import assert_load_equal, edge_load_brute, edge_load_ref
from edge_windows_ref import edge_windows_ref

T0 = 1_762_000_005_000_000  # a multiple of 15 s
STEP = 15_000_000
T = 120
W = 6
EPS = 1e-2
MIN_COUNT = 5
HANG_FROM = 60             # the window the hang begins in
HANG_US = 30 * STEP        # every call of the edge then lasts 30 windows longer


def singles(spans, S=2):
    """One single-span root trace per (start, dur) (edge ROOT -> svc)."""
    n = len(spans)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    return anomod.SpanSet([f"s{i}" for i in range(S)], np.arange(n + 1, dtype=np.uint64), ids, ids,
                          np.zeros(n, np.uint64), (np.arange(n) % S).astype(np.uint16),
                          np.zeros(n, np.uint16), np.asarray([d for _, d in spans], np.uint32),
                          unique_ids=True, start_us=np.asarray([s for s, _ in spans], np.uint64))


M = 10**6
U64 = 2**64
# (t0, step, T, [(start, dur), ...]): every border the definition names
BOUNDARY = [
    (M, 1000, 8, [
        (M + 3000, 500), (M + 3000, 1000), (M + 3000, 2500),      # s == lo_w
        (M + 2500, 500), (M + 1500, 1500),                        # e == lo_w (== hi_{w-1})
        (M + 2000, 1000), (M + 1500, 2500), (M + 2999, 1),        # e == hi_w
        (M + 100, 0), (M - 5, 0), (M + 8000, 0),                  # dur == 0
        (M - 300, 500), (M - 300, 5000), (M - 1, 2), (M - 300, 2**32 - 1),  # s < t0 < e
        (M - 300, 300), (M - 300, 299),                           # e == t0, e < t0
        (M + 7999, 1), (M + 7999, 2),                             # s == t0 + T * step - 1
        (M + 8000, 5), (M + 8100, 5), (U64 - 1, 7),               # s >= t0 + T * step
        (M, 8000), (M, 8001), (M + 1, 7998), (M + 999, 2), (M + 999, 1002),
    ]),
    # starts within 2^32 of 2^64: e saturates; t0 + T * step = 2^64
    (U64 - 2**33, 2**30, 8, [
        (U64 - 2**31, 2**32 - 1), (U64 - 2**32, 2**32 - 1), (U64 - 1, 5), (U64 - 2, 5),
        (U64 - 2**30, 2**30), (U64 - 2**30 - 1, 2**31), (U64 - 2**33 - 7, 2**32 - 1),
    ]),
    # t0 + T * step > 2^64
    (U64 - 2**41, 2**40, 4, [
        (U64 - 2**41, 2**32 - 1), (U64 - 2**40, 1), (U64 - 2**40 - 1, 2), (U64 - 3, 2**32 - 1),
        (U64 - 2**41 - 1, 1), (U64 - 2**41 - 1, 2),
    ]),
    (1, U64 - 1, 2, [(0, 1), (0, 2), (1, 5), (U64 - 1, 1), (U64 - 2, 9)]),
    # step = 1, T = 1
    (M, 1, 1, [(M, 1), (M - 1, 3), (M, 5), (M + 1, 1), (M - 1, 1), (M - 2, 2**32 - 1)]),
    (M, 1, 5, [(M + 1, 3), (M - 2, 4), (M + 4, 1), (M + 4, 9), (M + 5, 1), (M, 5)]),
]


def random_case(rng, n=40):
    """Small random spans around a small window range (both borders crossed)."""
    t0 = int(rng.integers(50, 200))
    step = int(rng.integers(1, 12))
    n_windows = int(rng.integers(1, 9))
    span = n_windows * step
    starts = rng.integers(t0 - 20, t0 + span + 10, n)
    durs = np.where(rng.random(n) < 0.15, 0, rng.integers(0, 3 * span + 2, n))
    return t0, step, n_windows, list(zip(starts.tolist(), durs.tolist()))


def hang_set():
    """(fault-free set, hung set, edge row, child service): SN traces laid out
    so that every window holds the same mix (12 / 6 / 2 traces of the 7- / 8- /
    20-span kinds), so every edge of the 20-span kind alone gets the same few
    calls in every window.  In the hung set the calls of one such edge that
    start in window HANG_FROM or later last HANG_US longer; start times are
    unchanged."""
    per = {7: 12, 8: 6, 20: 2}
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1), 8000)
    lens = np.diff(sp.trace_ptr).astype(np.int64)
    keep = np.zeros(sp.n_traces, bool)
    for k, c in per.items():
        keep[np.nonzero(lens == k)[0][: c * T]] = True
    sp = sp.select_traces(keep)
    lens = np.diff(sp.trace_ptr).astype(np.int64)
    t_start = np.zeros(sp.n_traces, np.uint64)
    for k, c in per.items():
        idx = np.nonzero(lens == k)[0]
        assert idx.shape[0] == c * T
        r = np.arange(idx.shape[0])
        t_start[idx] = T0 + (r // c) * STEP + (r % c) * 700_000 + k * 1000
    pos = np.arange(sp.n_spans, dtype=np.uint64) - np.repeat(sp.trace_ptr[:-1], lens)
    sp.start_us = np.repeat(t_start, lens) + pos * np.uint64(50)
    S = sp.n_services
    win = edge_windows_ref(sp, T0, STEP, T)
    quiet = np.nonzero((win.count.max(axis=0) < MIN_COUNT) & (win.count.min(axis=0) >= 1))[0]
    assert quiet.size > 0
    row = int(quiet[0])
    edges = native.span_edges(sp, S).astype(np.int64)
    hung = sp.select_traces(np.ones(sp.n_traces, bool))
    hung.start_us = sp.start_us.copy()
    late = (edges == row) & (sp.start_us >= T0 + HANG_FROM * STEP)
    assert late.any()
    hung.dur_us = sp.dur_us.copy()
    hung.dur_us[late] += np.uint32(HANG_US)
    return sp, hung, row, row % S


def load_scores_ref(sp):
    """(EdgeLoad, per-column reduced score, per-service score) through the
    restatement: reference table -> matrix -> oracle EWMA/z -> the load rule."""
    load = edge_load_ref(sp, T0, STEP, T)
    mm = load.matrix().pad_to_multiple(W)
    Z = native.ewma_z(mm.X, 2.0 / (W + 1), W, eps=EPS)
    Zl = np.asarray(Z, np.float64)[1:]
    k = max(1, Zl.shape[0] // 20)
    cols = np.sort(Zl, axis=0)[-k:].mean(axis=0)
    return load, cols, anomod.load_window_scores(Z, load, sp.n_services)


# ------------------------------------------------------------------ the references
def test_abi_has_the_entry_point():
    assert "anomod_edge_load_spans" in anomod.EXPORTED_SYMBOLS
    assert hasattr(anomod.Context, "edge_load")
    assert anomod.lib().anomod_edge_load_scan_segment() >= 2
    assert L.STAGE_EDGE_LOAD == 11 and L.STAGE_EDGE_LOAD_KERNEL == 12


@pytest.mark.parametrize("case", range(len(BOUNDARY)))
def test_ref_equals_brute_on_the_boundary_table(case):
    t0, step, n_windows, spans = BOUNDARY[case]
    for sub in [[s] for s in spans] + [spans]:
        sp = singles(sub)
        assert_load_equal(edge_load_ref(sp, t0, step, n_windows),
                          edge_load_brute(sp, t0, step, n_windows))


def test_boundary_singles_by_hand():
    t0, step, n_windows, _ = BOUNDARY[0]

    def one(s, d):
        r = edge_load_ref(singles([(s, d)]), t0, step, n_windows)
        return r.busy_us[:, 4].tolist(), r.carried[:, 4].tolist(), r.outside  # ROOT -> s0

    z = [0] * 8
    assert one(M + 3000, 1000) == ([0, 0, 0, 1000, 0, 0, 0, 0], z, 0)      # arrival, not carried
    assert one(M + 2500, 500) == ([0, 0, 500, 0, 0, 0, 0, 0], z, 0)        # e == lo_3: not open there
    assert one(M + 1500, 2500) == ([0, 500, 1000, 1000, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0], 0)
    assert one(M - 300, 500) == ([200, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], 0)  # clipped
    assert one(M - 300, 300) == (z, z, 1) and one(M + 100, 0) == (z, z, 1)
    assert one(M + 7999, 2) == ([0, 0, 0, 0, 0, 0, 0, 1], z, 0)
    assert one(M + 8000, 5) == (z, z, 1)
    assert one(M - 300, 2**32 - 1) == ([1000] * 8, [1] * 8, 0)


def test_ref_equals_brute_on_random_cases():
    rng = np.random.default_rng(11)
    for _ in range(150):
        t0, step, n_windows, spans = random_case(rng)
        sp = singles(spans, S=3)
        ref = edge_load_ref(sp, t0, step, n_windows)
        assert_load_equal(ref, edge_load_brute(sp, t0, step, n_windows))
        assert ref.outside < len(spans)


def test_ref_on_a_synthetic_set_with_parents():
    from edge_windows_ref import formula_starts

    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=3, p_orphan_ppm=20000), 60)
    sp.start_us = formula_starts(sp, M, 40_000, 50)
    for step, n_windows in ((1000, 40), (97, 512), (50_000, 1)):
        ref = edge_load_ref(sp, M, step, n_windows)
        assert_load_equal(ref, edge_load_brute(sp, M, step, n_windows))
    # a range that holds every span whole: busy sums to the latency sum per edge
    ref = edge_load_ref(sp, M, 1000, 512)
    assert ref.outside == int((sp.dur_us == 0).sum())
    edges = native.span_edges(sp, sp.n_services).astype(np.int64)
    want = np.zeros(edge_rows(sp.n_services), np.uint64)
    np.add.at(want, edges, sp.dur_us.astype(np.uint64))
    np.testing.assert_array_equal(ref.busy_us.sum(axis=0), want)


# ------------------------------------------------------------------ matrix, score rule
def test_edge_load_matrix_hand_made():
    svcs = ["a", "b"]
    S, E = 2, 8
    load = EdgeLoad.empty(svcs, 3_000_000, 500_000, 3)
    assert load.busy_us.shape == load.carried.shape == (3, E)
    assert load.busy_us.dtype == load.carried.dtype == np.uint64 and load.n_windows == 3
    a_b, root_b, orph_a = 0 * S + 1, S * S + 1, (S + 1) * S
    load.busy_us[:, a_b] = [7, 0, 2**40]
    load.carried[1, root_b] = 3        # active by its carried total alone
    load.busy_us[2, orph_a] = 1
    np.testing.assert_array_equal(load.active_rows(), [a_b, root_b, orph_a])
    mm = load.matrix()
    assert isinstance(mm, anomod.MetricMatrix)
    assert mm.X.dtype == np.float32 and mm.X.shape == (3, 3) and np.isfinite(mm.X).all()
    lab = lambda p, c: (("parent", p), ("child", c))  # noqa: E731
    assert mm.series == [("edge_busy_us", lab("a", "b")), ("edge_busy_us", lab("ROOT", "b")),
                         ("edge_busy_us", lab("ORPHAN", "a"))]
    want = np.array([[3.0, 0.0, 0.0], [0.0, 0.0, 0.0],
                     [np.log2(1.0 + 2.0**40), 0.0, 1.0]], np.float64)
    np.testing.assert_array_equal(mm.X, want.astype(np.float32))
    np.testing.assert_array_equal(mm.timestamps, np.array([3.0, 3.5, 4.0]))
    assert EdgeLoad.empty(svcs, 0, 1, 4).matrix().X.shape == (4, 0)


def test_load_window_scores_pure():
    svcs = ["a", "b", "c"]
    S = 3
    load = EdgeLoad.empty(svcs, 0, 1, 4)
    for r in (0 * S + 1, 1 * S + 2, S * S + 1):   # a->b, b->c, ROOT->b
        load.busy_us[0, r] = 1
    Z = np.zeros((41, 3), np.float32)
    Z[0] = 1e6                    # the first score window is dropped
    Z[5, 0], Z[9, 0] = 4.0, 2.0   # a->b: top-2 mean = 3
    Z[7, 1] = 8.0                 # b->c: 4
    Z[3, 2], Z[4, 2] = 10.0, 6.0  # ROOT->b: 8 > 3
    np.testing.assert_allclose(anomod.load_window_scores(Z, load, S), [0.0, 8.0, 4.0])
    assert anomod.load_window_scores(Z[:1], load, S).tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ the constructed fault
def test_hang_on_a_quiet_edge_shows_in_the_load_term_only():
    base, hung, row, child = hang_set()
    S = base.n_services
    # the start-window table's scored series cannot move: identical matrices
    wb = edge_windows_ref(base, T0, STEP, T)
    wh = edge_windows_ref(hung, T0, STEP, T)
    assert int(wb.count[:, row].max()) < MIN_COUNT and int(wb.count[:, row].min()) >= 1
    np.testing.assert_array_equal(wh.count, wb.count)
    assert int(wh.sum_us[:, row].sum()) > int(wb.sum_us[:, row].sum())
    mb, mh = wb.matrix(MIN_COUNT), wh.matrix(MIN_COUNT)
    assert mb.series == mh.series
    np.testing.assert_array_equal(mh.X, mb.X)   # (NaNs in the same places)
    # the load table does move, in that edge's column first of all
    load, cols, ls = load_scores_ref(hung)
    load0, cols0, ls0 = load_scores_ref(base)
    active = load.active_rows()
    np.testing.assert_array_equal(active, load0.active_rows())
    col = int(np.nonzero(active == row)[0][0])
    print("hung edge row", row, "column score", cols[col], "fault-free", cols0[col],
          "next", np.sort(cols)[-2])
    assert int(np.argmax(cols)) == col
    others = np.arange(cols.shape[0]) != col
    np.testing.assert_array_equal(cols[others], cols0[others])
    assert load.carried[HANG_FROM + 5, row] > 0 and not load0.carried[:, row].any()
    comp = ls / (1.0 + ls)
    print("load component:", dict(zip(hung.services, np.round(comp, 3))))
    assert int(np.argmax(comp)) == child
    assert int(np.argmax(ls0 / (1.0 + ls0))) != child or ls0[child] < ls[child]


def test_trace_load_needs_a_step():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1), 10)
    exp = anomod.Experiment("x", sp, None, None, {})
    with pytest.raises(ValueError, match="trace_step_s"):
        anomod.features(exp, trace_load=True)

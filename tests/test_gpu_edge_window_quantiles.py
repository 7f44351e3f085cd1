"""GPU: the per-window edge latency quantiles (csrc/edge_window_quantiles.hip)
against the reference helper (tests/edge_window_quantiles_ref.py), bit for bit
— no tolerance anywhere — plus the relations to the windowed table and to the
whole-run exact quantiles, the error codes, and the quantile trace term of
features() on the evidence set.

ANOMOD_EDGE_WINDOW_QUANTILES_WGS caps the workgroups of the two stream kernels:
results must not depend on it."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import edge_rows
from oracle import native

from edge_window_quantiles_ref import assert_quantiles_equal, edge_window_quantiles_ref
from edge_windows_ref import (assert_windows_equal, edge_windows_ref, formula_starts,
                              windows_of)
from test_edge_window_quantiles_host import slow_set
from test_edge_windows_host import FAULT, STEP, T, T0

pytestmark = pytest.mark.gpu

T0_US = 1_762_000_000_000_000
# workgroup cap: default geometry, one workgroup over the whole set, a few
GEOMETRIES = [None, "1", "3"]


def _geometry(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("ANOMOD_EDGE_WINDOW_QUANTILES_WGS", raising=False)
    else:
        monkeypatch.setenv("ANOMOD_EDGE_WINDOW_QUANTILES_WGS", cap)


def _check(ctx, sp, t0, step, n_windows, q_pct=(50, 99)):
    got = ctx.edge_window_quantiles(sp, t0, step, n_windows, q_pct=q_pct, with_table=False)
    assert got.q_pct == tuple(q_pct)
    assert_quantiles_equal(got, edge_window_quantiles_ref(sp, t0, step, n_windows, q_pct))
    return got


@pytest.fixture(scope="module")
def sn_set():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)
    sp.start_us = formula_starts(sp, T0_US, 64 * 1_000_000, 50)
    return sp


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("cap", GEOMETRIES)
def test_sn_time_ordered(ctx, sn_set, monkeypatch, cap):
    _geometry(monkeypatch, cap)
    got = _check(ctx, sn_set, T0_US, 1_000_000, 64)
    assert got.outside == 0 and int(got.q_count.sum()) == sn_set.n_spans
    # a window range that leaves spans outside on both sides
    got = _check(ctx, sn_set, T0_US + 5_500_000, 700_000, 40)
    assert 0 < got.outside < sn_set.n_spans


@pytest.mark.parametrize("cap", GEOMETRIES)
def test_sn_random_trace_times(ctx, sn_set, monkeypatch, cap):
    _geometry(monkeypatch, cap)
    rng = np.random.default_rng(2)
    lens = np.diff(sn_set.trace_ptr).astype(np.int64)
    t_start = rng.integers(0, 64 * 1_000_000 - 1000, sn_set.n_traces).astype(np.uint64)
    pos = np.arange(sn_set.n_spans, dtype=np.uint64) - np.repeat(sn_set.trace_ptr[:-1], lens)
    sp = sn_set.select_traces(np.ones(sn_set.n_traces, bool))
    sp.start_us = np.uint64(T0_US) + np.repeat(t_start, lens) + pos * np.uint64(50)
    got = _check(ctx, sp, T0_US, 1_000_000, 64)
    assert got.outside == 0


@pytest.mark.parametrize("cap", GEOMETRIES)
def test_trainticket_width(ctx, monkeypatch, cap):
    _geometry(monkeypatch, cap)
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=11, p_orphan_ppm=5000), 1500)
    assert edge_rows(sp.n_services) == 2208
    sp.start_us = formula_starts(sp, T0_US, 32 * 2_000_000, 120)
    got = _check(ctx, sp, T0_US, 2_000_000, 32)
    assert int(got.q_count.sum()) + got.outside == sp.n_spans


@pytest.fixture(scope="module")
def long_set():
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=5, p_orphan_ppm=10000), 300)
    lens = np.diff(sp.trace_ptr)
    assert lens.max() > 2000 and lens.min() >= 16
    sp.start_us = formula_starts(sp, T0_US, 16 * 3_000_000, 40)
    return sp, edge_window_quantiles_ref(sp, T0_US, 3_000_000, 16, (50, 99))


@pytest.mark.parametrize("cap", GEOMETRIES)
@pytest.mark.parametrize("unique", [True, False])
def test_long_traces(ctx, long_set, monkeypatch, cap, unique):
    """Traces of 16..4000 spans: the big-trace key pass under both scans."""
    _geometry(monkeypatch, cap)
    sp, ref = long_set
    sp.unique_ids = unique
    got = ctx.edge_window_quantiles(sp, T0_US, 3_000_000, 16, with_table=False)
    assert_quantiles_equal(got, ref)


def _adversarial():
    """Single-span root traces (edge ROOT -> svc) in shuffled order, windows of
    2^40 us from t0 = 2^64 - 2^41: t0 + T * step passes 2^64, so only windows
    0 and 1 can hold a span.
      svc 0: 3000 spans in one cell (window 0), all of duration 777
      svc 1..4: cells of exactly 1, 2, 100 and 101 spans in window 1
      svc 5: durations 0 and 2^32 - 1 in window 0 (plus three spans of 0 in
             window 1: a non-empty cell whose every pick is 0); starts below t0
    and five spans before trace_ptr[0] / four after the last trace, with
    in-window starts, that lie in no trace."""
    rng = np.random.default_rng(9)
    t0, step, n_windows = 2**64 - 2**41, 2**40, 4
    rec = [(0, t0 + int(rng.integers(0, step)), 777) for _ in range(3000)]
    for svc, c in ((1, 1), (2, 2), (3, 100), (4, 101)):
        rec += [(svc, t0 + step + int(rng.integers(0, step)), int(rng.integers(0, 2**32)))
                for _ in range(c)]
    rec += [(5, t0, 0), (5, t0 + step - 1, 2**32 - 1), (5, t0 + 7, 2**32 - 1), (5, t0 + 8, 0),
            (5, t0 + 9, 12345)]
    rec += [(5, 2**64 - 1 - k, 0) for k in range(3)]
    rec += [(5, t0 - 1, 5), (5, 0, 6), (5, t0 - 2**40, 7)] + [(k % 5, 17 * k, 9) for k in range(40)]
    rec = [rec[i] for i in rng.permutation(len(rec))]
    stray = [(1, t0 + step + 3, 1)] * 5
    rec = stray + rec + [(2, t0 + 5, 2)] * 4
    n = len(rec)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ptr = np.arange(5, n - 4 + 1, dtype=np.uint64)
    sp = anomod.SpanSet([f"s{i}" for i in range(6)], ptr, ids, ids, np.zeros(n, np.uint64),
                        np.asarray([r[0] for r in rec], np.uint16), np.zeros(n, np.uint16),
                        np.asarray([r[2] for r in rec], np.uint32), unique_ids=True,
                        start_us=np.asarray([r[1] for r in rec], np.uint64))
    return sp, t0, step, n_windows


@pytest.mark.parametrize("cap", GEOMETRIES)
def test_adversarial_cells(ctx, monkeypatch, cap):
    _geometry(monkeypatch, cap)
    sp, t0, step, n_windows = _adversarial()
    S = 6
    assert t0 + n_windows * step > 2**64 and int(sp.trace_ptr[0]) == 5
    q_pct = (0, 50, 99)
    got = _check(ctx, sp, t0, step, n_windows, q_pct)
    root = S * S   # row of ROOT -> s0
    assert got.outside == 43
    assert int(got.q_count.sum()) == sp.n_spans - 9 - 43
    assert int(got.q_count[0, root]) == 3000 and got.q_us[0, root].tolist() == [777] * 3
    assert [int(got.q_count[1, root + s]) for s in (1, 2, 3, 4)] == [1, 2, 100, 101]
    one = got.q_us[1, root + 1]
    assert one[0] == one[1] == one[2]                       # c = 1: every pick is the span
    two = got.q_us[1, root + 2]
    assert two[0] <= two[1] == two[2]                       # c = 2: int(2 * .5) = 1
    assert int(got.q_count[0, root + 5]) == 5
    assert got.q_us[0, root + 5].tolist() == [0, 12345, 2**32 - 1]
    assert int(got.q_count[1, root + 5]) == 3 and not got.q_us[1, root + 5].any()
    assert not got.q_count[2:].any() and not got.q_us[2:].any()


def test_cells_near_the_limit(ctx):
    """T * E = 65536 * 168 = 11 M cells (the limit is 2^24), a few hundred spans."""
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=4), 40)
    assert edge_rows(sp.n_services) == 168
    sp.start_us = formula_starts(sp, T0_US, 65536 * 1000, 3)
    got = _check(ctx, sp, T0_US, 1000, 65536, q_pct=(99,))
    assert got.outside == 0 and int(got.q_count.sum()) == sp.n_spans
    assert int(np.count_nonzero(got.q_count.any(axis=1))) >= 30   # spread over the windows


@pytest.mark.parametrize("q_pct", [(99,), (0,), (0, 99, 50, 50, 1, 98, 99, 0)])
def test_one_and_eight_picks(ctx, sn_set, q_pct):
    _check(ctx, sn_set, T0_US, 4_000_000, 16, q_pct)


# ------------------------------------------------------------------ relations
def test_relations_on_the_sn_set(ctx, sn_set):
    S = sn_set.n_services
    got = ctx.edge_window_quantiles(sn_set, T0_US, 1_000_000, 64, q_pct=(0, 99))
    tab = ctx.edge_windows(sn_set, T0_US, 1_000_000, 64)
    # with_table: the four tables of edge_windows ride along
    assert_windows_equal(got, tab)
    np.testing.assert_array_equal(got.q_count, tab.count)
    # q = 0: the per-cell minimum
    w = windows_of(sn_set.start_us, T0_US, 1_000_000, 64)
    assert got.outside == 0 and (w >= 0).all()
    cell = w * edge_rows(S) + native.span_edges(sn_set, S).astype(np.int64)
    mn = np.full(64 * edge_rows(S), 2**32 - 1, np.uint32)
    np.minimum.at(mn, cell, sn_set.dur_us)
    mn[tab.count.reshape(-1) == 0] = 0
    np.testing.assert_array_equal(got.q_us[:, :, 0].reshape(-1), mn)
    # c <= 100: int(c * .99) = c - 1, the cell's maximum
    small = (tab.count > 0) & (tab.count <= 100)
    assert small.sum() > 100
    np.testing.assert_array_equal(got.q_us[:, :, 1][small], tab.max_us[small])
    # one window over everything: the whole-run exact quantiles, as doubles
    q_pct = (50, 95, 99)
    one = ctx.edge_window_quantiles(sn_set, 0, 2**62, 1, q_pct=q_pct, with_table=False)
    exact, cnt = ctx.edge_quantiles_exact(sn_set, q_pct)
    np.testing.assert_array_equal(one.q_count[0], cnt)
    nz = cnt > 0
    assert nz.sum() > 10 and np.isnan(exact[~nz]).all()
    np.testing.assert_array_equal(one.q_us[0][nz].astype(np.float64), exact[nz])
    assert not one.q_us[0][~nz].any()


def test_a_device_set_and_repeated_calls(ctx, sn_set):
    """A device set keeps its columns across calls; the workspace of a call is
    its own (a small call after a large one reads no stale cell)."""
    dev = ctx.upload(sn_set)
    ref = edge_window_quantiles_ref(sn_set, T0_US, 1_000_000, 64, (50, 99))
    assert_quantiles_equal(ctx.edge_window_quantiles(dev, T0_US, 1_000_000, 64, with_table=False),
                           ref)
    small = sn_set.select_traces(np.arange(sn_set.n_traces) % 7 == 0)
    _check(ctx, small, T0_US + 20_000_000, 3_000_000, 8)
    assert_quantiles_equal(ctx.edge_window_quantiles(dev, T0_US, 1_000_000, 64, with_table=False),
                           ref)
    np.testing.assert_array_equal(dev.start_us(), sn_set.start_us)
    dev.free()


# ------------------------------------------------------------------ errors
def _raw_call(ctx, dev, S, n_windows, t0, step, q_pct=(50, 99), nq=None, cells=None):
    q = np.asarray(q_pct if len(q_pct) else (0,), np.uint32)
    nq = len(q_pct) if nq is None else nq
    cells = n_windows * edge_rows(S) if cells is None else cells
    cnt = np.zeros(max(cells, 1), np.uint64)
    out = np.zeros(max(cells, 1) * max(nq, 1), np.uint32)
    cs = L.EdgeWindowQuantilesC(S, n_windows, t0, step, nq, L.ptr(q, C.c_uint32),
                                L.ptr(cnt, C.c_uint64), L.ptr(out, C.c_uint32), 0)
    return L.lib().anomod_edge_window_quantiles_spans(ctx.handle, dev.handle, C.byref(cs))


def test_errors_and_empty_input(ctx, sn_set):
    S = sn_set.n_services
    bare = sn_set.select_traces(np.arange(sn_set.n_traces) < 50)
    bare.start_us = None
    dev = ctx.upload(bare)
    assert _raw_call(ctx, dev, S, 8, 0, 1000) == L.ESTATE       # no start column
    assert b"start" in L.lib().anomod_last_error(ctx.handle)
    with pytest.raises(anomod.AnomodError) as e:
        ctx.edge_window_quantiles(dev, 0, 1000, 8)
    assert e.value.status == L.ESTATE
    with pytest.raises(ValueError):
        ctx.edge_window_quantiles(bare, 0, 1000, 8)
    dev.set_start_us(np.zeros(dev.n_spans, np.uint64))
    assert _raw_call(ctx, dev, S, 8, 0, 1000) == L.OK
    # T * E > 2^24 (the arrays are never touched), T out of range, step 0
    assert _raw_call(ctx, dev, 46, (1 << 24) // 2208 + 1, 0, 1000, cells=1) == L.EINVAL
    assert _raw_call(ctx, dev, S, 65537, 0, 1000, cells=1) == L.EINVAL
    assert _raw_call(ctx, dev, S, 0, 0, 1000, cells=1) == L.EINVAL
    assert _raw_call(ctx, dev, S, 8, 0, 0) == L.EINVAL
    # nq 0 and 9, a percentage of 100
    assert _raw_call(ctx, dev, S, 8, 0, 1000, q_pct=(), nq=0) == L.EINVAL
    assert _raw_call(ctx, dev, S, 8, 0, 1000, q_pct=(1, 2, 3, 4, 5, 6, 7, 8, 9)) == L.EINVAL
    assert _raw_call(ctx, dev, S, 8, 0, 1000, q_pct=(1, 2, 3, 4, 5, 6, 7, 8)) == L.OK
    assert _raw_call(ctx, dev, S, 8, 0, 1000, q_pct=(50, 100)) == L.EINVAL
    for bad in ((), tuple(range(9)), (100,), (-1,)):
        with pytest.raises(anomod.AnomodError) as e:
            ctx.edge_window_quantiles(dev, 0, 1000, 8, q_pct=bad)
        assert e.value.status == L.EINVAL
    # a service index >= S
    assert _raw_call(ctx, dev, int(bare.svc.max()), 8, 0, 1000) == L.EINVAL
    assert b"service index" in L.lib().anomod_last_error(ctx.handle)
    # an ungrouped set
    ung = ctx.upload_ungrouped(bare)
    ung.set_start_us(np.zeros(ung.n_spans, np.uint64))
    assert _raw_call(ctx, ung, S, 8, 0, 1000) == L.ESTATE
    assert b"not grouped" in L.lib().anomod_last_error(ctx.handle)
    dev.free()
    ung.free()
    # an empty set: zeros
    empty = bare.select_traces(np.zeros(bare.n_traces, bool))
    empty.start_us = np.zeros(0, np.uint64)
    got = ctx.edge_window_quantiles(empty, 5, 1000, 8)
    assert got.outside == 0 and not got.q_us.any() and not got.q_count.any()
    assert got.q_us.shape == (8, edge_rows(S), 2) and not got.count.any()


# ------------------------------------------------------------------ end to end
def test_quantile_trace_term_on_the_evidence_set(ctx):
    sp = slow_set()
    exp = anomod.Experiment("synthetic_slow_tail", sp, None, FAULT, {})
    f = anomod.features(exp, ctx, trace_step_s=STEP / 1e6, trace_W=6, trace_quantile=99)
    assert f.params["trace_quantile"] == 99
    win = f.edge_windows
    assert (win.t0_us, win.step_us, win.n_windows) == (T0, STEP, T) and win.q_pct == (99,)
    assert_windows_equal(win, edge_windows_ref(sp, T0, STEP, T))
    assert_quantiles_equal(win, edge_window_quantiles_ref(sp, T0, STEP, T, (99,)))
    ts = f.trace_window_scores
    order = np.argsort(-ts)
    print("three-column trace scores:", dict(zip(sp.services, np.round(ts, 2))))
    assert sp.services[order[0]] == FAULT
    assert sp.services[int(np.argmax(f.params["components"]["trace"]))] == FAULT
    # without a quantile nothing changes: the default is the explicit None
    f0 = anomod.features(exp, ctx, trace_step_s=STEP / 1e6, trace_W=6)
    f1 = anomod.features(exp, ctx, trace_step_s=STEP / 1e6, trace_W=6, trace_quantile=None)
    np.testing.assert_array_equal(f0.service_scores, f1.service_scores)
    np.testing.assert_array_equal(f0.trace_window_scores, f1.trace_window_scores)
    assert "trace_quantile" not in f0.params and f0.edge_windows.q_us is None
    assert_windows_equal(f0.edge_windows, win)
    print("two-column trace scores:  ", dict(zip(sp.services, np.round(f0.trace_window_scores, 2))))

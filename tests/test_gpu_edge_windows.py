"""GPU: the windowed edge table (csrc/edge_windows.hip) against the reference
helper (tests/edge_windows_ref.py), bit for bit — no tolerance anywhere on the
table — plus the start-time column plumbing and the trace term of features().

ANOMOD_EDGE_WINDOWS_WGS / ANOMOD_EDGE_WINDOWS_TILE cap the window kernel's
workgroups and LDS tile windows: the small sets here would otherwise give every
workgroup a single batch (no tile movement) — results must not depend on them."""
import ctypes as C
import shutil

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import edge_rows
from oracle import native

from edge_windows_ref import (FIELDS, assert_windows_equal, edge_windows_ref, formula_starts,
                              windows_of)
from test_edge_windows_host import FAULT, STEP, T, T0, fault_set

pytestmark = pytest.mark.gpu

T0_US = 1_762_000_000_000_000
# (workgroup cap, tile-window cap): default geometry, one workgroup walking the
# whole set, three workgroups with a 2-window ring, every span to global atomics
GEOMETRIES = [(None, None), ("1", None), ("3", "2"), (None, "0")]


def _geometry(monkeypatch, geom):
    for name, v in zip(("ANOMOD_EDGE_WINDOWS_WGS", "ANOMOD_EDGE_WINDOWS_TILE"), geom):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _check(ctx, sp, t0, step, n_windows):
    got = ctx.edge_windows(sp, t0, step, n_windows)
    ref = edge_windows_ref(sp, t0, step, n_windows)
    assert_windows_equal(got, ref)
    return got


@pytest.fixture(scope="module")
def sn_set():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)
    sp.start_us = formula_starts(sp, T0_US, 64 * 1_000_000, 50)
    return sp


# 1
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_sn_time_ordered(ctx, sn_set, monkeypatch, geom):
    _geometry(monkeypatch, geom)
    got = _check(ctx, sn_set, T0_US, 1_000_000, 64)
    assert got.outside == 0
    table = ctx.edge_aggregate(sn_set, with_hist=False)
    np.testing.assert_array_equal(got.count.sum(axis=0), table.count)
    np.testing.assert_array_equal(got.errors.sum(axis=0), table.errors)
    np.testing.assert_array_equal(got.sum_us.sum(axis=0), table.sum_us)
    np.testing.assert_array_equal(got.max_us.max(axis=0), table.max_us)
    # a window range that leaves spans outside on both sides
    got = _check(ctx, sn_set, T0_US + 5_500_000, 700_000, 40)
    assert 0 < got.outside < sn_set.n_spans


# 2
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_sn_random_trace_times(ctx, sn_set, monkeypatch, geom):
    """Every trace at a random time: tiles miss, the global path carries it."""
    _geometry(monkeypatch, geom)
    rng = np.random.default_rng(2)
    lens = np.diff(sn_set.trace_ptr).astype(np.int64)
    t_start = rng.integers(0, 64 * 1_000_000 - 1000, sn_set.n_traces).astype(np.uint64)
    pos = np.arange(sn_set.n_spans, dtype=np.uint64) - np.repeat(sn_set.trace_ptr[:-1], lens)
    sp = sn_set.select_traces(np.ones(sn_set.n_traces, bool))
    sp.start_us = np.uint64(T0_US) + np.repeat(t_start, lens) + pos * np.uint64(50)
    got = _check(ctx, sp, T0_US, 1_000_000, 64)
    assert got.outside == 0


# 3
@pytest.mark.parametrize("geom", [(None, None), ("2", None)])
def test_trainticket_width(ctx, monkeypatch, geom):
    """E = 2208: the LDS tile holds one window."""
    _geometry(monkeypatch, geom)
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=11, p_orphan_ppm=5000), 1500)
    assert edge_rows(sp.n_services) == 2208
    sp.start_us = formula_starts(sp, T0_US, 32 * 2_000_000, 120)
    got = _check(ctx, sp, T0_US, 2_000_000, 32)
    assert int(got.count.sum()) + got.outside == sp.n_spans


@pytest.mark.parametrize("S", [30, 39])
def test_ring_of_two_or_three_windows(ctx, monkeypatch, S):
    """E = 960 / 1599: a ring of 3 / 2 tile windows that wraps as one
    workgroup walks 50 windows."""
    from test_gpu_edge import _random_spanset

    _geometry(monkeypatch, ("1", None))
    sp = _random_spanset(np.random.default_rng(S), S, 1500, 14)
    sp.start_us = formula_starts(sp, T0_US, 50 * 1000, 3)
    _check(ctx, sp, T0_US, 1000, 50)
    _check(ctx, sp, T0_US, 10_000, 6)   # a window per batch: the ring rotates and wraps


# 4
@pytest.mark.parametrize("unique", [True, False])
def test_long_traces(ctx, unique):
    """Traces of 16..4000 spans: the big-trace key pass."""
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=5, p_orphan_ppm=10000), 300)
    lens = np.diff(sp.trace_ptr)
    assert lens.max() > 2000 and lens.min() >= 16
    sp.unique_ids = unique
    sp.start_us = formula_starts(sp, T0_US, 16 * 3_000_000, 40)
    _check(ctx, sp, T0_US, 3_000_000, 16)


def _singles(starts, dur=None, flags=None, S=2):
    """One single-span root trace per start time (edge ROOT -> svc)."""
    n = len(starts)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    return anomod.SpanSet([f"s{i}" for i in range(S)], np.arange(n + 1, dtype=np.uint64), ids, ids,
                          np.zeros(n, np.uint64), (np.arange(n) % S).astype(np.uint16),
                          np.zeros(n, np.uint16) if flags is None else flags,
                          np.arange(1, n + 1, dtype=np.uint32) if dur is None else dur,
                          unique_ids=True, start_us=np.asarray(starts, np.uint64))


# 5
@pytest.mark.parametrize("t0,step,n_windows", [
    (10**6, 1, 5), (10**6, 2**40, 5), (10**6, 7, 1), (10**6, 2**40, 1),
    (2**64 - 2**41, 2**40, 4),       # t0 + T * step passes 2^64
    (0, 2**48, 65536), (2**64 - 1, 1, 3), (1, 2**64 - 1, 2),
])
def test_boundaries(ctx, t0, step, n_windows):
    end = t0 + n_windows * step
    starts = sorted({s for s in (0, t0 - 1, t0, t0 + step - 1, t0 + step, end - 1, end, 2**64 - 1)
                     if 0 <= s < 2**64})
    sp = _singles(starts)
    got = _check(ctx, sp, t0, step, n_windows)
    inside = [s for s in starts if s >= t0 and (s - t0) // step < n_windows]
    assert got.outside == len(starts) - len(inside)
    assert int(got.count.sum()) == len(inside) > 0
    np.testing.assert_array_equal(windows_of(inside, t0, step, n_windows),
                                  [(s - t0) // step for s in inside])


def test_spans_outside_every_trace_are_not_counted(ctx):
    """trace_ptr may cover only [trace_ptr[0], trace_ptr[-1]) of the columns."""
    sp = _singles([T0_US + 3 * k for k in range(4101)])
    cut = anomod.SpanSet(sp.services, np.array([3, 4, 4, 2050, 4098], np.uint64), sp.trace_hash,
                         sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us,
                         unique_ids=True, start_us=sp.start_us)
    got = _check(ctx, cut, T0_US, 2000, 10)
    assert got.outside == 0 and int(got.count.sum()) == 4095
    np.testing.assert_array_equal(got.count.sum(axis=0),
                                  ctx.edge_aggregate(cut, with_hist=False).count)


# 6
def test_one_hot_cell(ctx):
    n = 5000
    sp = _singles([T0_US + 3] * n, dur=np.full(n, 2**32 - 1, np.uint32),
                  flags=np.ones(n, np.uint16), S=1)
    got = _check(ctx, sp, T0_US, 10, 1)
    cell = (0, 1)  # ROOT -> s0
    assert int(got.count[cell]) == n and int(got.errors[cell]) == n
    assert int(got.sum_us[cell]) == n * (2**32 - 1)
    assert int(got.max_us[cell]) == 2**32 - 1
    assert int(got.count.sum()) == n


# 7
def test_scratch_reuse_leaves_no_stale_cells(ctx, sn_set):
    small = sn_set.select_traces(np.arange(sn_set.n_traces) % 7 == 0)
    _check(ctx, sn_set, T0_US, 1_000_000, 64)
    _check(ctx, small, T0_US + 20_000_000, 3_000_000, 8)
    _check(ctx, sn_set, T0_US, 1_000_000, 64)


# 8
@pytest.mark.parametrize("only", ["count", "max_us"])
def test_null_output_pointers_are_skipped(ctx, sn_set, only):
    got = ctx.edge_windows(sn_set, T0_US, 1_000_000, 64, outputs=(only,))
    ref = edge_windows_ref(sn_set, T0_US, 1_000_000, 64)
    np.testing.assert_array_equal(getattr(got, only), getattr(ref, only))
    assert got.outside == ref.outside
    for k in FIELDS:
        if k != only:
            assert not getattr(got, k).any()  # never written


# 9
def test_shards_sum_to_the_whole(ctx, sn_set):
    whole = ctx.edge_windows(sn_set, T0_US, 1_000_000, 64)
    parts = [ctx.edge_windows(sn_set.shard(4, r), T0_US, 1_000_000, 64) for r in range(4)]
    for k in ("count", "errors", "sum_us"):
        np.testing.assert_array_equal(sum(getattr(p, k) for p in parts), getattr(whole, k))
    np.testing.assert_array_equal(np.maximum.reduce([p.max_us for p in parts]), whole.max_us)
    assert sum(p.outside for p in parts) == whole.outside


# 10
def _raw_call(ctx, dev, S, n_windows, t0, step):
    cs = L.EdgeWindowsC(S, n_windows, t0, step, None, None, None, None, 0)
    return L.lib().anomod_edge_windows_spans(ctx.handle, dev.handle, C.byref(cs))


def test_errors_and_empty_input(ctx, sn_set):
    S = sn_set.n_services
    bare = sn_set.select_traces(np.arange(sn_set.n_traces) < 50)
    bare.start_us = None
    dev = ctx.upload(bare)
    assert not dev.has_start_us
    assert _raw_call(ctx, dev, S, 8, 0, 1000) == L.ESTATE
    with pytest.raises(anomod.AnomodError) as e:
        dev.start_us()
    assert e.value.status == L.ESTATE
    with pytest.raises(anomod.AnomodError) as e:
        ctx.edge_windows(dev, 0, 1000, 8)
    assert e.value.status == L.ESTATE
    with pytest.raises(ValueError):
        ctx.edge_windows(bare, 0, 1000, 8)
    dev.set_start_us(np.zeros(dev.n_spans, np.uint64))
    assert _raw_call(ctx, dev, S, 8, 0, 1000) == L.OK
    for n_windows, step in ((0, 1000), (65537, 1000), (8, 0)):
        assert _raw_call(ctx, dev, S, n_windows, 0, step) == L.EINVAL, (n_windows, step)
    assert _raw_call(ctx, dev, S, 65536, 0, 1000) == L.OK
    # T * E <= 2^24: at TrainTicket width (E = 2208) that is T <= 7598
    assert _raw_call(ctx, dev, 46, (1 << 24) // 2208, 0, 1000) == L.OK
    assert _raw_call(ctx, dev, 46, (1 << 24) // 2208 + 1, 0, 1000) == L.EINVAL
    with pytest.raises(anomod.AnomodError) as e:
        ctx.edge_windows(dev, 0, 1000, 65537)
    assert e.value.status == L.EINVAL
    # an ungrouped set: the grouped-set error of the exact quantiles
    ung = ctx.upload_ungrouped(bare)
    ung.set_start_us(np.zeros(ung.n_spans, np.uint64))
    assert _raw_call(ctx, ung, S, 8, 0, 1000) == L.EINVAL
    assert b"not grouped" in L.lib().anomod_last_error(ctx.handle)
    with pytest.raises(anomod.AnomodError):
        ung.fill_start_synthetic(0, 1000, 1)
    with pytest.raises(anomod.AnomodError) as e:  # n_traces * period_us must stay below 2^63
        dev.fill_start_synthetic(0, 2**63 // dev.n_traces + 1, 1)
    assert e.value.status == L.EINVAL
    dev.free()
    ung.free()
    # an empty set: zeros
    empty = bare.select_traces(np.zeros(bare.n_traces, bool))
    empty.start_us = np.zeros(0, np.uint64)
    got = ctx.edge_windows(empty, 5, 1000, 8)
    assert got.outside == 0 and not any(getattr(got, k).any() for k in FIELDS)
    assert got.count.shape == (8, edge_rows(S))


# 11
def test_start_column_plumbing(ctx, sn_set):
    dev = ctx.generate(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)
    assert not dev.has_start_us  # generated sets carry none
    dev.fill_start_synthetic(T0_US, 64 * 1_000_000, 50)
    assert dev.has_start_us
    np.testing.assert_array_equal(dev.start_us(), sn_set.start_us)  # the numpy formula
    host = dev.download()
    np.testing.assert_array_equal(host.start_us, sn_set.start_us)
    assert_windows_equal(ctx.edge_windows(dev, T0_US, 1_000_000, 64),
                         edge_windows_ref(sn_set, T0_US, 1_000_000, 64))
    # a period that does not divide evenly, a gap of 0, traces with no spans
    from test_gpu_edge import _random_spanset

    odd = _random_spanset(np.random.default_rng(4), 5, 777, 9)
    d2 = ctx.upload(odd)
    d2.fill_start_synthetic(12345, 999_983, 0)
    np.testing.assert_array_equal(d2.start_us(), formula_starts(odd, 12345, 999_983, 0))
    d2.free()
    # set / get round trip, through upload as well
    rng = np.random.default_rng(1)
    vals = rng.integers(0, 2**64, dev.n_spans, dtype=np.uint64)
    dev.set_start_us(vals)
    np.testing.assert_array_equal(dev.start_us(), vals)
    with pytest.raises(ValueError):
        dev.set_start_us(vals[:-1])
    up = ctx.upload(sn_set)
    assert up.has_start_us
    np.testing.assert_array_equal(up.start_us(), sn_set.start_us)
    # regrouped / shuffled copies carry no start column
    sh = ctx.shuffle(up, 3)
    assert sh.grouped and not sh.has_start_us
    mixed = ctx.shuffle(up, 3, window_traces=16)
    assert not mixed.grouped and not mixed.has_start_us
    grouped = ctx.group(mixed)
    assert grouped.grouped and not grouped.has_start_us
    for d in (dev, up, sh, mixed, grouped):
        d.free()


# 12
def test_product_path_on_the_golden(ctx, golden, tmp_path):
    exp_name = "Svc_Kill_Media_20251103_230000"
    d = tmp_path / "trace_data" / f"{exp_name}_traces_2025-11-03_23-10-00"
    d.mkdir(parents=True)
    shutil.copy(golden / "jaeger_small.json", d / "all_traces.json")
    exp = anomod.load_experiment(d, name=exp_name)
    sp = exp.spans
    assert sp.start_us is not None and sp.start_us.min() > 0
    W = 6
    f = anomod.features(exp, ctx, trace_step_s=60)
    step = 60_000_000
    t0 = int(sp.start_us.min()) // step * step
    n_windows = (int(sp.start_us.max()) - t0) // step + 1
    win = f.edge_windows
    assert (win.t0_us, win.step_us, win.n_windows) == (t0, step, n_windows)
    assert_windows_equal(win, edge_windows_ref(sp, t0, step, n_windows))
    assert win.outside == 0 and int(win.count.sum()) == sp.n_spans
    mm = win.matrix(5).pad_to_multiple(W)
    Zr = native.ewma_z(mm.X, 2.0 / (W + 1), W, eps=1e-2)
    want = anomod.trace_window_scores(Zr, win, sp.n_services)
    print("golden trace scores:", np.round(f.trace_window_scores, 4), "oracle:", np.round(want, 4))
    np.testing.assert_allclose(f.trace_window_scores, want, rtol=1e-5, atol=1e-6)
    comp = f.params["components"]
    np.testing.assert_array_equal(comp["trace"], f.trace_window_scores / (1 + f.trace_window_scores))
    # no step: nothing changes — no trace term, the parent's formula
    f0 = anomod.features(exp, ctx)
    assert "trace" not in f0.params["components"] and f0.edge_windows is None
    assert f0.trace_window_scores is None
    assert set(f0.params) == {"W", "alpha", "eps", "components"}
    for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
        np.testing.assert_array_equal(getattr(f0.edges, k), getattr(f.edges, k))
    c0 = f0.params["components"]
    np.testing.assert_array_equal(f0.service_scores,
                                  c0["error_rate"] + c0["latency"] + 0.25 * c0["metric"])
    np.testing.assert_array_equal(f.service_scores, f0.service_scores + 0.25 * comp["trace"])
    # a step for a set without start times is an error
    sp.start_us = None
    with pytest.raises(ValueError):
        anomod.features(exp, ctx, trace_step_s=60)


# 13
def test_fault_case_on_the_gpu(ctx):
    sp = fault_set()
    exp = anomod.Experiment("synthetic_fault", sp, None, FAULT, {})
    f = anomod.features(exp, ctx, trace_step_s=STEP / 1e6, trace_W=6)
    win = f.edge_windows
    assert (win.t0_us, win.step_us, win.n_windows) == (T0, STEP, T)
    assert_windows_equal(win, edge_windows_ref(sp, T0, STEP, T))
    ts = f.params["components"]["trace"]
    print("trace component:", dict(zip(sp.services, np.round(ts, 3))))
    assert sp.services[int(np.argmax(ts))] == FAULT
    assert FAULT in [s for s, _ in anomod.rank(f, ctx=ctx)[:3]]

"""GPU: the edge load table (csrc/edge_load.hip) against the reference helper
(tests/edge_load_ref.py), bit for bit — no tolerance anywhere on the tables —
in both forms of the stream kernel (parent rows of a resident set; edge keys
from the aggregation's walk), plus the plumbing and the load term of
features().

ANOMOD_EDGE_LOAD_WGS / ANOMOD_EDGE_LOAD_TILE cap the stream kernel's workgroups
and LDS tile windows: the small sets here would otherwise give every workgroup
a single batch (no tile movement) — results must not depend on them."""
import ctypes as C
import json
import shutil

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import edge_rows
from oracle import native

from edge_load_ref import FIELDS, assert_load_equal, edge_load_brute, edge_load_ref
from edge_windows_ref import formula_starts
from test_edge_load_host import BOUNDARY, EPS, W, singles

pytestmark = pytest.mark.gpu

T0_US = 1_762_000_000_000_000
# (workgroup cap, tile-window cap): default geometry, one workgroup walking the
# whole set, three workgroups with a 2-window ring, every partial to global atomics
GEOMETRIES = [(None, None), ("1", None), ("3", "2"), (None, "0")]
U64 = 2**64


def _geometry(monkeypatch, geom):
    for name, v in zip(("ANOMOD_EDGE_LOAD_WGS", "ANOMOD_EDGE_LOAD_TILE"), geom):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def get_rows(ctx, dev):
    """(status, column) of anomod_spans_parent_rows."""
    out = np.zeros(dev.n_spans, np.uint16)
    rc = L.lib().anomod_spans_parent_rows(ctx.handle, dev.handle, L.ptr(out, C.c_uint16),
                                          len(dev.services))
    return rc, out


def resident(ctx, sp):
    """The set on the device with its parent rows in place (one aggregation)."""
    dev = ctx.upload(sp)
    ctx.edge_aggregate(dev, with_hist=False)
    rc, _ = get_rows(ctx, dev)
    assert rc == L.OK
    return dev


def both_forms(ctx, sp, t0, step, n_windows, ref=None, capfd=None, monkeypatch=None):
    """The call in the rows form (a resident set after one aggregation) and in
    the keys form (the host set, uploaded for the call): both equal the
    reference.  Returns the rows-form result."""
    ref = edge_load_ref(sp, t0, step, n_windows) if ref is None else ref
    if monkeypatch is not None:
        monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    dev = resident(ctx, sp)
    if capfd is not None:
        capfd.readouterr()
    got = ctx.edge_load(dev, t0, step, n_windows)
    if capfd is not None:
        assert "edge_load_kernel<rows>" in capfd.readouterr().err
    dev.free()
    assert_load_equal(got, ref)
    keys = ctx.edge_load(sp, t0, step, n_windows)
    if capfd is not None:
        assert "edge_load_kernel<keys>" in capfd.readouterr().err
    assert_load_equal(keys, ref)
    return got


@pytest.fixture(scope="module")
def sn_set():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)
    sp.start_us = formula_starts(sp, T0_US, 64 * 1_000_000, 50)
    return sp


@pytest.fixture(scope="module")
def sn_refs(sn_set):
    """The references of case 1, computed once: the range that covers every
    span and one that leaves spans outside on both sides and opens in the
    middle of the longest span of the first seconds; (whole, clipped, its t0)."""
    early = np.nonzero(sn_set.start_us < T0_US + 8_000_000)[0]
    i = int(early[np.argmax(sn_set.dur_us[early])])
    t0c = int(sn_set.start_us[i]) + int(sn_set.dur_us[i]) // 2
    return (edge_load_ref(sn_set, T0_US, 1_000_000, 64),
            edge_load_ref(sn_set, t0c, 700_000, 40), t0c)


# 1
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_sn_time_ordered(ctx, sn_set, sn_refs, monkeypatch, capfd, geom):
    _geometry(monkeypatch, geom)
    whole, clipped, t0c = sn_refs
    got = both_forms(ctx, sn_set, T0_US, 1_000_000, 64, whole, capfd, monkeypatch)
    assert got.outside == 0
    table = ctx.edge_aggregate(sn_set, with_hist=False)
    np.testing.assert_array_equal(got.busy_us.sum(axis=0), table.sum_us)
    # the device set with the row stream switched off: the keys form
    dev = resident(ctx, sn_set)
    monkeypatch.setenv("ANOMOD_PARENT_ROWS", "0")
    capfd.readouterr()
    off = ctx.edge_load(dev, T0_US, 1_000_000, 64)
    assert "edge_load_kernel<keys>" in capfd.readouterr().err
    assert_load_equal(off, whole)
    assert_load_equal(ctx.edge_load(dev, t0c, 700_000, 40), clipped)
    monkeypatch.delenv("ANOMOD_PARENT_ROWS")
    dev.free()
    # a window range that clips spans on both sides
    got = both_forms(ctx, sn_set, t0c, 700_000, 40, clipped)
    assert 0 < got.outside < sn_set.n_spans
    assert got.carried[0].sum() > 0  # open at t0: clipped, not dropped


# 2
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_spans_over_many_windows(ctx, sn_set, monkeypatch, geom):
    """step 100 us, T = 4096, durations x 4: most spans cover tens of windows,
    so the sums come from the difference tables and the scan (16 segments);
    the wrapped negatives of several workgroups must cancel."""
    _geometry(monkeypatch, geom)
    sp = sn_set.select_traces(np.ones(sn_set.n_traces, bool))
    sp.dur_us = sn_set.dur_us * np.uint32(4)
    sp.start_us = formula_starts(sp, T0_US, 380_000, 3)
    assert np.median(sp.dur_us) > 20 * 100
    got = both_forms(ctx, sp, T0_US, 100, 4096)
    assert int(got.carried.sum()) > 10 * sp.n_spans
    assert int(got.busy_us.max()) < 2**40 and int(got.carried.max()) < 2**32  # nothing left wrapped


# 3
@pytest.mark.parametrize("case", range(len(BOUNDARY)))
def test_boundary_singles(ctx, case):
    t0, step, n_windows, spans = BOUNDARY[case]
    for sub in [[s] for s in spans]:
        sp = singles(sub)
        ref = edge_load_ref(sp, t0, step, n_windows)
        assert_load_equal(ctx.edge_load(sp, t0, step, n_windows), ref)
    sp = singles(spans)
    ref = edge_load_brute(sp, t0, step, n_windows)
    both_forms(ctx, sp, t0, step, n_windows, ref)


# 4
def _random_singles(rng, n, t0, span_us, max_dur, S=2):
    starts = rng.integers(t0 - span_us // 8, t0 + span_us + span_us // 8, n)
    durs = np.where(rng.random(n) < 0.1, 0, rng.integers(0, max_dur, n))
    return singles(list(zip(starts.tolist(), durs.tolist())), S=S)


def test_scan_segment_borders(ctx):
    seg = int(L.lib().anomod_edge_load_scan_segment())  # kLoadSeg of csrc/edge_load.hip
    assert seg >= 2
    rng = np.random.default_rng(5)
    for n_windows in sorted({1, 2, seg - 1, seg, seg + 1, 2 * seg + 1}):
        sp = _random_singles(rng, 300, T0_US, n_windows * 10, 6 * n_windows * 10)
        both_forms(ctx, sp, T0_US, 10, n_windows)


@pytest.mark.parametrize("S", [1, 15])
def test_scan_of_65536_windows(ctx, S):
    """T = 65536 at S = 1 (three rows: the scan must not walk T with three
    threads) and at S = 15 (T * E = 2^24 - 65536), with one span of 2^32 - 1 us
    at a step of 65,536 us that covers every window."""
    n_windows, step = 65536, 65536
    assert n_windows * edge_rows(S) <= 1 << 24 and (S == 1 or n_windows * edge_rows(S) == 2**24 - 65536)
    rng = np.random.default_rng(S)
    sp = _random_singles(rng, 400, T0_US, n_windows * step, 2**32, S=S)
    sp.start_us[0], sp.dur_us[0] = T0_US, 2**32 - 1
    ref = edge_load_ref(sp, T0_US, step, n_windows)
    assert int((ref.busy_us.sum(axis=1) > 0).sum()) == n_windows
    both_forms(ctx, sp, T0_US, step, n_windows, ref)


# 5
def test_one_hot_cell(ctx):
    n = 1 << 16
    sp = singles([(T0_US + 3, 7)] * n, S=1)
    got = both_forms(ctx, sp, T0_US, 10, 1)
    assert int(got.busy_us[0, 1]) == 7 * n and int(got.busy_us.sum()) == 7 * n  # ROOT -> s0
    assert not got.carried.any()
    n = 5000
    sp = singles([(T0_US + 3, 2**32 - 1)] * n, S=1)
    got = both_forms(ctx, sp, T0_US, 2**29, 8)
    assert int(got.busy_us[0, 1]) == n * (2**29 - 3) and int(got.busy_us[3, 1]) == n * 2**29
    assert int(got.busy_us[:, 1].sum()) == n * (2**32 - 3)  # the range ends 2 us before the spans
    assert got.carried[:, 1].tolist() == [0] + [n] * 7 and got.outside == 0


# 6
@pytest.mark.parametrize("unique", [True, False])
def test_long_traces(ctx, unique, monkeypatch, capfd):
    """Traces of 16..4000 spans: the keys form goes through the long-trace key pass."""
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=5, p_orphan_ppm=10000), 300)
    lens = np.diff(sp.trace_ptr)
    assert lens.max() > 256 and lens.min() >= 16
    sp.unique_ids = unique
    sp.start_us = formula_starts(sp, T0_US, 16 * 30_000, 40)
    both_forms(ctx, sp, T0_US, 30_000, 16, None, capfd, monkeypatch)


# 7
@pytest.mark.parametrize("geom", [(None, None), ("2", "1")])
def test_trainticket_width(ctx, monkeypatch, geom):
    """E = 2208: a tile of two windows, or of one."""
    _geometry(monkeypatch, geom)
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=11, p_orphan_ppm=5000), 1500)
    assert edge_rows(sp.n_services) == 2208
    sp.start_us = formula_starts(sp, T0_US, 32 * 20_000, 120)
    both_forms(ctx, sp, T0_US, 20_000, 32)


def test_table_too_wide_for_a_tile(ctx, monkeypatch, capfd):
    """S = 90, E = 8280: one window slot of u64 cells outgrows the LDS budget
    (Wt = 0 by itself): every partial goes to global atomics."""
    from test_gpu_edge import _random_spanset

    sp = _random_spanset(np.random.default_rng(90), 90, 600, 14)
    sp.start_us = formula_starts(sp, T0_US, 50 * 1000, 3)
    sp.dur_us = sp.dur_us % np.uint32(5000)
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    both_forms(ctx, sp, T0_US, 1000, 50)
    assert "tile 0 windows" in capfd.readouterr().err


# 8
@pytest.mark.parametrize("only", FIELDS)
def test_null_output_pointers_are_skipped(ctx, sn_set, sn_refs, only):
    t0c = sn_refs[2]
    dev = resident(ctx, sn_set)
    for src in (dev, sn_set):
        got = ctx.edge_load(src, t0c, 700_000, 40, outputs=(only,))
        np.testing.assert_array_equal(getattr(got, only), getattr(sn_refs[1], only))
        assert got.outside == sn_refs[1].outside
        for k in FIELDS:
            if k != only:
                assert not getattr(got, k).any()  # never written
    dev.free()


def test_scratch_reuse_leaves_no_stale_cells(ctx, sn_set, sn_refs):
    t0c = sn_refs[2]
    small = sn_set.select_traces(np.arange(sn_set.n_traces) % 7 == 0)
    dev = resident(ctx, sn_set)
    assert_load_equal(ctx.edge_load(dev, T0_US, 1_000_000, 64), sn_refs[0])
    assert_load_equal(ctx.edge_load(small, T0_US + 20_000_000, 3_000_000, 8),
                      edge_load_ref(small, T0_US + 20_000_000, 3_000_000, 8))
    assert_load_equal(ctx.edge_load(dev, T0_US, 1_000_000, 64), sn_refs[0])
    # the windowed table shares the slot
    ctx.edge_windows(sn_set, T0_US, 1_000_000, 64)
    assert_load_equal(ctx.edge_load(dev, t0c, 700_000, 40), sn_refs[1])
    dev.free()


def test_shards_sum_to_the_whole(ctx, sn_set, sn_refs):
    t0c = sn_refs[2]
    parts = [ctx.edge_load(sn_set.shard(2, r), t0c, 700_000, 40) for r in range(2)]
    for k in FIELDS:
        np.testing.assert_array_equal(sum(getattr(p, k) for p in parts), getattr(sn_refs[1], k))
    assert sum(p.outside for p in parts) == sn_refs[1].outside


def test_spans_outside_every_trace_are_not_counted(ctx):
    """trace_ptr may cover only [trace_ptr[0], trace_ptr[-1]) of the columns."""
    sp = singles([(T0_US + 3 * k, 1 + k % 5000) for k in range(4101)])
    cut = anomod.SpanSet(sp.services, np.array([3, 4, 4, 2050, 4098], np.uint64), sp.trace_hash,
                         sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us,
                         unique_ids=True, start_us=sp.start_us)
    ref = edge_load_ref(cut, T0_US, 2000, 10)
    got = both_forms(ctx, cut, T0_US, 2000, 10, ref)
    assert got.outside == 0
    assert int(got.busy_us.sum()) == int(cut.dur_us[3:4098].astype(np.uint64).sum())


def _raw_call(ctx, dev, S, n_windows, t0, step):
    cs = L.EdgeLoadC(S, n_windows, t0, step, None, None, 0)
    return L.lib().anomod_edge_load_spans(ctx.handle, dev.handle, C.byref(cs))


def test_errors_and_empty_input(ctx, sn_set):
    S = sn_set.n_services
    bare = sn_set.select_traces(np.arange(sn_set.n_traces) < 50)
    bare.start_us = None
    dev = ctx.upload(bare)
    assert _raw_call(ctx, dev, S, 8, 0, 1000) == L.ESTATE
    with pytest.raises(anomod.AnomodError) as e:
        ctx.edge_load(dev, 0, 1000, 8)
    assert e.value.status == L.ESTATE
    with pytest.raises(ValueError):
        ctx.edge_load(bare, 0, 1000, 8)
    dev.set_start_us(np.zeros(dev.n_spans, np.uint64))
    assert _raw_call(ctx, dev, S, 8, 0, 1000) == L.OK
    for n_windows, step in ((0, 1000), (65537, 1000), (8, 0)):
        assert _raw_call(ctx, dev, S, n_windows, 0, step) == L.EINVAL, (n_windows, step)
    assert _raw_call(ctx, dev, S, 65536, 0, 1000) == L.OK
    # T * E <= 2^24: at TrainTicket width (E = 2208) that is T <= 7598
    assert _raw_call(ctx, dev, 46, (1 << 24) // 2208, 0, 1000) == L.OK
    assert _raw_call(ctx, dev, 46, (1 << 24) // 2208 + 1, 0, 1000) == L.EINVAL
    # a service index >= S
    assert _raw_call(ctx, dev, int(bare.svc.max()), 8, 0, 1000) == L.EINVAL
    assert b"service index" in L.lib().anomod_last_error(ctx.handle)
    with pytest.raises(anomod.AnomodError) as e:
        ctx.edge_load(dev, 0, 1000, 65537)
    assert e.value.status == L.EINVAL
    ung = ctx.upload_ungrouped(bare)
    ung.set_start_us(np.zeros(ung.n_spans, np.uint64))
    assert _raw_call(ctx, ung, S, 8, 0, 1000) == L.EINVAL
    assert b"not grouped" in L.lib().anomod_last_error(ctx.handle)
    dev.free()
    ung.free()
    # an empty set: zeros
    empty = bare.select_traces(np.zeros(bare.n_traces, bool))
    empty.start_us = np.zeros(0, np.uint64)
    got = ctx.edge_load(empty, 5, 1000, 8)
    assert got.outside == 0 and not any(getattr(got, k).any() for k in FIELDS)
    assert got.busy_us.shape == (8, edge_rows(S))


def test_rows_and_hints_are_left_alone(ctx, sn_set, sn_refs, monkeypatch):
    """The call neither creates nor changes the row column and the hints."""
    t0c = sn_refs[2]
    # a resident set that was never aggregated: the keys form, and still no rows
    dev = ctx.upload(sn_set)
    assert get_rows(ctx, dev)[0] != L.OK
    assert_load_equal(ctx.edge_load(dev, T0_US, 1_000_000, 64), sn_refs[0])
    assert get_rows(ctx, dev)[0] != L.OK
    # aggregated: rows and hints unchanged by either form
    ctx.edge_aggregate(dev, with_hist=False)
    rc, rows = get_rows(ctx, dev)
    assert rc == L.OK
    hints = dev.hints
    assert_load_equal(ctx.edge_load(dev, t0c, 700_000, 40), sn_refs[1])
    monkeypatch.setenv("ANOMOD_PARENT_ROWS", "0")
    assert_load_equal(ctx.edge_load(dev, t0c, 700_000, 40), sn_refs[1])
    monkeypatch.delenv("ANOMOD_PARENT_ROWS")
    rc, after = get_rows(ctx, dev)
    assert rc == L.OK
    np.testing.assert_array_equal(after, rows)
    assert dev.hints == hints
    # rows written at one service count, read at another
    wide = anomod.SpanSet(sn_set.services + ["extra"], sn_set.trace_ptr, sn_set.trace_hash,
                          sn_set.span_id, sn_set.parent_span_id, sn_set.svc, sn_set.flags,
                          sn_set.dur_us, unique_ids=sn_set.unique_ids, start_us=sn_set.start_us)
    cs_ref = edge_load_ref(wide, T0_US, 1_000_000, 64)
    S1 = len(wide.services)
    busy = np.zeros((64, edge_rows(S1)), np.uint64)
    cs = L.EdgeLoadC(S1, 64, T0_US, 1_000_000, L.ptr(busy, C.c_uint64), None, 0)
    assert L.lib().anomod_edge_load_spans(ctx.handle, dev.handle, C.byref(cs)) == L.OK
    np.testing.assert_array_equal(busy, cs_ref.busy_us)
    dev.free()


def test_stage_timers(ctx, sn_set):
    dev = resident(ctx, sn_set)
    ctx.edge_load(dev, T0_US, 1_000_000, 64)
    whole, kern, scan = (ctx.stage_ms(s) for s in (L.STAGE_EDGE_LOAD, L.STAGE_EDGE_LOAD_KERNEL,
                                                  L.STAGE_EDGE_LOAD_SCAN))
    assert 0 < kern <= whole and 0 < scan <= whole
    dev.free()


# 9
def _golden_experiment(golden, tmp_path):
    exp_name = "Svc_Kill_Media_20251103_230000"
    d = tmp_path / "trace_data" / f"{exp_name}_traces_2025-11-03_23-10-00"
    d.mkdir(parents=True)
    shutil.copy(golden / "jaeger_small.json", d / "all_traces.json")
    return anomod.load_experiment(d, name=exp_name), d


def test_product_path_on_the_golden(ctx, golden, tmp_path):
    exp, _ = _golden_experiment(golden, tmp_path)
    sp = exp.spans
    f = anomod.features(exp, ctx, trace_step_s=60, trace_load=True)
    step = 60_000_000
    t0 = int(sp.start_us.min()) // step * step
    n_windows = (int(sp.start_us.max()) - t0) // step + 1
    load = f.edge_load
    assert (load.t0_us, load.step_us, load.n_windows) == (t0, step, n_windows)
    assert (f.edge_windows.t0_us, f.edge_windows.step_us, f.edge_windows.n_windows) == (t0, step, n_windows)
    assert_load_equal(load, edge_load_brute(sp, t0, step, n_windows))
    comp = f.params["components"]
    mm = load.matrix().pad_to_multiple(W)
    Zr = native.ewma_z(mm.X, 2.0 / (W + 1), W, eps=EPS)
    ls = anomod.load_window_scores(Zr, load, sp.n_services)
    print("golden load scores:", np.round(comp["load"], 4), "oracle:", np.round(ls / (1 + ls), 4))
    np.testing.assert_allclose(comp["load"], ls / (1 + ls), rtol=1e-5, atol=1e-6)
    # without the flag: bit-identical to the call that never knew it
    f0 = anomod.features(exp, ctx, trace_step_s=60)
    assert f0.edge_load is None and "load" not in f0.params["components"]
    assert "trace_load" not in f0.params
    c0 = f0.params["components"]
    np.testing.assert_array_equal(
        f0.service_scores, c0["error_rate"] + c0["latency"] + 0.25 * c0["metric"] + 0.25 * c0["trace"])
    np.testing.assert_array_equal(f.service_scores, f0.service_scores + 0.25 * comp["load"])
    np.testing.assert_array_equal(f.trace_window_scores, f0.trace_window_scores)
    with pytest.raises(ValueError):
        anomod.features(exp, ctx, trace_load=True)


def test_cli_prints_the_table(ctx, golden, tmp_path):
    from anomod.__main__ import main

    exp, d = _golden_experiment(golden, tmp_path)
    out = tmp_path / "features.json"
    assert main(["features", str(d), "--trace-step", "60", "--trace-load", "--out", str(out)]) == 0
    doc = json.loads(out.read_text())
    f = anomod.features(exp, ctx, trace_step_s=60, trace_load=True)
    got = doc["edge_load"]
    assert (got["t0_us"], got["step_us"], got["windows"]) == (
        f.edge_load.t0_us, f.edge_load.step_us, f.edge_load.n_windows)
    active = f.edge_load.active_rows()
    assert len(got["edges"]) == active.shape[0] > 0
    for row, r in zip(got["edges"], active.tolist()):
        assert row["busy_us"] == f.edge_load.busy_us[:, r].tolist()
        assert row["carried"] == f.edge_load.carried[:, r].tolist()
        assert row["child"] == exp.spans.services[r % exp.spans.n_services]
    assert set(doc["load_scores"]) == set(exp.spans.services)
    with pytest.raises(SystemExit):
        main(["features", str(d), "--trace-load"])

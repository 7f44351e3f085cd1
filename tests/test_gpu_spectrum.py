"""GPU: the trace spectrum (csrc/spectrum.hip) against the reference helper
(tests/spectrum_ref.py), bit for bit — class totals, per-class service and
edge coverage, bad spans per row, the class of every trace — on generated and
hand-made shapes, plus argument handling and the ranking term of features()."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment

from self_time_ref import add_delay
from spectrum_ref import (U32_MAX, assert_spectrum_equal, make_set, oracle_table, rows_ref,
                          service_ochiai_ref, spectrum_ref)
from test_spectrum_host import DELAY_US, FAULTS, synth

pytestmark = pytest.mark.gpu


def _check(ctx, sp, thr=None, use_errors=True, dev=None, rows=None):
    """Spectrum of `sp` (or of its device twin `dev`) == reference."""
    ref = spectrum_ref(sp, thr, use_errors, rows)
    got = ctx.trace_spectrum(sp if dev is None else dev, thr, use_errors)
    assert_spectrum_equal(got, ref)
    return got, ref


def _one_service_set(services, durs, flags=None):
    """Single-span root traces of service 0 with the given durations."""
    n = len(durs)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    return anomod.SpanSet(list(services), np.arange(n + 1, dtype=np.uint64), ids.copy(), ids,
                          np.zeros(n, np.uint64), np.zeros(n, np.uint16),
                          np.zeros(n, np.uint16) if flags is None else flags,
                          np.asarray(durs, np.uint32))


# ------------------------------------------------------------------ generated sets
@pytest.fixture(scope="module", params=[("SN", 4096), ("TT", 2048)], ids=["SN", "TT"])
def synth_case(request):
    topo, n = request.param
    sp = synth(topo, n, fault_service=FAULTS[topo])
    thr = anomod.spectrum_thresholds(oracle_table(synth(topo, n)), sp.services, rows="all")
    return topo, sp, thr, rows_ref(sp)


@pytest.mark.parametrize("use_errors", [True, False])
def test_generated_sets_host_and_device(ctx, synth_case, use_errors, monkeypatch, capfd):
    """A faulted set against a fault-free set's p99 thresholds, as a host set
    (uploaded for the call) and as a device set; both widths keep their
    counters in LDS (TrainTicket: E = 2208) and no trace outgrows a chunk."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    topo, sp, thr, rows = synth_case
    got, ref = _check(ctx, sp, thr, use_errors, rows=rows)
    assert "counters in LDS, long pass off" in capfd.readouterr().err
    assert ref["n_traces"].min() > 0 and ref["bad_spans"].sum() > 0
    d = ctx.upload(sp)
    try:
        _check(ctx, sp, thr, use_errors, dev=d, rows=rows)
        again = ctx.trace_spectrum(d, thr, use_errors, per_trace=False)   # NULL class column
        assert again.trace_abnormal is None
        np.testing.assert_array_equal(again.svc_traces, ref["svc_traces"])
        np.testing.assert_array_equal(again.n_traces, ref["n_traces"])
        # the rows are the edge table's
        table = ctx.edge_aggregate(d, with_hist=False)
        assert ((got.edge_traces.sum(axis=0) > 0) == (table.count > 0)).all()
        assert (got.bad_spans <= table.count).all()
    finally:
        d.free()
    np.testing.assert_array_equal(got.ochiai(), service_ochiai_ref(ref))


def test_generated_geometry(ctx, synth_case, monkeypatch):
    """The key walk cut into launches of <= 4096 spans gives the same result."""
    _, sp, thr, rows = synth_case
    monkeypatch.setenv("ANOMOD_MAX_LAUNCH_SPANS", "4096")
    _check(ctx, sp, thr, True, rows=rows)


# ------------------------------------------------------------------ long traces
def _flagged_trace(services, n, first_id, bad_at):
    """One trace of n spans over 3 services, a chain, whose only error flag
    (and only bad span) sits at position bad_at."""
    ids = np.arange(first_id, first_id + n, dtype=np.uint64)
    flags = np.zeros(n, np.uint16)
    flags[bad_at] = 1
    return anomod.SpanSet(list(services), np.array([0, n], np.uint64), ids.copy(), ids,
                          np.r_[np.uint64(0), ids[:-1]], (np.arange(n) % 3).astype(np.uint16),
                          flags, np.zeros(n, np.uint32))


def test_long_topology_and_hand_made_long_traces(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    long_ = anomod.synth_generate_host(
        anomod.SynthSpec("LONG", seed=1, p_orphan_ppm=2000, p_error_ppm=0), 64)
    lens = np.diff(long_.trace_ptr)
    assert (lens > 256).any() and (lens <= 256).any()
    last = _flagged_trace(long_.services, 5000, 1 << 50, 4999)
    first = _flagged_trace(long_.services, 5000, 1 << 51, 0)
    sp = anomod.SpanSet.concat([long_.select_traces(np.arange(64) < 32), last,
                                long_.select_traces(np.arange(64) >= 32), first])
    # the generated traces' own p99: about 1 % of their spans are bad
    thr = anomod.spectrum_thresholds(oracle_table(long_), sp.services, rows="all")
    got, ref = _check(ctx, sp, thr, True)
    assert "long pass on" in capfd.readouterr().err
    assert got.trace_abnormal[32] == 1 and got.trace_abnormal[-1] == 1
    assert ref["n_traces"].min() > 0
    got, _ = _check(ctx, sp, thr, False)     # without error flags the two are normal
    assert got.trace_abnormal[32] == 0 and got.trace_abnormal[-1] == 0
    got, _ = _check(ctx, sp, None, True)     # and the only abnormal traces without thresholds
    assert got.n_traces.tolist() == [64, 2]
    assert got.svc_traces[1].tolist() == [2, 2, 2] + [0] * (sp.n_services - 3)
    assert int(got.bad_spans.sum()) == 2


# ------------------------------------------------------------------ chunk edges
def test_chunk_edges(ctx):
    """Traces of 1 / 255 / 256 / 257 spans, an empty trace, 65 single-span
    traces in a row, and 200 spans on one edge.  Of the 74 traces only the last
    18 (217 spans) are packed, into one chunk; every other trace is a chunk of
    its own, so no chunk closes at 64 traces or 256 spans here — those borders
    are test_gpu_walk_borders.py's."""
    rng = np.random.default_rng(7)
    S = 5
    lens = np.r_[[1, 255, 256, 257, 0], [1] * 65, [200], [0, 3, 0]]
    sp = make_set(S, lens, rng)
    a = int(sp.trace_ptr[sp.n_traces - 4])
    assert int(sp.trace_ptr[sp.n_traces - 3]) - a == 200
    sp.svc[a:a + 200] = 2
    sp.parent_span_id[a:a + 200] = 0          # 200 x ROOT -> service 2
    sp.dur_us[a:a + 200] = 5
    sp.flags[a:a + 200] = 0
    sp.flags[a + 199] = 1
    rows = rows_ref(sp)
    thr = rng.integers(0, 1000, (S + 2) * S).astype(np.uint32)   # about half the spans bad
    thr[S * S + 2] = 700
    for use_errors in (True, False):
        got, ref = _check(ctx, sp, thr, use_errors, rows=rows)
        t200 = sp.n_traces - 4
        assert got.trace_abnormal[t200] == (1 if use_errors else 0)
        assert got.trace_abnormal[4] == 0 and got.trace_abnormal[-1] == 0    # empty traces
    assert ref["n_traces"].min() > 0
    only = sp.select_traces(np.arange(sp.n_traces) == sp.n_traces - 4)
    got, _ = _check(ctx, only, None, True)
    assert int(got.edge_traces.sum()) == 1 and got.edge_traces[1, S * S + 2] == 1
    assert int(got.svc_traces.sum()) == 1 and int(got.bad_spans.sum()) == 1


def test_every_trace_empty(ctx):
    sp = anomod.SpanSet(["a", "b"], np.zeros(6, np.uint64), [], [], [], [], [], [])
    got, _ = _check(ctx, sp)
    assert got.n_traces.tolist() == [5, 0] and got.trace_abnormal.tolist() == [0] * 5


# ------------------------------------------------------------------ threshold edges
def test_threshold_edges(ctx):
    services = ["a", "b"]
    S, row = 2, 2 * 2 + 0                     # ROOT -> a
    sp = _one_service_set(services, [10, 11, U32_MAX, 0])

    def classes(value):
        thr = np.full((S + 2) * S, U32_MAX, np.uint32)
        thr[row] = value
        got, _ = _check(ctx, sp, thr, False)
        return got.trace_abnormal.tolist()

    assert classes(10) == [0, 1, 1, 0]        # dur == thr is not bad, dur == thr + 1 is
    assert classes(U32_MAX) == [0, 0, 0, 0]   # UINT32_MAX never fires, dur == UINT32_MAX included
    assert classes(0) == [1, 1, 1, 0]         # thr = 0 with dur = 0 is not bad
    none, _ = _check(ctx, sp, None, False)
    full = ctx.trace_spectrum(sp, np.full((S + 2) * S, U32_MAX, np.uint32), False)
    for k in ("n_traces", "svc_traces", "edge_traces", "bad_spans", "trace_abnormal"):
        np.testing.assert_array_equal(getattr(none, k), getattr(full, k), err_msg=k)
    # another row's threshold does not apply
    thr = np.zeros((S + 2) * S, np.uint32)
    thr[row] = U32_MAX
    got, _ = _check(ctx, sp, thr, False)
    assert got.n_traces.tolist() == [4, 0]
    flagged = _one_service_set(services, [1, 1, 1], np.array([0, 1, 2], np.uint16))
    got, _ = _check(ctx, flagged, None, True)
    assert got.trace_abnormal.tolist() == [0, 1, 0]   # only the error bit counts
    got, _ = _check(ctx, flagged, None, False)
    assert got.n_traces.tolist() == [3, 0]


# ------------------------------------------------------------------ rows as the edge table's
def test_duplicated_ids_orphans_and_a_self_reference(ctx):
    sp = anomod.synth_generate_host(
        anomod.SynthSpec("SN", seed=9, p_orphan_ppm=50000, fault_service=FAULTS["SN"]), 600)
    sid, pid = sp.span_id.copy(), sp.parent_span_id.copy()
    ptr = sp.trace_ptr.astype(np.int64)
    for t in range(0, 600, 7):                # a later span repeats the trace's second id
        a, b = ptr[t], ptr[t + 1]
        sid[b - 1] = sid[a + 1]
    for t in range(3, 600, 11):               # a span that names itself
        a = ptr[t]
        pid[a + 2] = sid[a + 2]
    dup = anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sid, pid, sp.svc, sp.flags,
                         sp.dur_us, unique_ids=False)
    assert not dup.check_unique_ids()
    rows = rows_ref(dup)
    S = dup.n_services
    assert (rows // S == S + 1).any()         # orphans present
    assert not np.array_equal(rows, rows_ref(sp))
    thr = anomod.spectrum_thresholds(oracle_table(synth("SN", 600)), dup.services, rows="all")
    got, _ = _check(ctx, dup, thr, True, rows=rows)
    table = ctx.edge_aggregate(dup, with_hist=False)
    np.testing.assert_array_equal(np.bincount(rows, minlength=(S + 2) * S), table.count)
    assert ((got.edge_traces.sum(axis=0) > 0) == (table.count > 0)).all()


# ------------------------------------------------------------------ wide tables
@pytest.mark.parametrize("S", [300, 723])
def test_wide_table(ctx, S, monkeypatch, capfd):
    """E = 90 600 (and the widest table the call takes, E = 524 175): counters
    by global atomics, the long-trace bitmap still in LDS."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(S)
    sp = make_set(S, np.r_[rng.integers(1, 40, 30), [300], rng.integers(1, 40, 10)], rng)
    thr = np.full((S + 2) * S, 500, np.uint32)
    got, ref = _check(ctx, sp, thr, True)
    assert "counters in global memory, long pass on" in capfd.readouterr().err
    assert ref["n_traces"].min() > 0
    assert got.svc_traces[:, S - 1].sum() == ref["svc_traces"][:, S - 1].sum()


def test_width_limit(ctx):
    S = 724
    sp = make_set(S, [3, 4], np.random.default_rng(1))
    with pytest.raises(anomod.AnomodError) as e:
        ctx.trace_spectrum(sp)
    assert e.value.status == L.EINVAL and "anomod_trace_spectrum_spans" in str(e.value)


# ------------------------------------------------------------------ status cases
def test_status_cases(ctx):
    empty = anomod.SpanSet(["a", "b"], [0], [], [], [], [], [], [])
    got, _ = _check(ctx, empty)
    assert got.n_traces.tolist() == [0, 0] and got.trace_abnormal.shape == (0,)
    assert not got.svc_traces.any() and not got.edge_traces.any() and not got.bad_spans.any()
    sp = synth("SN", 200)
    lib = anomod.lib()
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))
    d = ctx.upload(sp)
    try:
        with pytest.raises(anomod.AnomodError) as e:
            ctx.trace_spectrum(loose)
        assert e.value.status == L.ESTATE and "not grouped" in str(e.value)
        # a service index >= n_services
        S = sp.n_services
        cs = L.TraceSpectrumC(S - 1, 1, None, (0, 0), None, None, None, None)
        assert lib.anomod_trace_spectrum_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
        assert b"anomod_trace_spectrum_spans" in lib.anomod_last_error(ctx.handle)
        # every output NULL: only the class totals
        cs = L.TraceSpectrumC(S, 1, None, (7, 7), None, None, None, None)
        assert lib.anomod_trace_spectrum_spans(ctx.handle, d.handle, C.byref(cs)) == L.OK
        ref = spectrum_ref(sp)
        assert [cs.n_traces[0], cs.n_traces[1]] == ref["n_traces"].tolist()
        with pytest.raises(ValueError):
            ctx.trace_spectrum(d, np.zeros(3, np.uint32))
    finally:
        d.free()
        loose.free()


def test_hints_and_later_results_unchanged(ctx):
    sp = synth("TT", 500)
    d = ctx.upload(sp)
    try:
        before = ctx.edge_aggregate(d)
        hints = d.hints
        first = ctx.trace_spectrum(d)
        assert d.hints == hints
        after = ctx.edge_aggregate(d)
        again = ctx.trace_spectrum(d)
        for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
            np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
        for k in ("n_traces", "svc_traces", "edge_traces", "bad_spans", "trace_abnormal"):
            np.testing.assert_array_equal(getattr(again, k), getattr(first, k), err_msg=k)
    finally:
        d.free()


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("topo", ["SN", "TT"])
def test_features_spectrum_term(ctx, topo):
    fault = FAULTS[topo]
    base = synth(topo)
    cur = add_delay(base, fault, DELAY_US)
    eb, ec = Experiment("base", base), Experiment("cur", cur, label=fault)
    fb = anomod.features(eb, ctx)
    plain = anomod.features(ec, ctx, baseline=fb)
    fs = anomod.features(ec, ctx, baseline=fb, spectrum=True)
    thr = anomod.spectrum_thresholds(fb.edges, cur.services, rows="root")
    ref = spectrum_ref(cur, thr, True)
    assert_spectrum_equal(fs.spectrum, ref)
    np.testing.assert_array_equal(fs.spectrum.thr_us, thr)
    comp = fs.params["components"]
    assert comp["spectrum_thresholds"] == "baseline"
    och = service_ochiai_ref(ref)
    np.testing.assert_allclose(comp["spectrum"], och, rtol=1e-12, atol=0)
    c = cur.services.index(fault)
    assert int(np.argmax(comp["spectrum"])) == c
    np.testing.assert_array_equal(fs.service_scores, plain.service_scores + 0.25 * comp["spectrum"])
    # without a baseline only error flags label traces
    fe = anomod.features(ec, ctx, spectrum=True)
    assert fe.params["components"]["spectrum_thresholds"] == "errors-only"
    assert fe.spectrum.thr_us is None
    assert_spectrum_equal(fe.spectrum, spectrum_ref(cur, None, True))
    # the default is what it was
    again = anomod.features(ec, ctx, baseline=fb, spectrum=False)
    assert plain.spectrum is None and again.spectrum is None
    np.testing.assert_array_equal(again.service_scores, plain.service_scores)
    assert set(plain.params["components"]) == {"error_rate", "latency", "metric"}
    assert plain.params["components"].keys() == again.params["components"].keys()
    lat = _latency_scores(plain, fb)
    np.testing.assert_array_equal(
        plain.service_scores,
        plain.params["components"]["error_rate"] + lat + 0.25 * plain.params["components"]["metric"])


def _latency_scores(feats, baseline):
    from anomod.engine import _latency_shift
    return _latency_shift(feats.edges, baseline.edges)

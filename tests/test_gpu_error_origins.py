"""GPU: the error origins (csrc/error_origins.hip) against the exact host model
(tests/error_origins_ref.py), bit for bit — the seven tables, the two scalars
and both per-span columns — plus origin + propagated == the edge table's
errors, argument handling, what the call leaves unchanged, and the origin rate
through features() and rank()."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment

from error_origins_ref import (ABSORBER, CLEAN, CONTAINED, LOOP, ORIGIN, PROPAGATED, SURFACED,
                               assert_origins_equal, build, chain_trace, hand_made,
                               inclusive_error_rate, origins_ref, propagate_errors, with_flags)
from test_error_origins_host import propagated
from test_gpu_self_time import _random_tree, window_border_case
from test_self_time_host import FAULTS, synth

pytestmark = pytest.mark.gpu

ERR = anomod.FLAG_ERROR


def _check(ctx, sp, dev=None, ref=None, edges=True):
    """Everything the call returns for `sp` (or its device twin) == the model."""
    ref = origins_ref(sp) if ref is None else ref
    got = ctx.error_origins(sp if dev is None else dev, per_span=True)
    assert_origins_equal(got, ref)
    if edges:
        table = ctx.edge_aggregate(sp if dev is None else dev, with_hist=False)
        np.testing.assert_array_equal(got.origin + got.propagated, table.errors)
    return got


def _cls(got):
    return (got.span_state & 3).tolist()


def _fate(got):
    return (got.span_state >> 2).tolist()


# ------------------------------------------------------------------ hand-made
def test_hand_made_trace(ctx):
    sp, cls, fate, hops = hand_made()
    got = _check(ctx, sp)
    assert (_cls(got), _fate(got), got.span_hops.tolist()) == (cls, fate, hops)
    assert got.error_spans == 9 and got.loop_spans == 0
    both = anomod.SpanSet.concat([sp, sp])      # equal ids in two traces stay apart
    got = _check(ctx, both)
    assert (_cls(got), _fate(got), got.span_hops.tolist()) == (cls * 2, fate * 2, hops * 2)


def test_sixty_five_one_span_traces(ctx):
    """More one-span traces than a chunk's 64; every span starts and ends its
    failure.  (The share policy packs only the last 16 of them into one chunk:
    the 64-trace limit itself is met in test_gpu_walk_borders.py.)"""
    n = 65
    sp = build(3, [([t + 1], [0], [ERR], [t % 3]) for t in range(n)])
    got = _check(ctx, sp)
    assert set(got.span_state.tolist()) == {ORIGIN | SURFACED << 2} and not got.span_hops.any()
    assert got.error_spans == n and int(got.surfaced.sum()) == n and int(got.stopped.sum()) == 0


@pytest.mark.parametrize("variant", ["flagged", "clean_root", "reversed"])
@pytest.mark.parametrize("L_", [256, 257])
def test_chain_at_the_chunk_limit(ctx, L_, variant, monkeypatch, capfd):
    """A chain trace of 256 (one chunk: the 8th jump round) and of 257 spans
    (the long-trace kernel) between two 3-span chains, every span flagged."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    mid = chain_trace(L_, 100, flagged_root=variant != "clean_root", reverse=variant == "reversed")
    sp = build(4, [chain_trace(3, 10), mid, chain_trace(3, 5000)])
    got = _check(ctx, sp)
    assert f", {L_ - 256} long traces" in capfd.readouterr().err
    state, hops = got.span_state[3:3 + L_], got.span_hops[3:3 + L_]
    if variant == "reversed":
        state, hops = state[::-1], hops[::-1]
    depth = np.arange(L_)
    if variant == "clean_root":
        assert state[0] == ABSORBER and hops[0] == 0
        assert (state[1:-1] == PROPAGATED | CONTAINED << 2).all()
        assert state[-1] == ORIGIN | CONTAINED << 2 and hops[-1] == L_ - 2
        np.testing.assert_array_equal(hops[1:], depth[1:] - 1)
        # stopped once, on the row of the root's child: parent service 0, child 1
        assert int(got.stopped.sum()) == 1 and got.stopped[0 * 4 + 1] == 1
    else:
        assert (state[:-1] == PROPAGATED | SURFACED << 2).all()
        assert state[-1] == ORIGIN | SURFACED << 2 and hops[-1] == L_ - 1
        np.testing.assert_array_equal(hops, depth)
        assert int(got.stopped.sum()) == 0
    assert int(got.hops_max.max()) == hops[-1] and got.loop_spans == 0


@pytest.mark.parametrize("L_", [300, 200])
def test_star(ctx, L_):
    """A flagged root with L_ - 1 flagged children: the long-trace kernel
    (300) and one chunk (200).  Every child ORs into the same word."""
    ids = np.arange(1000, 1000 + L_, dtype=np.uint64)
    pid = np.r_[np.uint64(0), np.full(L_ - 1, 1000, np.uint64)]
    sp = build(2, [(ids, pid, np.full(L_, ERR), np.arange(L_) % 2)])
    got = _check(ctx, sp)
    assert got.span_state[0] == PROPAGATED | SURFACED << 2 and got.span_hops[0] == 0
    assert (got.span_state[1:] == ORIGIN | SURFACED << 2).all() and (got.span_hops[1:] == 1).all()
    assert int(got.origin.sum()) == L_ - 1 and int(got.hops_sum.sum()) == L_ - 1


@pytest.mark.parametrize("L_", [12, 300])
def test_reference_cycle(ctx, L_):
    """1 -> 2 -> 3 -> 1, all flagged, a flagged tail (4) hanging off 1, and a
    clean tree in the same trace: the four are in a loop, the call returns."""
    k = L_ - 4
    ids = np.r_[[1, 2, 3, 4], np.arange(100, 100 + k)].astype(np.uint64)
    pid = np.r_[[2, 3, 1, 1], [0], 100 + (np.arange(1, k) - 1) // 2].astype(np.uint64)
    flags = np.r_[[ERR] * 4, np.zeros(k)]
    sp = build(3, [(ids, pid, flags, np.arange(L_) % 3)])
    got = _check(ctx, sp)
    assert got.loop_spans == 4 and got.error_spans == 4
    assert _cls(got)[:4] == [PROPAGATED, PROPAGATED, PROPAGATED, ORIGIN]
    assert _fate(got)[:4] == [LOOP] * 4 and not got.span_hops.any()
    assert not got.span_state[4:].any() and int(got.stopped.sum() + got.surfaced.sum()) == 0


# ------------------------------------------------------------------ random trees
def _flagged_tree(rng, lens, share, **kw):
    sp = _random_tree(rng, lens, **kw)
    return with_flags(sp, (rng.random(sp.n_spans) < share) * ERR)


@pytest.mark.parametrize("S,n_long,kernel", [(9, 0, "bidir"), (30, 0, "split"), (9, 1, "split"),
                                             (9, 1, "forward")])
def test_random_trees(ctx, monkeypatch, capfd, S, n_long, kernel):
    """Unique ids, random ancestors, orphans, self-references, shuffled inside
    the traces, 30 % flags, traces of 1..256 spans (and one of 300): the three
    scans, counters in LDS (S = 9, 30) — declared unique with the scans from
    both ends forced on, and not declared unique."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    if kernel != "forward":
        monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "1")
    rng = np.random.default_rng(200 + S + n_long)
    lens = np.r_[rng.integers(100, 257, 40), rng.integers(1, 30, 60), [256], [300] * n_long]
    rng.shuffle(lens)
    sp = _flagged_tree(rng, lens, 0.3, S=S, self_ref=0.02)
    if kernel != "forward":
        assert sp.check_unique_ids()
    got = _check(ctx, sp)
    assert f"error_origins_kernel<{kernel}>, {n_long} long traces" in capfd.readouterr().err
    assert min(int(getattr(got, k).sum()) for k in got.TABLES) > 0
    assert got.loop_spans == 0


# ------------------------------------------------------------------ long traces
def test_one_shuffled_trace_of_5000_spans(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = _flagged_tree(np.random.default_rng(21), [5000], 0.6)
    got = _check(ctx, sp)
    assert "error_origins_kernel<forward>, 1 long traces" in capfd.readouterr().err
    assert int(got.hops_max.max()) >= 3 and int(got.absorbers.sum()) > 0


def test_shuffled_chain_of_5000_spans(ctx):
    """13 jump rounds, hops up to 4,999."""
    ids, pid, flags, svc = chain_trace(5000, 1, S=9)
    order = np.random.default_rng(3).permutation(5000)
    sp = build(9, [(ids[order], pid[order], flags[order], svc[order])])
    got = _check(ctx, sp)
    np.testing.assert_array_equal(got.span_hops[np.argsort(order)], np.arange(5000))
    assert int(got.hops_max.max()) == 4999 and int(got.origin.sum()) == 1


def test_long_and_short_traces_mixed(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(22)
    lens = np.r_[rng.integers(1, 60, 300), [257, 256, 2049, 4097]]
    rng.shuffle(lens)
    _check(ctx, _flagged_tree(rng, lens, 0.3))
    assert ", 3 long traces" in capfd.readouterr().err


def test_clean_long_trace_between_flagged_ones(ctx, monkeypatch, capfd):
    """The long-trace kernel leaves a trace without a flag alone."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    clean = chain_trace(300, 1000)
    clean = (clean[0], clean[1], np.zeros(300, np.uint16), clean[3])
    sp = build(4, [chain_trace(300, 1), clean, chain_trace(300, 2000, flagged_root=False)])
    got = _check(ctx, sp)
    assert ", 3 long traces" in capfd.readouterr().err
    assert not got.span_state[300:600].any() and got.error_spans == 599
    assert int(got.surfaced.sum()) == 1 and int(got.stopped.sum()) == 1


def test_duplicated_ids_at_window_and_block_borders(ctx, monkeypatch, capfd):
    """test_gpu_self_time.window_border_case with flags on the planted children
    and on both carriers of their parent ids: the first carrier gets the
    child-error bit, across the lookup's window and block borders."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, want = window_border_case()
    later = [2050, 2048, 4096]
    flags = np.zeros(sp.n_spans, np.uint16)
    flags[list(want) + list(want.values()) + later] = ERR
    sp = with_flags(sp, flags)
    got = _check(ctx, sp)
    assert "error_origins_kernel<forward>, 3 long traces" in capfd.readouterr().err
    cls = got.span_state & 3
    assert (cls[sorted(set(want.values()))] == PROPAGATED).all()
    # the later copies have no child (2048 and 4096 name their own id, which the
    # first carrier holds: they are its children)
    assert cls[2050] == ORIGIN and cls[2048] == ORIGIN and cls[4096] == ORIGIN


def test_long_topology(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=1, p_orphan_ppm=2000), 2000)
    n_long = int((np.diff(sp.trace_ptr) > 256).sum())
    assert n_long > 0
    busiest = sp.services[int(np.bincount(sp.svc).argmax())]
    sp = propagate_errors(sp, busiest, 0.3, 0.7, np.random.default_rng(5))
    got = _check(ctx, sp)
    assert f", {n_long} long traces" in capfd.readouterr().err
    assert int(got.origin.sum()) > 0 and int(got.propagated.sum()) > 0


# ------------------------------------------------------------------ synthetic sets
@pytest.fixture(scope="module", params=["SN", "TT"])
def synth_case(request):
    sp = propagated(request.param, 20000)
    return request.param, sp, origins_ref(sp)


def test_synthetic_parity(ctx, synth_case, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    topo, sp, ref = synth_case
    assert sp.unique_ids
    _check(ctx, sp, ref=ref)
    want = {"SN": "error_origins_kernel<bidir>", "TT": "error_origins_kernel<split>"}[topo]
    assert want + ", 0 long traces" in capfd.readouterr().err


def test_synthetic_shuffled_inside_traces(ctx, synth_case):
    """Equal tables; the columns against the reference of the download."""
    _, sp, ref = synth_case
    d = ctx.upload(sp)
    sh = ctx.shuffle(d, seed=5, window_traces=0)
    try:
        host = sh.download()
        assert not np.array_equal(host.span_id, sp.span_id)
        got = ctx.error_origins(sh, per_span=True)
        assert_origins_equal(got, ref, per_span=False)
        href = origins_ref(host)
        np.testing.assert_array_equal(got.span_state, href.span_state)
        np.testing.assert_array_equal(got.span_hops, href.hops)
        np.testing.assert_array_equal(got.origin + got.propagated,
                                      ctx.edge_aggregate(sh, with_hist=False).errors)
    finally:
        sh.free()
        d.free()


def test_device_grouped_set(ctx, synth_case):
    """Upload ungrouped, group on the device (max_trace_len unknown)."""
    _, sp, ref = synth_case
    order = np.random.default_rng(3).permutation(sp.n_spans)
    loose = sp.take(order, np.array([0, sp.n_spans], np.uint64))
    d = ctx.upload_ungrouped(loose)
    g = ctx.group(d)
    try:
        host = g.download()
        got = _check(ctx, host, dev=g)
        assert_origins_equal(got, ref, per_span=False)
    finally:
        g.free()
        d.free()


def test_no_flag_at_all(ctx):
    sp = synth("SN", 3000)
    sp = with_flags(sp, np.zeros(sp.n_spans))
    got = _check(ctx, sp)
    assert not any(getattr(got, k).any() for k in got.TABLES)
    assert not got.span_state.any() and not got.span_hops.any() and got.error_spans == 0


def test_empty_and_one_span(ctx):
    got = _check(ctx, build(2, []))
    assert got.span_state.shape == (0,) and got.error_spans == 0 and not got.origin.any()
    got = _check(ctx, build(2, [([5], [0], [ERR], [1])]))
    assert got.span_state.tolist() == [ORIGIN | SURFACED << 2] and got.origin[2 * 2 + 1] == 1
    got = _check(ctx, build(2, [([5], [0], [0], [1])]))
    assert got.span_state.tolist() == [CLEAN]


# ------------------------------------------------------------------ arguments
def test_argument_handling(ctx):
    sp = propagated("SN", 200)
    lib = anomod.lib()
    d = ctx.upload(sp)
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))
    try:
        S = sp.n_services
        cs = L.ErrorOriginsC(S)
        assert lib.anomod_error_origins_spans(ctx.handle, loose.handle, C.byref(cs)) == L.ESTATE
        assert b"not grouped" in lib.anomod_last_error(ctx.handle)
        cs = L.ErrorOriginsC(S - 1)
        assert lib.anomod_error_origins_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
        # NULL outputs are skipped: only origin and span_hops asked for
        ref = origins_ref(sp)
        origin = np.zeros(ref.origin.shape[0], np.uint64)
        hops = np.zeros(sp.n_spans, np.uint32)
        cs = L.ErrorOriginsC(S, 0, 0, L.ptr(origin, C.c_uint64), None, None, None, None, None,
                             None, None, L.ptr(hops, C.c_uint32))
        assert lib.anomod_error_origins_spans(ctx.handle, d.handle, C.byref(cs)) == L.OK
        np.testing.assert_array_equal(origin, ref.origin)
        np.testing.assert_array_equal(hops, ref.hops)
        assert (cs.error_spans, cs.loop_spans) == (ref.error_spans, 0)
    finally:
        loose.free()
        d.free()


def test_later_results_unchanged(ctx):
    """edge_aggregate and self_time of a device set are equal before and after
    the call, and a second call equals the first."""
    sp = propagated("TT", 1500)
    d = ctx.upload(sp)
    try:
        before, self_before = ctx.edge_aggregate(d), ctx.self_time(d)
        first = ctx.error_origins(d, per_span=True)
        after, self_after = ctx.edge_aggregate(d), ctx.self_time(d)
        again = ctx.error_origins(d, per_span=True)
        for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
            np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
            np.testing.assert_array_equal(getattr(self_after, k), getattr(self_before, k),
                                          err_msg=k)
        for k in first.TABLES + ("span_state", "span_hops"):
            np.testing.assert_array_equal(getattr(again, k), getattr(first, k), err_msg=k)
        assert (again.error_spans, again.loop_spans) == (first.error_spans, first.loop_spans)
    finally:
        d.free()


# ------------------------------------------------------------------ the ranking
def test_origin_rate_through_features(ctx):
    fault = FAULTS["SN"]
    sp = propagated("SN", 3000)
    c = sp.services.index(fault)
    exp = Experiment("cur", sp, label=fault)
    fo = anomod.features(exp, ctx, error_origins=True)
    assert fo.params["components"]["error_kind"] == "origin"
    assert_origins_equal(fo.error_origins, origins_ref(sp), per_span=False)
    rate = fo.params["components"]["error_rate"]
    assert rate[c] > 0 and (np.delete(rate, c) == 0.0).all()
    np.testing.assert_array_equal(rate, fo.error_origins.origin_rate(fo.edges.count))
    fi = anomod.features(exp, ctx)
    inc = fi.params["components"]["error_rate"]
    assert "error_kind" not in fi.params["components"] and fi.error_origins is None
    np.testing.assert_array_equal(inc, inclusive_error_rate(sp))
    assert (np.delete(inc, c) > 0).any()
    ranking = anomod.rank(fo, ctx=ctx)
    print("origin ranking:", ranking[:3], "inclusive:", anomod.rank(fi, ctx=ctx)[:3])
    assert ranking[0][0] == fault


def test_default_unchanged(ctx):
    exp = anomod.load_experiment(anomod.SynthSpec("SN", seed=4, fault_service=FAULTS["SN"]),
                                 n_traces=400)
    a = anomod.features(exp, ctx)
    b = anomod.features(exp, ctx, error_origins=False)
    assert a.error_origins is None and b.error_origins is None
    np.testing.assert_array_equal(a.service_scores, b.service_scores)
    assert a.params.keys() == b.params.keys()
    assert set(a.params["components"]) == set(b.params["components"]) == \
        {"error_rate", "latency", "metric"}
    for k, v in a.params["components"].items():
        np.testing.assert_array_equal(v, b.params["components"][k])
    assert {k: v for k, v in a.params.items() if k != "components"} == \
        {k: v for k, v in b.params.items() if k != "components"}

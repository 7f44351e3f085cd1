"""GPU: the critical path (csrc/critical_path.hip) against the reference helper
(tests/critical_path_ref.py), bit for bit — the edge table (count, errors,
sum, min, max, hist, p50 / p99 with NaNs equal) and the per-span cp_us and
on_path columns — plus argument handling, what the call leaves unchanged, and
the latency term through features()."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment

from critical_path_ref import (FANOUT_SERVICES, T0_US, cp_table_ref, critical_path_ref,
                               fanout_set, hand_set, nested_set, random_starts, with_cols)
from self_time_ref import assert_table_equal, parents_ref
from test_critical_path_host import P_SEQ, synth
from test_gpu_self_time import _random_tree, _spanset
from test_gpu_self_time import window_border_case

pytestmark = pytest.mark.gpu

FIELDS = ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us")


def _check(ctx, sp, dev=None, ref=None):
    """Table, cp_us and on_path of `sp` (or of its device twin) == reference."""
    if ref is None:
        cp, on, nsel = critical_path_ref(sp)
        ref = (cp, on, nsel, cp_table_ref(sp, cp, on))
    cp, on, _, tab = ref
    got = ctx.critical_path(sp if dev is None else dev, per_span=True)
    np.testing.assert_array_equal(got.on_path, on, err_msg="on_path")
    np.testing.assert_array_equal(got.cp_us, cp, err_msg="cp_us")
    assert_table_equal(got.edges, tab)
    return got, ref


def _with_start(sp, start):
    return with_cols(sp, start_us=np.asarray(start, np.uint64))


def _shuffled(sp, seed):
    """sp with every trace shuffled inside itself (ids stay unique)."""
    rng = np.random.default_rng(seed)
    ptr = sp.trace_ptr.astype(np.int64)
    order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])
    out = sp.take(order.astype(np.int64), sp.trace_ptr)
    out.unique_ids = sp.unique_ids
    return out


# ------------------------------------------------------------------ hand-made
def test_hand_made_traces(ctx):
    sp, want_on, want_cp = hand_set()
    got, _ = _check(ctx, sp)
    np.testing.assert_array_equal(got.on_path, want_on)
    np.testing.assert_array_equal(got.cp_us, want_cp)
    assert int(got.edges.count.sum()) == int(want_on.sum())
    assert int(got.edges.sum_us.sum()) == int(want_cp.sum())


# ------------------------------------------------------------------ synthetic sets
@pytest.fixture(scope="module", params=[("SN", "nested"), ("SN", "random"), ("TT", "nested"),
                                        ("TT", "random")], ids=lambda p: "-".join(p))
def synth_case(request):
    topo, kind = request.param
    sp = synth(topo, 2000)
    par = parents_ref(sp)
    sp = nested_set(sp, par, P_SEQ[topo], seed=7) if kind == "nested" else random_starts(sp, 9, par)
    cp, on, nsel = critical_path_ref(sp, par)
    return topo, kind, sp, (cp, on, nsel, cp_table_ref(sp, cp, on))


def test_synthetic_declared_unique(ctx, synth_case, monkeypatch, capfd):
    """As generated (unique ids, collector order): the scans from both ends."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    topo, kind, sp, ref = synth_case
    assert sp.unique_ids
    on = ref[1]
    assert 0.05 <= on.mean() <= 0.95     # neither everything nor nothing passes
    got, _ = _check(ctx, sp, ref=ref)
    want = {"SN": "critical_path_kernel<bidir>", "TT": "critical_path_kernel<split>"}[topo]
    assert want in capfd.readouterr().err
    if kind == "nested":                 # conservation, through the table
        head = parents_ref(sp) == -1
        assert int(got.edges.sum_us.sum()) == int(sp.dur_us[head].astype(np.uint64).sum())
    share = got.service_share()
    assert abs(share.sum() - 1.0) < 1e-12 and (share >= 0).all()


def test_synthetic_not_declared_unique(ctx, synth_case, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    _, _, sp, ref = synth_case
    plain = with_cols(sp)
    plain.unique_ids = False
    _check(ctx, plain, ref=ref)
    assert "critical_path_kernel<forward>" in capfd.readouterr().err


def test_synthetic_shuffled_inside_traces(ctx, synth_case):
    """Children before parents, other positions (the tie rule is positional):
    against the reference of the shuffled set."""
    _, _, sp, _ = synth_case
    sh = _shuffled(sp, seed=5)
    assert sh.unique_ids and not np.array_equal(sh.span_id, sp.span_id)
    _check(ctx, sh)


def test_device_generated_set(ctx):
    """2^14 traces generated on the device, start times filled there; compared
    after the download."""
    d = ctx.generate(anomod.SynthSpec("SN", seed=3, p_orphan_ppm=2000), 1 << 14)
    try:
        d.fill_start_synthetic(T0_US, 10_000_000, 37)
        host = d.download()
        assert host.start_us is not None and host.n_traces == 1 << 14
        got, (_, on, _, _) = _check(ctx, host, dev=d)
        assert 0 < on.sum() < host.n_spans
    finally:
        d.free()


# ------------------------------------------------------------------ hand-built shapes
def test_sixty_five_one_span_traces(ctx):
    """More one-span traces than a chunk's 64; every span is a head.  (The
    share policy packs only the last 16 of them into one chunk: the 64-trace
    limit itself is met in test_gpu_walk_borders.py.)"""
    n = 65
    sp = _spanset(3, [1] * n, np.arange(1, n + 1), np.zeros(n), np.arange(n) * 3)
    sp = _with_start(sp, T0_US + np.arange(n) * 10)
    got, _ = _check(ctx, sp)
    np.testing.assert_array_equal(got.cp_us, sp.dur_us)
    assert got.on_path.all()


@pytest.mark.parametrize("L_", [256, 257])
def test_trace_at_the_chunk_limit(ctx, L_, monkeypatch, capfd):
    """The same random tree with random starts at 256 (one chunk) and 257
    spans (long-trace kernel), between short traces (each of the three a chunk
    of its own: no dynamic tail, nothing is packed)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = _random_tree(np.random.default_rng(31), [3, L_, 3], dur_hi=5000)
    sp = random_starts(sp, seed=4)
    _, (_, on, nsel, _) = _check(ctx, sp)
    assert f", {L_ - 256} long traces" in capfd.readouterr().err
    assert 0 < on.sum() < sp.n_spans and nsel.max() >= 2


def _chain(N, first_id=1):
    """A chain N deep, every child inside its parent: cp_us = 2, the leaf 1."""
    sid = np.arange(first_id, first_id + N, dtype=np.uint64)
    pid = np.r_[np.uint64(0), sid[:-1]]
    dur = (np.arange(N)[::-1] * 2 + 1).astype(np.uint32)
    return sid, pid, dur, T0_US + np.arange(N)


def _star(n_children, simultaneous, first_id=1):
    """A root and its children, back to back (all selected, one per round) or
    all starting together (durations in four values: the first of the longest
    wins, every other child is off the path)."""
    k = np.arange(n_children)
    sid = np.arange(first_id, first_id + n_children + 1, dtype=np.uint64)
    pid = np.r_[np.uint64(0), np.full(n_children, first_id, np.uint64)]
    if simultaneous:
        cd = 100 + 10 * (k % 4)
        start = np.r_[T0_US, np.full(n_children, T0_US + 5)]
        root = 200
    else:
        cd = 7 + k % 3
        start = np.r_[T0_US, T0_US + 5 + np.r_[0, np.cumsum(cd)[:-1]]]
        root = int(cd.sum()) + 10
    return sid, pid, np.r_[root, cd].astype(np.uint32), start


def test_chunk_extremes(ctx):
    """In one chunk: a 256-deep chain (all 8 jump rounds), a star of 255
    back-to-back children (255 selection rounds), a star of 255 simultaneous
    children (one round, 254 losers)."""
    parts = [_chain(256, 1), _star(255, False, 1000), _star(255, True, 2000)]
    sid, pid, dur, start = (np.concatenate([p[k] for p in parts]) for k in range(4))
    sp = _with_start(_spanset(4, [256, 256, 256], sid, pid, dur), start)
    got, (_, on, nsel, _) = _check(ctx, sp)
    assert on[:256].all() and (got.cp_us[:255] == 2).all() and got.cp_us[255] == 1
    assert nsel[256] == 255 and on[256:512].all() and got.cp_us[256] == 10
    assert nsel[512] == 1 and on[512:].sum() == 2 and got.cp_us[512] == 200 - 130
    assert on[512 + 4] == 1            # the first child of 130 us (k = 3)


# ------------------------------------------------------------------ long traces
def test_one_shuffled_trace_of_5000_spans(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = _random_tree(np.random.default_rng(21), [5000])
    par = parents_ref(sp)
    for made in (random_starts(sp, 6, par), nested_set(sp, par, 0.5, 8)):
        _, (_, on, _, _) = _check(ctx, made)
        assert "critical_path_kernel<forward>, 1 long traces" in capfd.readouterr().err
        assert 0 < on.sum() < 5000


def test_long_chain_and_long_star(ctx):
    """A 5,000-deep chain (13 jump rounds) and a sequential star of 4,999
    children (4,999 selection rounds) through the long-trace kernel."""
    parts = [_chain(5000, 1), _star(4999, False, 10_000)]
    sid, pid, dur, start = (np.concatenate([p[k] for p in parts]) for k in range(4))
    sp = _with_start(_spanset(4, [5000, 5000], sid, pid, dur), start)
    got, (_, on, nsel, _) = _check(ctx, sp)
    assert on.all() and nsel[5000] == 4999 and got.cp_us[5000] == 10
    assert (got.cp_us[:4999] == 2).all()


def test_long_and_short_traces_mixed(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(22)
    lens = np.r_[rng.integers(1, 60, 300), [1000] * 5, [257, 256, 2049, 4097]]
    rng.shuffle(lens)
    sp = _random_tree(rng, lens, self_ref=0.01)
    sp = random_starts(sp, seed=12)
    _check(ctx, sp)
    assert ", 8 long traces" in capfd.readouterr().err
    sp.unique_ids = True    # ids are unique; in-trace shuffled: the order probe says forward
    _check(ctx, sp)
    assert ", 8 long traces" in capfd.readouterr().err


def test_duplicated_ids_at_window_and_block_borders(ctx, monkeypatch, capfd):
    """test_gpu_self_time.window_border_case: children of an id carried twice
    belong to the first carrier, across the lookup's window and block borders."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, want = window_border_case()
    par = parents_ref(sp)
    assert all(par[c] == p for c, p in want.items())
    for made in (random_starts(sp, 9, par), nested_set(sp, par, 0.5, 8)):
        _, (_, on, _, _) = _check(ctx, made)
        assert "critical_path_kernel<forward>, 3 long traces" in capfd.readouterr().err
        assert 0 < on.sum() < sp.n_spans


# ------------------------------------------------------------------ arguments
def test_argument_handling(ctx):
    sp = random_starts(synth("SN", 200), seed=2)
    lib = anomod.lib()
    S = sp.n_services
    cp, on, _ = critical_path_ref(sp)
    ref = cp_table_ref(sp, cp, on)
    d = ctx.upload(sp)
    bare = ctx.upload(anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id,
                                     sp.parent_span_id, sp.svc, sp.flags, sp.dur_us))
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))
    # spans [10, n - 7) lie in traces, the rest outside trace_ptr
    cut = sp.trace_ptr.copy()
    first, last = int(cut[3]), int(cut[-4])
    part = anomod.SpanSet(sp.services, cut[3:-3], sp.trace_hash, sp.span_id, sp.parent_span_id,
                          sp.svc, sp.flags, sp.dur_us, start_us=sp.start_us)
    try:
        table = anomod.EdgeTable.empty(sp.services, with_hist=False)
        cs = table.c_struct()
        args = (S, C.byref(cs), None, None)
        assert lib.anomod_edge_critical_path_spans(ctx.handle, bare.handle, *args) == L.ESTATE
        assert b"start-time column" in lib.anomod_last_error(ctx.handle)
        with pytest.raises(ValueError):
            ctx.critical_path(anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id,
                                             sp.parent_span_id, sp.svc, sp.flags, sp.dur_us))
        assert lib.anomod_edge_critical_path_spans(ctx.handle, loose.handle, *args) == L.ESTATE
        assert b"not grouped" in lib.anomod_last_error(ctx.handle)
        small = anomod.EdgeTable.empty(sp.services[:S - 1], with_hist=False)
        cs = small.c_struct()
        rc = lib.anomod_edge_critical_path_spans(ctx.handle, d.handle, S - 1, C.byref(cs), None,
                                                 None)
        assert rc == L.EINVAL
        # NULL outputs are skipped: only sum_us and on_path asked for
        sum_us = np.zeros(ref["sum_us"].shape[0], np.uint64)
        got_on = np.full(sp.n_spans, 9, np.uint8)
        cs = L.EdgeTableC(S, L.HIST_BINS, None, None, L.ptr(sum_us, C.c_uint64), None, None, None,
                          None, None)
        rc = lib.anomod_edge_critical_path_spans(ctx.handle, d.handle, S, C.byref(cs), None,
                                                 L.ptr(got_on, C.c_uint8))
        assert rc == L.OK
        np.testing.assert_array_equal(sum_us, ref["sum_us"])
        np.testing.assert_array_equal(got_on, on)
        # spans outside every trace read 0 / 0
        got = ctx.critical_path(part, per_span=True)
        pcp, pon, _ = critical_path_ref(part)
        np.testing.assert_array_equal(got.cp_us, pcp)
        np.testing.assert_array_equal(got.on_path, pon)
        assert not got.on_path[:first].any() and not got.cp_us[last:].any()
        np.testing.assert_array_equal(got.on_path[first:last], on[first:last])
        assert_table_equal(got.edges, cp_table_ref(part, pcp, pon))
        # n == 0
        empty = _with_start(_spanset(2, [], [], [], []), [])
        got = ctx.critical_path(empty, per_span=True)
        assert got.cp_us.shape == (0,) and got.on_path.shape == (0,)
        assert got.edges.count.sum() == 0 and np.isnan(got.edges.p99_us).all()
        assert (got.edges.min_us == 2**32 - 1).all()
    finally:
        loose.free()
        bare.free()
        d.free()


def test_hints_and_later_results_unchanged(ctx):
    """The call leaves the set's hints alone, and edge_aggregate, self_time
    and trace_spectrum after it equal what they gave before it."""
    sp = synth("TT", 1500)
    sp = nested_set(sp, parents_ref(sp), 0.5, seed=1)
    d = ctx.upload(sp)
    try:
        before = (ctx.edge_aggregate(d), ctx.self_time(d), ctx.trace_spectrum(d))
        hints = d.hints
        first = ctx.critical_path(d)
        assert d.hints == hints
        after = (ctx.edge_aggregate(d), ctx.self_time(d), ctx.trace_spectrum(d))
        again = ctx.critical_path(d)
        assert d.hints == hints
        for k in FIELDS:
            np.testing.assert_array_equal(getattr(after[0], k), getattr(before[0], k), err_msg=k)
            np.testing.assert_array_equal(getattr(after[1], k), getattr(before[1], k), err_msg=k)
            np.testing.assert_array_equal(getattr(again.edges, k), getattr(first.edges, k),
                                          err_msg=k)
        for k in ("n_traces", "svc_traces", "edge_traces", "bad_spans", "trace_abnormal"):
            np.testing.assert_array_equal(getattr(after[2], k), getattr(before[2], k), err_msg=k)
    finally:
        d.free()


# ------------------------------------------------------------------ through features()
def test_gateway_own_work_through_features(ctx):
    """+50 ms on the fan-out gateway's own work: the critical-path term names
    the gateway alone and the ranking puts it first; the self-time term
    misses it."""
    base, cur = fanout_set(200, seed=5), fanout_set(200, seed=5, gateway_extra_us=50_000)
    g = FANOUT_SERVICES.index("gateway")
    eb, ec = Experiment("base", base), Experiment("cur", cur, label="gateway")
    fb = anomod.features(eb, ctx, critical_path=True, self_time=True)
    assert fb.params["components"]["latency_kind"] == "inclusive"   # no baseline
    cp, on, _ = critical_path_ref(base)
    assert_table_equal(fb.cp_edges, cp_table_ref(base, cp, on))
    fc = anomod.features(ec, ctx, critical_path=True, self_time=True, baseline=fb)
    assert fc.params["components"]["latency_kind"] == "critical"    # ahead of "self"
    lat = fc.params["components"]["latency"]
    assert lat[g] > 0 and (np.delete(lat, g) == 0.0).all()
    fs = anomod.features(ec, ctx, self_time=True, baseline=fb)
    assert fs.params["components"]["latency_kind"] == "self" and fs.cp_edges is None
    assert fs.params["components"]["latency"][g] == 0.0
    # a baseline without the table: the next kind in line, and said so
    fm = anomod.features(ec, ctx, critical_path=True,
                         baseline=anomod.features(eb, ctx, self_time=True))
    assert fm.params["components"]["latency_kind"] == "inclusive"
    ranking = anomod.rank(fc, ctx=ctx)
    print("critical-path ranking:", ranking[:3])
    assert ranking[0][0] == "gateway"


def test_default_unchanged(ctx):
    exp = anomod.load_experiment(anomod.SynthSpec("SN", seed=4,
                                                  fault_service="home-timeline-service"),
                                 n_traces=400)
    a = anomod.features(exp, ctx)
    sp = exp.spans
    exp.spans = with_cols(sp, start_us=T0_US + np.arange(sp.n_spans, dtype=np.uint64) * 11)
    c = anomod.features(exp, ctx, critical_path=True)
    assert c.cp_edges is not None and c.params["components"]["latency_kind"] == "inclusive"
    exp.spans = sp
    b = anomod.features(exp, ctx)         # after the call: what it gave before it
    assert a.cp_edges is None and b.cp_edges is None
    np.testing.assert_array_equal(a.service_scores, b.service_scores)
    np.testing.assert_array_equal(c.service_scores, a.service_scores)
    assert set(a.params["components"]) == {"error_rate", "latency", "metric"}
    assert a.params["components"].keys() == b.params["components"].keys()
    for k, v in a.params["components"].items():
        np.testing.assert_array_equal(v, b.params["components"][k])
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(a.edges, k), getattr(b.edges, k), err_msg=k)

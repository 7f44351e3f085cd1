"""GPU: the self-time edge table (csrc/self_time.hip) against the reference
helper (tests/self_time_ref.py), bit for bit — count, errors, sum, min, max,
hist, p50 / p99 (NaNs equal) and the per-span self_us column — plus argument
handling, the propagated-fault property through features(), and the unchanged
default."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment

from self_time_ref import (add_delay, ancestors_and_descendants, assert_table_equal,
                           class_shares, parents_ref, self_table_ref, self_us_ref)
from test_self_time_host import DELAY_US, FAULTS, synth

pytestmark = pytest.mark.gpu

U32_MAX = 2**32 - 1


def _check(ctx, sp, dev=None, ref=None):
    """Table and self_us of `sp` (or of its device twin `dev`) == reference."""
    su = self_us_ref(sp)
    ref = self_table_ref(sp, su) if ref is None else ref
    got, got_su = ctx.self_time(sp if dev is None else dev, per_span=True)
    np.testing.assert_array_equal(got_su, su, err_msg="self_us")
    assert_table_equal(got, ref)
    return got, got_su


def _spanset(S, lens, sid, pid, dur, svc=None, flags=None):
    lens = np.asarray(lens, np.int64)
    ptr = np.zeros(lens.shape[0] + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    n = int(ptr[-1])
    sid = np.asarray(sid, np.uint64)
    svc = np.arange(n) % S if svc is None else svc
    flags = np.arange(n) % 7 == 0 if flags is None else flags
    return anomod.SpanSet([f"svc{i:02d}" for i in range(S)], ptr, sid.copy(), sid,
                          np.asarray(pid, np.uint64), np.asarray(svc, np.uint16),
                          np.asarray(flags, np.uint16), np.asarray(dur, np.uint32))


def _star(L_, first_id, dur_child, dur_root):
    """One trace: a root and L_ - 1 direct children."""
    sid = np.arange(first_id, first_id + L_, dtype=np.uint64)
    pid = np.r_[np.uint64(0), np.full(L_ - 1, first_id, np.uint64)]
    dur = np.r_[np.uint32(dur_root), np.full(L_ - 1, dur_child, np.uint32)]
    return sid, pid, dur


def _random_tree(rng, lens, orphan=0.03, dur_hi=20000, S=9, self_ref=0.0):
    """Traces of the given lengths: unique ids, random-ancestor parents (a
    share `self_ref` of the spans naming their own id), then every trace
    shuffled inside itself (children before parents)."""
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    starts = np.r_[0, np.cumsum(lens)[:-1]]
    t_of = np.repeat(np.arange(lens.shape[0]), lens)
    pos = np.arange(n) - starts[t_of]
    sid = rng.permutation(np.arange(1, n + 1, dtype=np.uint64)) + np.uint64(1 << 40)
    pick = starts[t_of] + (rng.random(n) * np.maximum(pos, 1)).astype(np.int64)
    pid = np.where(pos > 0, sid[pick], np.uint64(0))
    orph = (pos > 0) & (rng.random(n) < orphan)
    pid[orph] = rng.integers(1, 1 << 39, int(orph.sum()), dtype=np.uint64)
    own = rng.random(n) < self_ref
    pid[own] = sid[own]
    dur = rng.integers(0, dur_hi, n).astype(np.uint32)
    order = np.concatenate([s + rng.permutation(k) for s, k in zip(starts, lens)]).astype(np.int64)
    svc = rng.integers(0, S, n)
    return _spanset(S, lens, sid[order], pid[order], dur[order], svc[order],
                    (rng.random(n) < 0.1)[order])


# ------------------------------------------------------------------ synthetic sets
@pytest.fixture(scope="module", params=["SN", "TT"])
def synth_case(request):
    sp = synth(request.param, 20000)
    su = self_us_ref(sp)
    return request.param, sp, su, self_table_ref(sp, su)


def test_synthetic_parity_and_classes(ctx, synth_case, monkeypatch, capfd):
    """As generated (unique ids, collector order: the scans from both ends);
    each of the three self-time classes holds >= 10 % of the spans, so dur_us
    or 0 cannot pass."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    topo, sp, su, ref = synth_case
    assert sp.unique_ids
    shares = class_shares(sp, su)
    print(topo, "class shares:", np.round(shares, 3))
    assert min(shares) >= 0.10
    got, _ = _check(ctx, sp, ref=ref)
    want = {"SN": "self_time_kernel<bidir>", "TT": "self_time_kernel<split>"}[topo]
    assert want in capfd.readouterr().err
    table = ctx.edge_aggregate(sp, with_hist=False)
    np.testing.assert_array_equal(got.count, table.count)
    np.testing.assert_array_equal(got.errors, table.errors)
    assert int(got.sum_us.sum()) == int(su.astype(np.uint64).sum())


def test_synthetic_not_declared_unique(ctx, synth_case, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    _, sp, _, ref = synth_case
    plain = sp.select_traces(np.ones(sp.n_traces, bool))
    plain.unique_ids = False
    _check(ctx, plain, ref=ref)
    assert "self_time_kernel<forward>" in capfd.readouterr().err


def test_synthetic_shuffled_inside_traces(ctx, synth_case):
    """Same table as the unshuffled reference; self_us against the reference
    of the shuffled download."""
    _, sp, _, ref = synth_case
    d = ctx.upload(sp)
    sh = ctx.shuffle(d, seed=5, window_traces=0)
    try:
        host = sh.download()
        assert not np.array_equal(host.span_id, sp.span_id)
        got, got_su = ctx.self_time(sh, per_span=True)
        assert_table_equal(got, ref)
        np.testing.assert_array_equal(got_su, self_us_ref(host))
        table = ctx.edge_aggregate(sh, with_hist=False)
        np.testing.assert_array_equal(got.count, table.count)
        np.testing.assert_array_equal(got.errors, table.errors)
    finally:
        sh.free()
        d.free()


def test_device_grouped_set(ctx):
    """Upload ungrouped, group on the device (max_trace_len unknown)."""
    sp = synth("SN", 3000)
    rng = np.random.default_rng(3)
    order = rng.permutation(sp.n_spans)
    loose = sp.take(order, np.array([0, sp.n_spans], np.uint64))
    d = ctx.upload_ungrouped(loose)
    g = ctx.group(d)
    try:
        host = g.download()
        _check(ctx, host, dev=g)
        np.testing.assert_array_equal(ctx.self_time(g).count, self_table_ref(sp)["count"])
    finally:
        g.free()
        d.free()


# ------------------------------------------------------------------ hand-built shapes
def test_sixty_five_one_span_traces(ctx):
    """More one-span traces than a chunk's 64 — but the share policy walks the
    first 49 as chunks of their own and packs only the last 16 (65 // 4), so
    the 64-trace limit is not met here: test_gpu_walk_borders.py (pack_64x4,
    pack_65x4, pack_span_limit) closes chunks by it."""
    n = 65
    sp = _spanset(3, [1] * n, np.arange(1, n + 1), np.zeros(n), np.arange(n) * 3)
    got, su = _check(ctx, sp)
    np.testing.assert_array_equal(su, sp.dur_us)


@pytest.mark.parametrize("L_", [256, 257])
def test_trace_at_the_chunk_limit(ctx, L_):
    """A chain trace of exactly 256 (one chunk) / 257 spans (long-trace
    kernel) between short traces.  With three traces there is no dynamic tail
    (3 // 4 == 0): every trace is a chunk of its own, so this is about the
    trace's length, not about packing (253 + 3 against 254 + 3 is
    pack_span_limit in test_gpu_walk_borders.py)."""
    sid = np.arange(1, L_ + 7, dtype=np.uint64) + np.uint64(1 << 33)
    lens = [3, L_, 3]
    pid = np.r_[np.uint64(0), sid[:-1]]
    for s in (0, 3, 3 + L_):
        pid[s] = 0
    dur = (np.arange(L_ + 6)[::-1] * 11 + 5).astype(np.uint32)
    sp = _spanset(4, lens, sid, pid, dur)
    _, su = _check(ctx, sp)
    assert (su[3:3 + L_ - 1] == 11).all()  # a chain: dur minus the one child's


def test_fan_out_child_sum_does_not_wrap(ctx):
    """A 300-span trace whose root has 299 children of 2^32 - 1 us: the u64
    child sum must not wrap and the root's self time is 0."""
    sid, pid, dur = _star(300, 1000, U32_MAX, U32_MAX)
    sp = _spanset(2, [300], sid, pid, dur)
    _, su = _check(ctx, sp)
    assert su[0] == 0 and (su[1:] == U32_MAX).all()
    assert (299 * U32_MAX) % 2**32 < U32_MAX   # a wrapped u32 sum would leave self > 0
    # the same fan-out inside one chunk (LDS child sums), 200 spans
    sid, pid, dur = _star(200, 5000, U32_MAX, U32_MAX)
    _, su = _check(ctx, _spanset(2, [200], sid, pid, dur))
    assert su[0] == 0


def test_small_shapes(ctx):
    """Child before its parent, a duplicated id (children go to the first
    carrier), a self-reference, an orphan."""
    ids = [10, 20, 30, 20, 40, 50, 60]
    pids = [20, 0, 20, 20, 40, 999, 30]
    durs = [5, 100, 7, 50, 9, 11, 30]
    sp = _spanset(2, [7], ids, pids, durs, svc=[0, 1, 0, 1, 0, 1, 0])
    got, su = _check(ctx, sp)
    assert su.tolist() == [5, 38, 0, 50, 9, 11, 30]
    assert got.count[0 * 2 + 0] == 2      # a -> a: the self-reference and span 6 under span 2
    assert got.count[3 * 2 + 1] == 1      # ORPHAN -> b
    both = anomod.SpanSet.concat([sp, sp])  # the same ids in two traces stay apart
    _, su2 = _check(ctx, both)
    assert su2.tolist() == su.tolist() * 2
    uniq = _spanset(2, [3], [7, 8, 9], [8, 0, 9], [4, 10, 6])   # unique ids, a self-reference
    uniq.unique_ids = True
    _, su3 = _check(ctx, uniq)
    assert su3.tolist() == [4, 6, 6]


def test_zero_durations_one_span_and_empty(ctx):
    rng = np.random.default_rng(11)
    z = _random_tree(rng, [5, 40, 1, 17])
    z = anomod.SpanSet(z.services, z.trace_ptr, z.trace_hash, z.span_id, z.parent_span_id, z.svc,
                       z.flags, np.zeros(z.n_spans, np.uint32))
    got, su = _check(ctx, z)
    assert not su.any() and got.sum_us.sum() == 0 and got.count.sum() == z.n_spans
    one = _spanset(2, [1], [5], [0], [77])
    _, su = _check(ctx, one)
    assert su.tolist() == [77]
    empty = _spanset(2, [], [], [], [])
    got, su = _check(ctx, empty)
    assert su.shape == (0,) and got.count.sum() == 0 and np.isnan(got.p99_us).all()
    assert (got.min_us == U32_MAX).all()


@pytest.mark.parametrize("S,n_long,kernel", [(9, 0, "bidir"), (30, 0, "split"), (9, 1, "split")])
def test_forced_scans_from_both_ends(ctx, monkeypatch, capfd, S, n_long, kernel):
    """Unique ids, random ancestors, self-references and orphans, traces of
    1..256 spans (and one of 300), with the scans from both ends forced on
    (such sets are not in collector order): the SN-width u64 scan, and the
    split-word scan of wider tables and of sets with long traces, give the
    reference too."""
    monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "1")
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(100 + S)
    lens = np.r_[rng.integers(100, 257, 40), rng.integers(1, 30, 60), [256], [300] * n_long]
    rng.shuffle(lens)
    sp = _random_tree(rng, lens, S=S, self_ref=0.02)
    assert sp.check_unique_ids()
    assert ((sp.parent_span_id == sp.span_id) & (sp.span_id != 0)).sum() > 20
    _check(ctx, sp)
    assert f"self_time_kernel<{kernel}>, {n_long} long traces" in capfd.readouterr().err


# ------------------------------------------------------------------ long traces
def test_one_shuffled_trace_of_5000_spans(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = _random_tree(np.random.default_rng(21), [5000])
    _check(ctx, sp)
    assert "self_time_kernel<forward>, 1 long traces" in capfd.readouterr().err


def test_long_and_short_traces_mixed(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(22)
    lens = np.r_[rng.integers(1, 60, 300), [1000] * 5, [257, 256, 2049, 4097]]
    rng.shuffle(lens)
    sp = _random_tree(rng, lens)
    _check(ctx, sp)
    assert ", 8 long traces" in capfd.readouterr().err
    sp.unique_ids = True    # ids are unique; in-trace shuffled: the order probe says forward
    _check(ctx, sp)
    assert ", 8 long traces" in capfd.readouterr().err


def window_border_case(S=9):
    """Traces of 4097 / 2049 / 300 / 7 spans, not declared unique, for the
    long-trace parent lookup (windows of 2,048 ids, blocks of 4,096 spans):
    unique ids with earlier-span parents, unshuffled, then in the 4,097-span
    trace the same id planted at positions (5, 2050), (2047, 2048) and (4095,
    4096) — across a window border, on the two sides of one, and on the two
    sides of the block border — with children of each pair that sit nearer to
    the later copy: the first copy must win.  The span at 2048 names its own
    id (its first carrier is 2047, a window earlier), the one at 4096 too (no
    position follows it: the other child of that pair sits at 100), and span 3
    of the 2,049-span trace names the id of that trace's position 2048, the
    only span of its last window.  Returns (span set, {span: parent}), the
    parents checked against the host model and against the nearest copy."""
    rng = np.random.default_rng(77)
    lens = np.array([4097, 2049, 300, 7], np.int64)
    n = int(lens.sum())
    starts = np.r_[0, np.cumsum(lens)[:-1]]
    t_of = np.repeat(np.arange(lens.shape[0]), lens)
    pos = np.arange(n) - starts[t_of]
    sid = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(1 << 40)
    pick = starts[t_of] + (rng.random(n) * np.maximum(pos, 1)).astype(np.int64)
    pid = np.where(pos > 0, sid[pick], np.uint64(0))
    for first, later in ((5, 2050), (2047, 2048), (4095, 4096)):
        sid[later] = sid[first]
    s1 = int(starts[1])
    want = {2051: 5, 2049: 2047, 2048: 2047, 4096: 4095, 100: 4095, s1 + 3: s1 + 2048}
    for child, parent in want.items():
        pid[child] = sid[parent]
    pid[4095] = sid[0]              # (span 100 hangs under it: no reference cycle)
    pid[s1 + 2048] = sid[s1]        # (the same for span 3 of the second trace)
    sp = _spanset(S, lens, sid, pid, rng.integers(1, 20000, n), rng.integers(0, S, n),
                  rng.random(n) < 0.1)
    assert not sp.unique_ids and not sp.check_unique_ids()
    par = parents_ref(sp)
    for child, parent in want.items():
        assert par[child] == parent
    carriers = {c: np.flatnonzero(sp.span_id[:4097] == sp.parent_span_id[c]) for c in want if c < s1}
    nearest = {c: int(k[np.argmin(np.abs(k - c) + (k == c) * n)]) for c, k in carriers.items()}
    assert nearest == {2051: 2050, 2049: 2048, 2048: 2047, 4096: 4095, 100: 4095}
    assert all(len(k) == 2 and k[0] == want[c] for c, k in carriers.items())
    return sp, want


def test_duplicated_ids_at_window_and_block_borders(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, want = window_border_case()
    _, su = _check(ctx, sp)
    assert "self_time_kernel<forward>, 3 long traces" in capfd.readouterr().err
    # span 2047 carries its children's durations, span 2048 none (the model's
    # sums, spelled out for the pair on the two sides of a window border)
    kids = [c for c, p in enumerate(parents_ref(sp)) if p == 2047]
    assert {2048, 2049} <= set(kids) and not (parents_ref(sp) == 2048).any()
    assert su[2048] == sp.dur_us[2048]
    assert su[2047] == max(0, int(sp.dur_us[2047]) - int(sp.dur_us[kids].astype(np.int64).sum()))


def test_long_topology(ctx, monkeypatch, capfd):
    """SynthSpec("LONG"): unique ids, traces beyond a chunk; the long-trace
    kernel ran."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=1, p_orphan_ppm=2000), 2000)
    n_long = int((np.diff(sp.trace_ptr) > 256).sum())
    assert n_long > 0
    got, _ = _check(ctx, sp)
    assert f", {n_long} long traces" in capfd.readouterr().err
    table = ctx.edge_aggregate(sp, with_hist=False)
    np.testing.assert_array_equal(got.count, table.count)
    np.testing.assert_array_equal(got.errors, table.errors)


# ------------------------------------------------------------------ arguments
def test_argument_handling(ctx):
    sp = synth("SN", 200)
    lib = anomod.lib()
    d = ctx.upload(sp)
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))
    try:
        S = sp.n_services
        table = anomod.EdgeTable.empty(sp.services, with_hist=False)
        cs = table.c_struct()
        rc = lib.anomod_edge_self_time_spans(ctx.handle, loose.handle, S, C.byref(cs), None)
        assert rc == L.ESTATE
        assert b"not grouped" in lib.anomod_last_error(ctx.handle)
        small = anomod.EdgeTable.empty(sp.services[:S - 1], with_hist=False)
        cs = small.c_struct()
        rc = lib.anomod_edge_self_time_spans(ctx.handle, d.handle, S - 1, C.byref(cs), None)
        assert rc == L.EINVAL
        # NULL outputs are skipped: only sum_us and self_us asked for
        ref = self_table_ref(sp)
        sum_us = np.zeros(ref["sum_us"].shape[0], np.uint64)
        su = np.zeros(sp.n_spans, np.uint32)
        cs = L.EdgeTableC(S, L.HIST_BINS, None, None, L.ptr(sum_us, C.c_uint64), None, None, None,
                          None, None)
        rc = lib.anomod_edge_self_time_spans(ctx.handle, d.handle, S, C.byref(cs),
                                             L.ptr(su, C.c_uint32))
        assert rc == L.OK
        np.testing.assert_array_equal(sum_us, ref["sum_us"])
        np.testing.assert_array_equal(su, self_us_ref(sp))
    finally:
        loose.free()
        d.free()


def test_hints_and_later_results_unchanged(ctx):
    """An aggregation after the self-time call equals one before it."""
    sp = synth("TT", 1500)
    d = ctx.upload(sp)
    try:
        first = ctx.self_time(d)
        before = ctx.edge_aggregate(d)
        again = ctx.self_time(d)
        after = ctx.edge_aggregate(d)
        for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
            np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
            np.testing.assert_array_equal(getattr(again, k), getattr(first, k), err_msg=k)
    finally:
        d.free()


# ------------------------------------------------------------------ propagated fault
def test_propagated_fault_through_features(ctx):
    fault = FAULTS["SN"]
    base = synth("SN", 3000)
    par = parents_ref(base)
    anc, desc = ancestors_and_descendants(base, fault, par)
    assert anc and desc
    cur = add_delay(base, fault, DELAY_US, par)
    S, c = base.n_services, base.services.index(fault)
    tb, tc = ctx.self_time(base), ctx.self_time(cur)
    assert_table_equal(tb, self_table_ref(base))
    assert_table_equal(tc, self_table_ref(cur))
    other = np.arange((S + 2) * S) % S != c
    for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
        np.testing.assert_array_equal(getattr(tc, k)[other], getattr(tb, k)[other], err_msg=k)
    hit = ~other & (tb.count > 0)
    assert hit.any() and (tc.sum_us[hit] > tb.sum_us[hit]).all()

    eb, ec = Experiment("base", base), Experiment("cur", cur, label=fault)
    fb = anomod.features(eb, ctx, self_time=True)
    assert fb.params["components"]["latency_kind"] == "inclusive"   # no baseline
    fs = anomod.features(ec, ctx, self_time=True, baseline=fb)
    assert fs.params["components"]["latency_kind"] == "self"
    assert_table_equal(fs.self_edges, self_table_ref(cur))
    lat = fs.params["components"]["latency"]
    assert lat[c] > 0 and (np.delete(lat, c) == 0.0).all()
    fi = anomod.features(ec, ctx, self_time=False, baseline=fb)
    assert "latency_kind" not in fi.params["components"] and fi.self_edges is None
    inc = fi.params["components"]["latency"]
    assert (np.delete(inc, c) > 0).any()
    # a baseline without the self-time table: the inclusive shift, and said so
    fm = anomod.features(ec, ctx, self_time=True, baseline=anomod.features(eb, ctx))
    assert fm.params["components"]["latency_kind"] == "inclusive"
    np.testing.assert_array_equal(fm.params["components"]["latency"], inc)
    ranking = anomod.rank(fs, ctx=ctx)
    print("self-time ranking:", ranking[:3], "inclusive:", anomod.rank(fi, ctx=ctx)[:3])
    assert ranking[0][0] == fault


def test_default_unchanged(ctx):
    exp = anomod.load_experiment(anomod.SynthSpec("SN", seed=4, fault_service=FAULTS["SN"]),
                                 n_traces=400)
    a = anomod.features(exp, ctx)
    b = anomod.features(exp, ctx, self_time=False)
    assert a.self_edges is None and b.self_edges is None
    np.testing.assert_array_equal(a.service_scores, b.service_scores)
    assert a.params.keys() == b.params.keys()
    assert a.params["components"].keys() == b.params["components"].keys()
    assert set(a.params["components"]) == {"error_rate", "latency", "metric"}
    for k, v in a.params["components"].items():
        np.testing.assert_array_equal(v, b.params["components"][k])
    assert {k: v for k, v in a.params.items() if k != "components"} == \
        {k: v for k, v in b.params.items() if k != "components"}
    c = anomod.features(exp, ctx, self_time=True)
    np.testing.assert_array_equal(c.service_scores, a.service_scores)
    assert c.self_edges is not None

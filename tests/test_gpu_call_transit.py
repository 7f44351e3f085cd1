"""GPU: the call transit (csrc/call_transit.hip) against the exact host model
(tests/call_transit_ref.py), bit for bit — the two tables, the five count
arrays, the scalars and the three per-span columns — plus the invariants of
the definition, the kernel path taken (ANOMOD_LOG_KERNEL), argument handling,
what the call leaves unchanged, and the transit shift through features()."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment, _squash

from call_transit_ref import (CALL, EARLY, LATE, PAIRED, T0_US, TIMED, U32_MAX, assert_invariants,
                              assert_transit_equal, build, check_hand_made, hand_made,
                              transit_ref, transit_set)
from critical_path_ref import random_starts
from self_time_ref import parents_ref
from test_gpu_self_time import _random_tree, window_border_case

pytestmark = pytest.mark.gpu

FIELDS = ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us")


def _check(ctx, sp, dev=None, ref=None):
    """Everything the call returns for `sp` (or its device twin) == the model,
    and the invariants hold on the result."""
    par = parents_ref(sp)
    ref = transit_ref(sp, par) if ref is None else ref
    got = ctx.call_transit(sp if dev is None else dev, per_span=True)
    assert_transit_equal(got, ref)
    assert_invariants(got, sp, par)
    return got


def _timed_tree(rng, lens, seed, holes=0.05, **kw):
    """_random_tree (orphans, shuffled inside the traces) with random_starts
    (children start anywhere around their parent's interval) and a share of
    the start times zeroed."""
    sp = random_starts(_random_tree(rng, lens, **kw), seed)
    sp.start_us = np.where(rng.random(sp.n_spans) < holes, 0, sp.start_us).astype(np.uint64)
    return sp


def _every_class(got):
    """Paired, early, late, untimed and a call with both records all occur."""
    st = got.span_state
    assert int(((st & PAIRED) != 0).sum()) > 0 and int(((st & PAIRED) == 0).sum()) > 0
    assert int(got.early.sum()) > 0 and int(got.late.sum()) > 0 and int(got.untimed.sum()) > 0
    assert int((st == (CALL | PAIRED | TIMED)).sum()) > 0
    assert int(got.request.count.sum()) > 0 and int(got.response.count.sum()) > 0


# ------------------------------------------------------------------ hand-made
def test_hand_made_trace(ctx):
    sp = hand_made()
    check_hand_made(_check(ctx, sp))
    both = anomod.SpanSet.concat([sp, sp])      # equal ids in two traces stay apart
    check_hand_made(_check(ctx, both), 2)


def test_sixty_five_one_span_traces(ctx, monkeypatch, capfd):
    """More one-span traces than a chunk's 64: heads only, nothing recorded."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = build(3, [[(t + 1, 0, t % 3, 100 + t, 5, t % 2)] for t in range(65)])
    got = _check(ctx, sp)
    assert "call_transit_kernel<forward>, 0 long traces" in capfd.readouterr().err
    assert (got.calls, got.paired) == (0, 0) and not got.span_state.any()
    assert not got.request.count.any() and not got.response.count.any()
    assert np.isnan(got.request.p99_us).all() and (got.response.min_us == U32_MAX).all()
    assert not any(getattr(got, k).any() for k in got.TABLES)


def _small(first_id, svc=1):
    """A client span and its callee: one paired call, request 3, response 2."""
    return [(first_id, 0, 0, 500, 20), (first_id + 1, first_id, svc, 503, 15)]


@pytest.mark.parametrize("L_", [256, 257])
@pytest.mark.parametrize("shape", ["chain", "star"])
def test_trace_at_the_chunk_limit(ctx, L_, shape, monkeypatch, capfd):
    """A trace that fills the chunk and one span more (the long-trace kernel),
    between two small traces: a chain (every call paired, one kid per span)
    and a star (kids = L - 1 on the root, nothing paired)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    i = np.arange(L_)
    if shape == "chain":    # starts wander around the parent's, ends too: every class but untimed
        rows = [(100 + k, 0 if k == 0 else 99 + k, k % 3, 10_000 + 7 * k - (k % 5) * 9,
                 5_000 - 9 * k + (k % 4) * 6, k % 11 == 0) for k in i.tolist()]
    else:
        rows = [(100 + k, 0 if k == 0 else 100, k % 3, 10_000 + k, 50) for k in i.tolist()]
    sp = build(3, [_small(10), rows, _small(5000, 2)])
    got = _check(ctx, sp)
    assert f"call_transit_kernel<forward>, {L_ - 256} long traces" in capfd.readouterr().err
    assert got.calls == L_ - 1 + 2
    if shape == "chain":
        assert got.paired == L_ - 1 + 2
        assert int(got.early.sum()) > 0 and int(got.late.sum()) > 0
        assert int(got.request.errors.sum()) > 0
    else:
        assert got.paired == 2 and int(got.request.count.sum()) == 2
        assert (got.span_state[3:2 + L_] == CALL).all()


def test_edge_values(ctx):
    """Equal starts and equal ends (records of 0), gaps of 2^32 - 1 and 2^32
    either way (both read 2^32 - 1), starts near 2^64 whose ends saturate, and
    a duplicated parent id with one child per carrier (both count on the first
    carrier: unpaired)."""
    top = 2**64 - 1
    s = 10
    pairs = [(500, 100, 500, 100, 1), (500, 100, 499, 102, 0)]
    for gap in (U32_MAX, U32_MAX + 1):
        pairs += [(s, U32_MAX, s + gap, 0, 0), (s + gap, 5, s, 1, 0), (s + gap + 7, 0, s, 7, 1),
                  (s, 1, s + 1 + gap - 4, 4, 0)]
    pairs += [(top - 10, 100, top - 5, 100, 0), (top - 10, 4, top - 5, 100, 0),
              (top - 10, 100, top - 8, 3, 0), (top, 0, top, U32_MAX, 0), (top, U32_MAX, 1, 0, 0)]
    rows = [[(1, 0, 0, ps, pd), (2, 1, 1, cs, cd, f)] for ps, pd, cs, cd, f in pairs]
    rows.append([(1, 0, 0, 100, 100), (5, 1, 0, 110, 20), (5, 1, 0, 140, 20), (6, 5, 1, 112, 5),
                 (7, 5, 1, 142, 5)])
    got = _check(ctx, build(2, rows))
    assert got.paired == len(pairs) and got.calls == len(pairs) + 4
    assert got.request.max_us[1] == U32_MAX == got.response.max_us[1]
    assert got.request.min_us[1] == 0 == got.response.min_us[1]
    assert (got.span_state[-4:] == CALL).all()


# ------------------------------------------------------------------ scans
@pytest.mark.parametrize("S,unique,kernel", [(9, False, "forward"), (9, True, "bidir"),
                                             (24, True, "split")])
def test_the_three_scans(ctx, monkeypatch, capfd, S, unique, kernel):
    """The same random trees (unique ids, random ancestors, orphans,
    self-references, shuffled inside the traces, traces of 1..256 spans, random
    starts with zeros among them) not declared unique, declared unique with
    the scans from both ends forced on, and over 24 services (E = 624 rows:
    the split-word scan)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    if unique:
        monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "1")
    rng = np.random.default_rng(300)
    lens = np.r_[rng.integers(100, 257, 30), rng.integers(1, 30, 60), [256]]
    rng.shuffle(lens)
    sp = _timed_tree(rng, lens, seed=4, S=9, self_ref=0.02)
    if S == 24:     # the same trees over more services: 8 -> 23, others as they are
        sp.services = [f"svc{i:02d}" for i in range(24)]
        sp.svc = np.where(sp.svc == 8, 23, sp.svc).astype(np.uint16)
    if unique:
        assert sp.check_unique_ids()
    got = _check(ctx, sp)
    assert f"call_transit_kernel<{kernel}>, 0 long traces" in capfd.readouterr().err
    _every_class(got)
    assert got.request.count[(S - 1) * S:S * S].any() or got.request.count[S - 1:S * S:S].any()


# ------------------------------------------------------------------ counters
def test_every_paired_call_of_one_row_early_and_late(ctx, monkeypatch, capfd):
    """3,000 two-span traces and one trace of 601 spans (the long-trace kernel)
    in which every paired call lies on the row 0 -> 1, starts almost 2^32 us
    before its parent and ends after it: every event lands on one row's
    counters, and early_us sums past 2^32 (a u32 partial sum wraps with the
    second event) without wrapping."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    big = T0_US
    rows = [[(2 * t + 1, 0, 0, big + t, 10), (2 * t + 2, 2 * t + 1, 1, big + t - (2**32 - 100) - t % 3, 2**32 - 1)]
            for t in range(3000)]
    long = [(10_000, 0, 0, big, 100)]
    for k in range(300):    # the root's 300 client spans (unpaired) and their callees (paired)
        long.append((20_000 + k, 10_000, 0, big + k, 10))
        long.append((30_000 + k, 20_000 + k, 1, big + k - (2**32 - 100), 2**32 - 1))
    sp = build(2, rows + [long])
    got = _check(ctx, sp)
    assert "call_transit_kernel<forward>, 1 long traces" in capfd.readouterr().err
    assert (got.calls, got.paired) == (3000 + 600, 3300)
    assert got.early.tolist()[:4] == [0, 3300, 0, 0] and got.late[1] == 3300
    assert got.early_us[1] == 3300 * (2**32 - 100) + 3000 > 2**32 * 3000
    assert got.late_us[1] == 3300 * 89 - 3000
    assert not got.request.count.any() and not got.response.count.any()
    assert (got.span_state[1:6000:2] == (CALL | PAIRED | TIMED | EARLY | LATE)).all()


def test_wide_table_overflows_the_sparse_counters(ctx):
    """S = 40 (1,680 rows).  One trace of 6,001 spans — a root, 3,000 client
    spans and their callees on random services, a quarter untimed, the others
    early and late — is counted by one workgroup, which meets more (kind, row)
    pairs than its sparse table has slots: the adds that find none go to the
    global words.  Beside it 40 full chunks of random trees.  The same arrays."""
    rng = np.random.default_rng(8)
    sp = _timed_tree(rng, [256] * 40, seed=9, holes=0.2, S=40)
    psvc, csvc = rng.integers(0, 40, 3000).tolist(), rng.integers(0, 40, 3000).tolist()
    long = [(1, 0, 0, T0_US, 100)]
    for k in range(3000):
        long.append((10 + k, 1, psvc[k], T0_US + k, 10))
        long.append((10_000 + k, 10 + k, csvc[k], 0 if k % 4 == 0 else T0_US + k - 5, 30))
    one = build(40, [long])
    got = _check(ctx, one)
    used = sum(int((getattr(got, k) > 0).sum()) for k in ("untimed", "early", "late"))
    assert used > 2 * 512      # more than the workgroup's table holds
    assert (got.calls, got.paired, int(got.untimed.sum())) == (6000, 3000, 750)
    _check(ctx, anomod.SpanSet.concat([sp, one]))


# ------------------------------------------------------------------ long traces
def test_duplicated_ids_at_window_and_block_borders(ctx, monkeypatch, capfd):
    """test_gpu_self_time.window_border_case: the children of a duplicated id
    count on the first carrier across the lookup's window and block borders
    (traces of 4,097 and 2,049 spans)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, want = window_border_case()
    sp = random_starts(sp, 3)
    sp.start_us[::17] = 0
    got = _check(ctx, sp)
    assert "call_transit_kernel<forward>, 3 long traces" in capfd.readouterr().err
    par = parents_ref(sp)
    for child, parent in want.items():
        assert par[child] == parent and got.span_state[child] & CALL
    _every_class(got)


def test_long_and_short_traces_mixed(ctx, monkeypatch, capfd):
    """2,049 and 4,097 spans: one past the window and the block of big_parents."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(22)
    lens = np.r_[rng.integers(1, 60, 300), [257, 256, 2049, 4097]]
    rng.shuffle(lens)
    got = _check(ctx, _timed_tree(rng, lens, seed=5))
    assert ", 3 long traces" in capfd.readouterr().err
    _every_class(got)


def test_chain_of_5000_spans(ctx):
    """Every span but the last has one kid: 4,999 paired calls."""
    k = np.arange(5000)
    rows = [(1 + j, j, j % 9, T0_US + 3 * j - (j % 7) * 4, 40_000 - 6 * j + (j % 5) * 3, j % 3 == 0)
            for j in k.tolist()]
    got = _check(ctx, build(9, [rows]))
    assert (got.calls, got.paired) == (4999, 4999)
    assert int(got.request.count.sum() + got.early.sum()) == 4999 and int(got.early.sum()) > 0


def test_one_shuffled_trace_of_5000_spans(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(21)
    got = _check(ctx, _timed_tree(rng, [5000], seed=6, S=4))
    assert "call_transit_kernel<forward>, 1 long traces" in capfd.readouterr().err
    _every_class(got)


@pytest.mark.parametrize("L_", [66_001, 65_538])
def test_star_beyond_16_bits(ctx, L_):
    """A root with 66,000 children, and with 2^16 + 1 — a kids count kept in
    16 bits would read 1 there and pair every child.  Nothing is paired."""
    n = L_ - 1
    ids = np.arange(1, L_ + 1, dtype=np.uint64)
    sp = anomod.SpanSet(["a", "b"], np.array([0, L_], np.uint64), np.ones(L_, np.uint64), ids,
                        np.r_[np.uint64(0), np.ones(n, np.uint64)], np.r_[0, np.ones(n)].astype(np.uint16),
                        np.zeros(L_, np.uint16), np.full(L_, 10, np.uint32),
                        start_us=T0_US + np.arange(L_, dtype=np.uint64))
    got = _check(ctx, sp)
    assert n > 1 << 16 and (got.calls, got.paired) == (n, 0)
    assert (got.span_state[1:] == CALL).all() and not got.request.count.any()


# ------------------------------------------------------------------ resident sets
def test_device_grouped_set_hints_and_later_results_unchanged(ctx):
    """Upload ungrouped, group on the device, give the set its start column:
    the same result as for the host set; the set's hints and a later
    edge_aggregate are what they were, and a second call equals the first."""
    rng = np.random.default_rng(31)
    sp = _random_tree(rng, rng.integers(1, 120, 200), S=7)
    sp.trace_hash = np.repeat(rng.permutation(sp.n_traces).astype(np.uint64) + 1000,
                              np.diff(sp.trace_ptr).astype(np.int64))   # what the device groups by
    order = rng.permutation(sp.n_spans)
    loose = sp.take(order, np.array([0, sp.n_spans], np.uint64))
    d = ctx.upload_ungrouped(loose)
    g = ctx.group(d)
    try:
        host = random_starts(g.download(), 8)
        host.start_us[::13] = 0
        g.set_start_us(host.start_us)
        ctx.self_time(g)                    # probes the order hint
        before, hints = ctx.edge_aggregate(g), g.hints
        ref = transit_ref(host)
        first = _check(ctx, host, dev=g, ref=ref)
        assert g.hints == hints
        assert_transit_equal(ctx.call_transit(host, per_span=True), ref)    # uploaded for the call
        after = ctx.edge_aggregate(g)
        again = ctx.call_transit(g, per_span=True)
        assert g.hints == hints
        for k in FIELDS:
            np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
        assert_transit_equal(again, ref)
        _every_class(first)
        # without the histogram and the columns: the same tables
        lean = ctx.call_transit(g, with_hist=False)
        assert lean.request.hist is None and lean.span_state is None
        assert_transit_equal(lean, ref, per_span=False)
    finally:
        g.free()
        d.free()


# ------------------------------------------------------------------ arguments
def test_argument_handling(ctx):
    rng = np.random.default_rng(2)
    sp = _timed_tree(rng, rng.integers(1, 80, 60), seed=2, S=5)
    lib = anomod.lib()
    S = sp.n_services
    E = (S + 2) * S
    ref = transit_ref(sp)
    bare_host = anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id,
                               sp.parent_span_id, sp.svc, sp.flags, sp.dur_us)
    d = ctx.upload(sp)
    bare = ctx.upload(bare_host)
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))

    def call(handle, n_services=S, tables=None, **arrays):
        req = anomod.EdgeTable.empty(sp.services[:n_services], with_hist=False)
        resp = anomod.EdgeTable.empty(sp.services[:n_services], with_hist=False)
        rq, rs = (req.c_struct(), resp.c_struct()) if tables is None else tables
        cs = L.CallTransitC(n_services, 0, 0, C.pointer(rq), C.pointer(rs))
        for k, (a, ct) in arrays.items():
            setattr(cs, k, L.ptr(a, ct))
        return lib.anomod_call_transit_spans(ctx.handle, handle, C.byref(cs)), cs, req, resp

    try:
        assert call(bare.handle)[0] == L.ESTATE
        assert b"start-time column" in lib.anomod_last_error(ctx.handle)
        with pytest.raises(ValueError):
            ctx.call_transit(bare_host)
        assert call(loose.handle)[0] == L.ESTATE
        assert b"not grouped" in lib.anomod_last_error(ctx.handle)
        assert call(d.handle, S - 1)[0] == L.EINVAL
        cs = L.CallTransitC(S)                      # the two tables are required
        assert lib.anomod_call_transit_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
        # NULL arrays are skipped: only late_us and span_state asked for, and
        # only sum_us of the response table
        late_us = np.full(E, 9, np.uint64)
        state = np.full(sp.n_spans, 9, np.uint8)
        sum_us = np.full(E, 9, np.uint64)
        rq = L.EdgeTableC(S, L.HIST_BINS)
        rs = L.EdgeTableC(S, L.HIST_BINS, None, None, L.ptr(sum_us, C.c_uint64))
        rc, cs, _, _ = call(d.handle, tables=(rq, rs), late_us=(late_us, C.c_uint64),
                            span_state=(state, C.c_uint8))
        assert rc == L.OK and (cs.calls, cs.paired) == (ref.calls, ref.paired)
        np.testing.assert_array_equal(late_us, ref.late_us)
        np.testing.assert_array_equal(state, ref.span_state)
        np.testing.assert_array_equal(sum_us, ref.response["sum_us"])
        rc, cs, req, resp = call(d.handle)          # no array at all
        assert rc == L.OK and cs.paired == ref.paired
        np.testing.assert_array_equal(req.count, ref.request["count"])
        np.testing.assert_array_equal(resp.p99_us, ref.response["p99_us"])
        # n == 0: empty tables and zeros
        got = _check(ctx, build(2, []))
        assert got.span_state.shape == (0,) and (got.calls, got.paired) == (0, 0)
        assert got.request.count.sum() == 0 and np.isnan(got.response.p99_us).all()
        assert (got.request.min_us == U32_MAX).all() and not got.early_us.any()
        # one span: a head
        got = _check(ctx, build(2, [[(5, 0, 1, 3, 4, 1)]]))
        assert got.span_state.tolist() == [0] and got.calls == 0
    finally:
        loose.free()
        bare.free()
        d.free()


# ------------------------------------------------------------------ the ranking
def test_transit_shift_through_features(ctx):
    """+20 ms on the request and +5 ms on the response gap of the pair into b,
    a quarter of those calls abandoned: b's own duration and self time stay
    what they were, so the latency term says nothing; the transit term names
    b alone.  One synthetic scenario shows the mechanism, not ranking quality:
    no top-1 is asserted."""
    base = transit_set(2000, 17)
    cur = transit_set(2000, 17, slow="b", d_req=20_000, d_resp=5_000, abandon=0.25)
    names = base.services
    b = names.index("b")
    e_base, e_cur = Experiment("base", base), Experiment("cur", cur, label="b")
    fb = anomod.features(e_base, ctx, transit=True)
    plain = anomod.features(e_base, ctx)
    # without a baseline: no score changes, every earlier component is what it was
    assert "transit_shift" not in fb.params["components"]
    np.testing.assert_array_equal(fb.service_scores, plain.service_scores)
    assert set(fb.params["components"]) - set(plain.params["components"]) == \
        {"abandoned_rate", "skew_rate"}
    for k, v in plain.params["components"].items():
        np.testing.assert_array_equal(fb.params["components"][k], v, err_msg=k)
    on = anomod.features(e_cur, ctx, baseline=fb, transit=True)
    off = anomod.features(e_cur, ctx, baseline=fb)
    ref = transit_ref(cur)
    assert_transit_equal(on.transit, ref, per_span=False)
    comp = on.params["components"]
    shift = comp["transit_shift"]
    print("transit_shift:", dict(zip(names, shift.tolist())))
    assert shift[b] > 0 and len(shift) == 4 and (np.delete(shift, b) == 0.0).all()
    assert comp["latency"][b] == 0.0 and off.params["components"]["latency"][b] == 0.0
    fb_self = anomod.features(e_base, ctx, self_time=True)
    on_self = anomod.features(e_cur, ctx, baseline=fb_self, self_time=True)
    assert on_self.params["components"]["latency_kind"] == "self"
    assert on_self.params["components"]["latency"][b] == 0.0
    row = names.index("a") * 4 + b
    want = ref.late[row] / (ref.response["count"][row] + ref.late[row])
    assert comp["abandoned_rate"][b] == want > 0.2
    assert (np.delete(comp["abandoned_rate"], b) == 0.0).all() and not comp["skew_rate"].any()
    np.testing.assert_array_equal(on.service_scores - off.service_scores,
                                  (off.service_scores + 0.25 * _squash(shift)) - off.service_scores)
    np.testing.assert_array_equal(on.service_scores, off.service_scores + 0.25 * _squash(shift))
    for title, f in (("without --transit", off), ("with --transit", on)):
        print(title, anomod.rank(f, ctx=ctx))


def test_default_unchanged(ctx):
    """With the flag off, the score, the parameters and the components are
    what a call without the flag gives."""
    e_base = Experiment("base", transit_set(300, 1))
    exp = Experiment("cur", transit_set(300, 2, slow="c", d_req=900))
    fb = anomod.features(e_base, ctx)
    a = anomod.features(exp, ctx, baseline=fb)
    b = anomod.features(exp, ctx, baseline=fb, transit=False)
    assert a.transit is None and b.transit is None
    np.testing.assert_array_equal(a.service_scores, b.service_scores)
    assert set(a.params["components"]) == set(b.params["components"]) == \
        {"error_rate", "latency", "metric"}
    for k, v in a.params["components"].items():
        np.testing.assert_array_equal(v, b.params["components"][k])

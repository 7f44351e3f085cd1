"""GPU: the call repeats (csrc/call_repeats.hip) against the exact host model
(tests/call_repeats_ref.py), bit for bit — the nine tables, the scalars and both
per-span columns — plus the invariants of the definition, groups + repeats ==
the edge table's count, argument handling, what the call leaves unchanged, and
the amplification shift through features()."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment, _squash

from call_repeats_ref import (add_repeats, assert_invariants, assert_repeats_equal, build,
                              hand_made, repeats_ref, star)
from self_time_ref import NO_PARENT, parents_ref
from test_gpu_self_time import _random_tree, window_border_case
from test_self_time_host import FAULTS, synth

pytestmark = pytest.mark.gpu

ERR = anomod.FLAG_ERROR


def _check(ctx, sp, dev=None, ref=None):
    """Everything the call returns for `sp` (or its device twin) == the model;
    the invariants hold on the result; groups + repeats plus the spans that
    name themselves is the edge table's count on the first S * S rows."""
    ref = repeats_ref(sp) if ref is None else ref
    got = ctx.call_repeats(sp if dev is None else dev, per_span=True)
    assert_repeats_equal(got, ref)
    par = parents_ref(sp)
    assert_invariants(got, sp, par)
    S = sp.n_services
    table = ctx.edge_aggregate(sp if dev is None else dev, with_hist=False)
    heads = sp.svc[(par == NO_PARENT) & (sp.parent_span_id == sp.span_id) &
                   (sp.parent_span_id != 0)].astype(np.int64)
    selfs = np.bincount(heads * S + heads, minlength=S * S)      # row svc -> svc
    np.testing.assert_array_equal((got.groups + got.repeats)[:S * S] + selfs,
                                  table.count[:S * S])
    return got


def _timed(sp, rng, hi=6):
    """sp with start times and durations drawn from a few values: zeros, ties
    and zero durations all occur."""
    return anomod.SpanSet(list(sp.services), sp.trace_ptr, sp.trace_hash, sp.span_id,
                          sp.parent_span_id, sp.svc, sp.flags,
                          rng.integers(0, 3, sp.n_spans).astype(np.uint32), sp.trace_ids,
                          sp.unique_ids, start_us=rng.integers(0, hi, sp.n_spans).astype(np.uint64))


def _flagged_tree(rng, lens, share=0.3, **kw):
    sp = _random_tree(rng, lens, **kw)
    sp.flags = ((rng.random(sp.n_spans) < share) * ERR).astype(np.uint16)
    return sp


# ------------------------------------------------------------------ hand-made
def test_hand_made_trace(ctx):
    sp, size, want = hand_made()
    got = _check(ctx, sp)
    assert got.span_group_size.tolist() == size
    for k, rows in want.items():
        assert {r: int(v) for r, v in enumerate(getattr(got, k)) if v} == rows, k
    assert (got.grouped_spans, got.max_size, got.timed) == (9, 2, False)
    both = anomod.SpanSet.concat([sp, sp])      # equal ids in two traces stay apart
    got = _check(ctx, both)
    assert got.span_group_size.tolist() == size * 2
    for k, rows in want.items():
        twice = rows if k == "size_max" else {r: 2 * v for r, v in rows.items()}
        assert {r: int(v) for r, v in enumerate(getattr(got, k)) if v} == twice, k


def test_sixty_five_one_span_traces(ctx):
    """More one-span traces than a chunk's 64: heads only, everything is zero."""
    sp = build(3, [([t + 1], [0], [ERR], [t % 3]) for t in range(65)], start=100)
    got = _check(ctx, sp)
    assert not any(getattr(got, k).any() for k in got.TABLES)
    assert (got.grouped_spans, got.max_size, got.timed) == (0, 0, True)
    assert not got.span_group_size.any() and not got.span_after_error.any()


SIZES = (1, 2, 3, 4, 7, 8, 63, 64, 127, 128)
BUCKETS = [1, 2, 2, 1, 0, 1, 2, 1]      # of SIZES: 1 | 2, 3 | 4, 7 | 8 | - | 63 | 64, 127 | 128


def test_group_sizes_at_the_bucket_borders(ctx, monkeypatch, capfd):
    """One star per size on the row 0 -> 1 (chunks), and the same ten groups
    under one root on ten callees (407 spans: the long-trace kernel)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = build(2, [star(n + 1, 1, first_id=1000 * (k + 1)) for k, n in enumerate(SIZES)])
    got = _check(ctx, sp)
    assert ", 0 long traces" in capfd.readouterr().err
    assert got.size_hist[1].tolist() == BUCKETS and int(got.size_hist.sum()) == len(SIZES)
    assert got.size_max[1] == 128 and got.repeated[1] == 9 and got.groups[1] == 10
    ids = np.arange(1, 2 + sum(SIZES), dtype=np.uint64)
    pid = np.r_[np.uint64(0), np.full(sum(SIZES), 1, np.uint64)]
    svc = np.r_[0, np.repeat(np.arange(1, 11), SIZES)]
    order = np.r_[0, 1 + np.random.default_rng(1).permutation(sum(SIZES))]
    sp = build(11, [(ids, pid[order], np.zeros(ids.shape[0]), svc[order])])
    got = _check(ctx, sp)
    assert ", 1 long traces" in capfd.readouterr().err
    assert got.size_hist.sum(axis=0).tolist() == BUCKETS
    assert got.size_max[1:11].tolist() == list(SIZES)


@pytest.mark.parametrize("L_", [256, 257])
def test_star_at_the_chunk_limit(ctx, L_, monkeypatch, capfd):
    """A star that fills the chunk — n = e = 255: both halves of the group word
    at their largest — and one span more (the long-trace kernel), every child
    flagged, between two small stars."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = build(2, [star(4, 1, 10), star(L_, 1, 100, flagged=True), star(3, 1, 5000)], start=7)
    got = _check(ctx, sp)
    assert f"call_repeats_kernel<forward>, {L_ - 256} long traces" in capfd.readouterr().err
    assert got.max_size == L_ - 1 and got.exhausted[1] == 1 and got.recovered[1] == 0
    assert (got.span_group_size[5:4 + L_] == L_ - 1).all()
    assert got.size_hist[1].tolist() == [0, 2, 0, 0, 0, 0, 0, 1]
    assert not got.after_error.any()            # equal starts: nothing follows the failure


# ------------------------------------------------------------------ scans
@pytest.mark.parametrize("S,unique,kernel", [(9, False, "forward"), (9, True, "bidir"),
                                             (24, True, "split")])
def test_the_three_scans(ctx, monkeypatch, capfd, S, unique, kernel):
    """The same random trees (unique ids, random ancestors, orphans,
    self-references, shuffled inside the traces, 30 % flags, traces of 1..256
    spans) not declared unique, declared unique with the scans from both ends
    forced on, and over 24 services (E = 624 rows: the split-word scan) with
    services 0 and 23 both called — untimed and timed."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    if unique:
        monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "1")
    rng = np.random.default_rng(300)
    lens = np.r_[rng.integers(100, 257, 30), rng.integers(1, 30, 60), [256]]
    rng.shuffle(lens)
    sp = _flagged_tree(rng, lens, S=9, self_ref=0.02)
    if S == 24:     # the same trees over more services: 0 -> 0, 8 -> 23, others as they are
        sp.services = [f"svc{i:02d}" for i in range(24)]
        sp.svc = np.where(sp.svc == 8, 23, sp.svc).astype(np.uint16)
    if unique:
        assert sp.check_unique_ids()
    ref = repeats_ref(sp)
    callees = {c for _, c in ref.members}
    assert {0, S - 1} <= callees and ref.max_size >= 3
    got = _check(ctx, sp, ref=ref)
    assert f"call_repeats_kernel<{kernel}>, 0 long traces" in capfd.readouterr().err
    assert min(int(getattr(got, k).sum()) for k in got.TABLES if k != "after_error") > 0
    got = _check(ctx, _timed(sp, rng))
    assert f"call_repeats_kernel<{kernel}>, 0 long traces" in capfd.readouterr().err
    assert got.timed and int(got.after_error.sum()) > 0


def test_wide_table_in_the_sparse_counters(ctx, monkeypatch, capfd):
    """S = 64 (E = 4,224): the dense LDS counters do not fit, so every sum goes
    through the sparse table, and 64 random services over full chunks and a
    3,000-span trace give a workgroup more words than the table has slots: the
    adds that find none go to the global words.  The same tables."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(5)
    sp = _flagged_tree(rng, [256] * 8 + [3000], S=64)
    ref = repeats_ref(sp)
    assert int((ref.groups > 0).sum()) > 1024
    _check(ctx, _timed(sp, rng))
    assert ", 1 long traces" in capfd.readouterr().err


def test_large_groups_on_a_mid_sized_table(ctx, monkeypatch, capfd):
    """S = 32 (E = 1,088, dense counters) with three callees: groups of four
    and more reach the histogram's sparse counters, in chunks and long traces."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(6)
    sp = _flagged_tree(rng, np.r_[rng.integers(1, 200, 40), [300, 700]], S=3)
    sp.services = [f"svc{i:02d}" for i in range(32)]
    sp.svc = (sp.svc.astype(np.int64) * 15).astype(np.uint16)        # callees 0, 15, 30
    got = _check(ctx, _timed(sp, rng))
    assert ", 2 long traces" in capfd.readouterr().err
    assert int(got.size_hist[:, 2:].sum()) > 0 and got.max_size >= 4


# ------------------------------------------------------------------ long traces
def test_duplicated_ids_at_window_and_block_borders(ctx, monkeypatch, capfd):
    """test_gpu_self_time.window_border_case: the children of a duplicated id
    join the first carrier's groups across the lookup's window and block
    borders (traces of 4,097 and 2,049 spans)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, want = window_border_case()
    got = _check(ctx, sp)
    assert "call_repeats_kernel<forward>, 3 long traces" in capfd.readouterr().err
    ref = repeats_ref(sp)
    for child, parent in want.items():
        assert child in ref.members[(parent, int(sp.svc[child]))]
    assert got.max_size >= 2


def test_long_and_short_traces_mixed(ctx, monkeypatch, capfd):
    """2,049 and 4,097 spans: one past the window and the block of big_parents."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(22)
    lens = np.r_[rng.integers(1, 60, 300), [257, 256, 2049, 4097]]
    rng.shuffle(lens)
    sp = _flagged_tree(rng, lens)
    _check(ctx, sp)
    assert ", 3 long traces" in capfd.readouterr().err
    got = _check(ctx, _timed(sp, rng))
    assert got.timed and int(got.after_error.sum()) > 0


def test_chain_of_5000_spans(ctx):
    """Every group has one member: the hash table is full of singletons."""
    ids = np.arange(1, 5001, dtype=np.uint64)
    sp = build(9, [(ids, np.r_[np.uint64(0), ids[:-1]], np.arange(5000) % 3 == 0,
                    np.arange(5000) % 9)])
    got = _check(ctx, sp)
    assert int(got.groups.sum()) == 4999 and not got.repeats.any() and got.max_size == 1
    assert int(got.size_hist[:, 0].sum()) == 4999


def test_star_of_5000_spans_on_two_callees(ctx):
    got = _check(ctx, build(3, [star(5000, 2)]))
    assert got.groups[1] == 1 and got.groups[2] == 1
    assert got.size_max[1:3].tolist() == [2500, 2499] and got.max_size == 2500


def test_star_of_66000_flagged_children(ctx):
    """One group of more than 2^16 members, every one flagged: the long-trace
    counts are not packed in 16 bits."""
    n = 66000
    got = _check(ctx, build(2, [star(n + 1, 1, flagged=True)]))
    assert n > 1 << 16 and got.max_size == n and got.repeats[1] == n - 1
    assert got.exhausted[1] == 1 and got.size_hist[1, 7] == 1
    assert (got.span_group_size[1:] == n).all()


def test_one_shuffled_trace_of_5000_spans(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(21)
    sp = _timed(_flagged_tree(rng, [5000], 0.4, S=4), rng, hi=50)
    got = _check(ctx, sp)
    assert "call_repeats_kernel<forward>, 1 long traces" in capfd.readouterr().err
    assert got.max_size >= 3 and int(got.recovered.sum()) > 0 and int(got.after_error.sum()) > 0


# ------------------------------------------------------------------ time
def _group(starts, durs, flags):
    """A root and one group under it (service 1) with the given start times,
    durations and flags."""
    k = len(starts)
    ids = np.arange(1, k + 2, dtype=np.uint64)
    t = (ids, np.r_[np.uint64(0), np.full(k, 1, np.uint64)], [0, *flags], [0] + [1] * k)
    return build(2, [t], dur=np.array([1, *durs], np.uint32),
                 start=np.array([50, *starts], np.uint64))


def test_after_error_at_the_end_of_the_failure(ctx):
    """[fail 100-110, next at 110] counts the second member, a next at 109 not."""
    got = _check(ctx, _group([100, 110], [10, 5], [ERR, 0]))
    assert got.span_after_error.tolist() == [0, 0, 1] and got.after_error[1] == 1
    got = _check(ctx, _group([100, 109], [10, 5], [ERR, 0]))
    assert not got.span_after_error.any() and not got.after_error.any()
    assert got.recovered[1] == 1 and got.timed


def test_zero_duration_failure_occupies_one_microsecond(ctx):
    got = _check(ctx, _group([100, 100, 101], [0, 5, 5], [ERR, 0, 0]))
    assert got.span_after_error.tolist() == [0, 0, 0, 1] and got.after_error[1] == 1


def test_failure_without_a_start_time_is_ignored(ctx):
    got = _check(ctx, _group([0, 200, 300], [10, 5, 5], [ERR, 0, 0]))
    assert not got.after_error.any() and got.recovered[1] == 1
    # a second failure with a start time takes over; a member without one never counts
    got = _check(ctx, _group([0, 200, 300, 0], [10, 5, 5, 5], [ERR, ERR, 0, 0]))
    assert got.span_after_error.tolist() == [0, 0, 0, 1, 0]


def test_parallel_fan_out_counts_nothing(ctx):
    """Ten members with equal starts, one failed; then the same set without
    start times: timed 0, after_error zero, every other table unchanged."""
    sp = _group([500] * 10, [20] * 10, [0, 0, 0, ERR] + [0] * 6)
    got = _check(ctx, sp)
    assert not got.after_error.any() and got.recovered[1] == 1 and got.max_size == 10
    bare = anomod.SpanSet(list(sp.services), sp.trace_ptr, sp.trace_hash, sp.span_id,
                          sp.parent_span_id, sp.svc, sp.flags, sp.dur_us)
    untimed = _check(ctx, bare)
    assert not untimed.timed and not untimed.after_error.any()
    for k in got.TABLES:
        if k != "after_error":
            np.testing.assert_array_equal(getattr(untimed, k), getattr(got, k), err_msg=k)
    # the same for a set whose retries do follow their failures
    cur, _ = add_repeats(synth("SN", 300), FAULTS["SN"], 0.5, 3, np.random.default_rng(2))
    got = _check(ctx, cur)
    assert int(got.after_error.sum()) > 0
    bare = anomod.SpanSet(list(cur.services), cur.trace_ptr, cur.trace_hash, cur.span_id,
                          cur.parent_span_id, cur.svc, cur.flags, cur.dur_us, None,
                          cur.unique_ids)
    untimed = _check(ctx, bare)
    assert not untimed.timed and not untimed.after_error.any()
    for k in got.TABLES:
        if k != "after_error":
            np.testing.assert_array_equal(getattr(untimed, k), getattr(got, k), err_msg=k)


def test_start_times_at_the_top_of_the_range(ctx):
    """A failure whose end lies past 2^64 - 1 is followed by nothing."""
    top = 2**64 - 1
    got = _check(ctx, _group([top - 1, top, top], [5, 1, 1], [ERR, 0, 0]))
    assert not got.after_error.any()
    got = _check(ctx, _group([top - 1, top, top - 1], [1, 1, 1], [ERR, 0, 0]))
    assert got.span_after_error.tolist() == [0, 0, 1, 0]


# ------------------------------------------------------------------ synthetic sets
@pytest.mark.parametrize("topo,kernel", [("SN", "bidir"), ("TT", "split")])
def test_synthetic_parity(ctx, topo, kernel, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    base = synth(topo, 1500)
    sp, made = add_repeats(base, FAULTS[topo], 0.3, 4, np.random.default_rng(9))
    assert sp.unique_ids and made.shape[0] > 0
    sp.scan_order = 1       # the siblings stand right before the original: collector order
    got = _check(ctx, sp)
    assert f"call_repeats_kernel<{kernel}>, 0 long traces" in capfd.readouterr().err
    assert int(got.after_error.sum()) >= 3 * made.shape[0]


def test_long_topology(ctx, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=1, p_orphan_ppm=2000), 300)
    n_long = int((np.diff(sp.trace_ptr) > 256).sum())
    assert n_long > 0
    got = _check(ctx, sp)
    assert f", {n_long} long traces" in capfd.readouterr().err
    assert int(got.groups.sum()) > 0


def test_empty_and_one_span(ctx):
    got = _check(ctx, build(2, []))
    assert got.span_group_size.shape == (0,) and got.grouped_spans == 0 and not got.groups.any()
    got = _check(ctx, build(2, [([5], [0], [ERR], [1])], start=3))
    assert got.span_group_size.tolist() == [0] and got.timed and not got.groups.any()


# ------------------------------------------------------------------ arguments
def test_argument_handling(ctx):
    sp, _ = add_repeats(synth("SN", 200), FAULTS["SN"], 0.5, 3, np.random.default_rng(4))
    lib = anomod.lib()
    d = ctx.upload(sp)
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))
    try:
        S = sp.n_services
        cs = L.CallRepeatsC(S)
        assert lib.anomod_call_repeats_spans(ctx.handle, loose.handle, C.byref(cs)) == L.ESTATE
        assert b"not grouped" in lib.anomod_last_error(ctx.handle)
        cs = L.CallRepeatsC(S - 1)
        assert lib.anomod_call_repeats_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
        # NULL outputs are skipped: only repeats, size_max and span_after_error asked for
        ref = repeats_ref(sp)
        repeats = np.zeros(ref.repeats.shape[0], np.uint64)
        smax = np.zeros(ref.repeats.shape[0], np.uint32)
        after = np.zeros(sp.n_spans, np.uint8)
        cs = L.CallRepeatsC(S, 0, 0, 0, None, L.ptr(repeats, C.c_uint64), None, None, None, None,
                            None, None, L.ptr(smax, C.c_uint32), None, L.ptr(after, C.c_uint8))
        assert lib.anomod_call_repeats_spans(ctx.handle, d.handle, C.byref(cs)) == L.OK
        np.testing.assert_array_equal(repeats, ref.repeats)
        np.testing.assert_array_equal(smax, ref.size_max)
        np.testing.assert_array_equal(after, ref.span_after_error)
        assert (cs.grouped_spans, cs.max_size, cs.timed) == (ref.grouped_spans, ref.max_size, 1)
        cs = L.CallRepeatsC(S)      # no output at all
        assert lib.anomod_call_repeats_spans(ctx.handle, d.handle, C.byref(cs)) == L.OK
        assert cs.grouped_spans == ref.grouped_spans
    finally:
        loose.free()
        d.free()


def test_device_twin_hints_and_later_results_unchanged(ctx):
    """A device set gives what the host set gives; the set's hints, an
    aggregation and the self time are the same before and after the call (the
    order hint is probed by the self-time call first), and a second call
    equals the first."""
    sp, _ = add_repeats(synth("TT", 600), FAULTS["TT"], 0.5, 2, np.random.default_rng(6))
    ref = repeats_ref(sp)
    d = ctx.upload(sp)
    try:
        before, self_before = ctx.edge_aggregate(d), ctx.self_time(d)
        hints = d.hints
        first = _check(ctx, sp, dev=d, ref=ref)
        assert d.hints == hints
        assert_repeats_equal(ctx.call_repeats(sp, per_span=True), ref)
        after, self_after = ctx.edge_aggregate(d), ctx.self_time(d)
        again = ctx.call_repeats(d, per_span=True)
        assert d.hints == hints
        for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
            np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
            np.testing.assert_array_equal(getattr(self_after, k), getattr(self_before, k),
                                          err_msg=k)
        for k in first.TABLES + ("span_group_size", "span_after_error"):
            np.testing.assert_array_equal(getattr(again, k), getattr(first, k), err_msg=k)
    finally:
        d.free()


def test_device_grouped_set(ctx):
    """Upload ungrouped, group on the device (max_trace_len unknown)."""
    sp, _ = add_repeats(synth("SN", 500), FAULTS["SN"], 0.5, 3, np.random.default_rng(8))
    sp.start_us = None      # (an ungrouped upload carries no start column)
    order = np.random.default_rng(3).permutation(sp.n_spans)
    loose = sp.take(order, np.array([0, sp.n_spans], np.uint64))
    d = ctx.upload_ungrouped(loose)
    g = ctx.group(d)
    try:
        host = g.download()
        got = _check(ctx, host, dev=g)
        ref = repeats_ref(sp)
        assert_repeats_equal(got, ref, per_span=False)
    finally:
        g.free()
        d.free()


# ------------------------------------------------------------------ the ranking
def test_repeat_shift_through_features(ctx):
    fault = "home-timeline-service"
    base = synth("SN", 3000)
    cur, made = add_repeats(base, fault, 0.5, 3, np.random.default_rng(12))
    c = base.services.index(fault)
    e_base, e_cur = Experiment("base", base), Experiment("cur", cur, label=fault)
    fb = anomod.features(e_base, ctx, repeats=True)
    assert "repeat_shift" not in fb.params["components"]     # without a baseline: no term
    np.testing.assert_array_equal(fb.service_scores, anomod.features(e_base, ctx).service_scores)
    on = anomod.features(e_cur, ctx, baseline=fb, repeats=True)
    off = anomod.features(e_cur, ctx, baseline=fb)
    assert_repeats_equal(on.repeats, repeats_ref(cur), per_span=False)
    shift = on.params["components"]["repeat_shift"]
    print("repeat_shift:", dict(zip(base.services, shift.tolist())))
    assert shift[c] > 0 and len(shift) == 12 and (np.delete(shift, c) == 0.0).all()
    np.testing.assert_array_equal(on.service_scores, off.service_scores + 0.25 * _squash(shift))
    assert on.params["components"]["amplification"][c] > 0
    assert on.params["components"]["retry_rate"][c] > 0
    rec = on.repeats.per_service("recovered")[c] - fb.repeats.per_service("recovered")[c]
    assert rec == made.shape[0] and fb.repeats.per_service("recovered")[c] == 0
    assert on.repeats.per_service("recovered")[c] == made.shape[0]


def test_default_unchanged(ctx):
    """With the flag off, every field of Features is what a call without the
    flag gives."""
    e_base = anomod.load_experiment(anomod.SynthSpec("SN", seed=3), n_traces=400)
    exp = anomod.load_experiment(anomod.SynthSpec("SN", seed=4, fault_service=FAULTS["SN"]),
                                 n_traces=400)
    fb = anomod.features(e_base, ctx)
    a = anomod.features(exp, ctx, baseline=fb)
    b = anomod.features(exp, ctx, baseline=fb, repeats=False)
    assert a.repeats is None and b.repeats is None
    np.testing.assert_array_equal(a.service_scores, b.service_scores)
    assert a.params.keys() == b.params.keys()
    assert set(a.params["components"]) == set(b.params["components"]) == \
        {"error_rate", "latency", "metric"}
    for k, v in a.params["components"].items():
        np.testing.assert_array_equal(v, b.params["components"][k])
    assert {k: v for k, v in a.params.items() if k != "components"} == \
        {k: v for k, v in b.params.items() if k != "components"}
    for name in anomod.Features.__dataclass_fields__:
        x, y = getattr(a, name), getattr(b, name)
        if name in ("params", "service_scores"):
            continue
        if name == "edges":
            for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
                np.testing.assert_array_equal(getattr(x, k), getattr(y, k), err_msg=k)
        elif isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y, err_msg=name)
        else:
            assert x == y, name

"""Call transit, host side (no GPU): the C entry point's export and NULL
handling, the reference model (tests/call_transit_ref.py) on the hand-made
trace and on edge values, its invariants on random trees, the transit_set input
helper, the helpers of CallTransit and the CLI's document, the score term of
features(transit=True) on a stand-in context, and the CLI flag."""
import ctypes as C
import inspect
import json
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import _squash, _transit_shift
from conftest import PKG_DIR

from call_transit_ref import (CALL, EARLY, LATE, PAIRED, TIMED, U32_MAX, U64_MAX, as_call_transit,
                              assert_invariants, build, check_hand_made, hand_made, transit_ref,
                              transit_set)
from call_repeats_ref import add_repeats
from critical_path_ref import random_starts
from self_time_ref import parents_ref
from test_call_repeats_host import HostContext, RepeatsContext
from test_gpu_self_time import _random_tree


# ------------------------------------------------------------------ surface
def test_library_exports_the_entry_point():
    assert "anomod_call_transit_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    cs = L.CallTransitC(1)
    assert lib.anomod_call_transit_spans(None, None, C.byref(cs)) == L.EINVAL
    assert b"anomod_call_transit_spans" in lib.anomod_last_error(None)


def test_python_surface():
    p = inspect.signature(anomod.features).parameters
    assert "transit" in p and p["transit"].default is False
    assert list(p)[-1] == "transit"                       # after every earlier option
    assert "transit" in anomod.Features.__dataclass_fields__
    q = inspect.signature(anomod.Context.call_transit).parameters
    assert list(q)[1:] == ["spans", "with_hist", "per_span"]
    assert q["with_hist"].default is True and q["per_span"].default is False
    assert [f for f, _ in L.CallTransitC._fields_] == [
        "n_services", "calls", "paired", "request", "response", "untimed", "early", "late",
        "early_us", "late_us", "span_req_us", "span_resp_us", "span_state"]
    assert (L.TRANSIT_CALL, L.TRANSIT_PAIRED, L.TRANSIT_TIMED, L.TRANSIT_EARLY,
            L.TRANSIT_LATE) == (CALL, PAIRED, TIMED, EARLY, LATE) == (1, 2, 4, 8, 16)
    assert anomod.CallTransit is anomod.spans.CallTransit and "CallTransit" in anomod.__all__


def test_cli_lists_the_flag():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--transit" in r.stdout


# ------------------------------------------------------------------ the model
def test_reference_on_the_hand_made_trace():
    sp = hand_made()
    par = parents_ref(sp)
    assert par.tolist() == [-1, 0, 0, 1, 2, 3, -1, -1]
    r = transit_ref(sp, par)
    check_hand_made(r)
    assert_invariants(r, sp, par)
    both = anomod.SpanSet.concat([sp, sp])       # equal ids in two traces stay apart
    r2 = transit_ref(both)
    check_hand_made(r2, 2)
    assert_invariants(r2, both)


def _pair(ps, pd, cs, cd, flags=0):
    """A root client span (service 0) and its one child (service 1): row 1."""
    return build(2, [[(1, 0, 0, ps, pd), (2, 1, 1, cs, cd, flags)]])


def test_reference_equal_starts_and_equal_ends():
    r = transit_ref(_pair(500, 100, 500, 100, anomod.FLAG_ERROR))
    assert r.span_state.tolist() == [0, CALL | PAIRED | TIMED]
    for t in (r.request, r.response):
        assert (t["count"][1], t["errors"][1], t["sum_us"][1], t["min_us"][1], t["max_us"][1]) == \
            (1, 1, 0, 0, 0)
        assert t["hist"][1, 0] == 1 and t["p99_us"][1] == 0.0
    assert not r.early.any() and not r.late.any()
    # one microsecond to either side: early / late by 1, no record
    r = transit_ref(_pair(500, 100, 499, 102))
    assert r.span_state.tolist() == [0, CALL | PAIRED | TIMED | EARLY | LATE]
    assert (r.early[1], r.early_us[1], r.late[1], r.late_us[1]) == (1, 1, 1, 1)
    assert not r.request["count"].any() and not r.response["count"].any()


@pytest.mark.parametrize("gap", [U32_MAX, U32_MAX + 1])
def test_reference_clamps_gaps_at_the_u32_limit(gap):
    """Request and early gaps, response and late gaps of 2^32 - 1 and 2^32:
    both read 2^32 - 1."""
    s = 10
    r = transit_ref(_pair(s, U32_MAX, s + gap, 0))        # request gap; the child ends late
    assert r.span_req_us.tolist() == [0, U32_MAX] and r.request["max_us"][1] == U32_MAX
    assert r.request["sum_us"][1] == U32_MAX
    assert (r.late[1], r.late_us[1]) == (gap > U32_MAX, gap - U32_MAX)   # equal ends are not late
    r = transit_ref(_pair(s + gap, 5, s, 1))              # early by gap, ends before the parent
    assert (r.early[1], r.early_us[1]) == (1, U32_MAX) and not r.request["count"].any()
    assert r.span_resp_us.tolist() == [0, U32_MAX] and r.response["count"][1] == 1
    r = transit_ref(_pair(s, 0, s, 0))
    assert r.span_resp_us.tolist() == [0, 0]
    r = transit_ref(_pair(s + gap + 7, 0, s, 7))          # child [s, s + 7), parent at s + gap + 7
    assert r.span_resp_us.tolist() == [0, U32_MAX] and r.early_us[1] == U32_MAX
    r = transit_ref(_pair(s, 1, s + 1 + gap - 4, 4))      # the child ends gap after the parent
    assert (r.late[1], r.late_us[1]) == (1, U32_MAX)


def test_reference_saturates_ends_near_the_top_of_the_range():
    top = U64_MAX
    # both ends saturate at 2^64 - 1: equal ends, a response of 0
    r = transit_ref(_pair(top - 10, 100, top - 5, 100))
    assert r.span_state.tolist() == [0, CALL | PAIRED | TIMED]
    assert r.span_req_us.tolist() == [0, 5] and r.span_resp_us.tolist() == [0, 0]
    assert r.response["count"][1] == 1 and r.response["max_us"][1] == 0
    # the child's end saturates, the parent's does not: late by what is left below the top
    r = transit_ref(_pair(top - 10, 4, top - 5, 100))
    assert r.span_state.tolist() == [0, CALL | PAIRED | TIMED | LATE] and r.late_us[1] == 6
    # the parent's saturates, the child's does not
    r = transit_ref(_pair(top - 10, 100, top - 8, 3))
    assert r.span_resp_us.tolist() == [0, 5]


def test_reference_duplicated_parent_id_counts_on_the_first_carrier():
    """Two carriers of id 5 with one child each: both children count on the
    first carrier, so it has two kids and neither call is paired; the second
    carrier has none."""
    rows = [(1, 0, 0, 100, 100), (5, 1, 0, 110, 20), (5, 1, 0, 140, 20), (6, 5, 1, 112, 5),
            (7, 5, 1, 142, 5)]
    sp = build(2, [rows])
    par = parents_ref(sp)
    assert par.tolist() == [-1, 0, 0, 1, 1]
    r = transit_ref(sp, par)
    assert (r.calls, r.paired) == (4, 0) and r.span_state.tolist() == [0, CALL, CALL, CALL, CALL]
    assert not r.request["count"].any() and not r.untimed.any()
    assert_invariants(r, sp, par)
    # with one child only, the pair is the first carrier's, whichever copy is nearer
    sp = build(2, [rows[:3] + rows[4:]])
    r = transit_ref(sp)
    assert r.paired == 1 and r.span_req_us.tolist() == [0, 0, 0, 32]


def _holes(sp, rng, share=0.05):
    """sp with a share of its start times zeroed (no time recorded)."""
    sp.start_us = np.where(rng.random(sp.n_spans) < share, 0, sp.start_us).astype(np.uint64)
    return sp


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_invariants_on_random_trees(seed):
    rng = np.random.default_rng(seed)
    tree = _random_tree(rng, np.r_[rng.integers(1, 60, 80), [300]], S=5, self_ref=0.03)
    sp = _holes(random_starts(tree, seed), rng)
    par = parents_ref(sp)
    r = transit_ref(sp, par)
    assert_invariants(r, sp, par)
    assert 0 < r.paired < r.calls < sp.n_spans
    for k in ("early", "late", "untimed"):
        assert int(getattr(r, k).sum()) > 0, k
    assert int(r.request["count"].sum()) > 0 and int(r.response["count"].sum()) > 0
    both = (r.span_state & (EARLY | LATE)) == 0
    assert int((both & ((r.span_state & TIMED) != 0)).sum()) > 0     # both records
    assert int(r.request["errors"].sum()) > 0


def test_transit_set_moves_only_the_slow_pair():
    base = transit_set(300, 7)
    cur = transit_set(300, 7, slow="b", d_req=20_000, d_resp=5_000, abandon=0.25)
    rb, rc = transit_ref(base), transit_ref(cur)
    assert_invariants(rb, base)
    assert_invariants(rc, cur)
    S = 4
    a, b, c, front = 0, 1, 2, 3
    assert (rb.calls, rb.paired) == (6 * 300, 4 * 300)         # a's two client spans are unpaired
    assert not rb.early.any() and not rb.late.any() and not rb.untimed.any()
    rows = {"ab": a * S + b, "ac": a * S + c, "fa": front * S + a, "ff": front * S + front}
    assert sorted(np.flatnonzero(rb.request["count"]).tolist()) == sorted(rows.values())
    for t in ("request", "response"):
        lo, hi = (150, 250) if t == "request" else (100, 200)
        tb, tc = getattr(rb, t), getattr(rc, t)
        for k in ("ab", "ac", "fa"):
            assert lo <= tb["min_us"][rows[k]] and tb["max_us"][rows[k]] <= hi
        for k in ("ac", "fa", "ff"):                            # no other pair's gaps change
            for f in ("count", "sum_us", "min_us", "max_us"):
                assert tc[f][rows[k]] == tb[f][rows[k]], (t, k, f)
    d = rc.request["sum_us"][rows["ab"]] - rb.request["sum_us"][rows["ab"]]
    assert d == 300 * 20_000
    late = int(rc.late[rows["ab"]])
    assert 0 < late < 150 and rc.late_us[rows["ab"]] == late and rc.late.sum() == late
    kept = rc.response["count"][rows["ab"]]
    assert kept == 300 - late and rc.response["min_us"][rows["ab"]] >= 5_100
    # b's own span is unchanged: its inclusive duration does not move
    np.testing.assert_array_equal(cur.dur_us[cur.svc == b], base.dur_us[base.svc == b])
    with pytest.raises(AssertionError):
        transit_set(3, 1, slow="a")


# ------------------------------------------------------------------ helpers
def test_call_transit_helpers():
    tr = anomod.CallTransit.empty(["a", "b"], with_hist=False, n_spans=3)
    E = 8
    assert all(getattr(tr, k).shape == (E,) and getattr(tr, k).dtype == np.uint64
               for k in tr.TABLES)
    assert tr.request.hist is None and tr.response.hist is None and tr.request is not tr.response
    assert (tr.span_req_us.dtype, tr.span_resp_us.dtype, tr.span_state.dtype) == \
        (np.uint32, np.uint32, np.uint8) and tr.span_state.shape == (3,)
    plain = anomod.CallTransit.empty(["a", "b"])
    assert plain.request.hist.shape == (E, anomod.HIST_BINS) and plain.span_state is None
    # rows p * 2 + c: a -> a 0, a -> b 1, b -> a 2, b -> b 3
    tr.request.count[[0, 1, 2]] = [50, 6, 30]
    tr.request.sum_us[[0, 1, 2]] = [500, 600, 900]
    tr.request.p99_us[[0, 1, 2]] = [9000.0, 150.0, 40.0]
    tr.response.count[[0, 1, 2]] = [50, 5, 40]
    tr.response.sum_us[[1, 2]] = [100, 400]
    tr.response.p99_us[[1, 2]] = [30.0, 20.0]
    tr.early[[0, 1, 2]] = [7, 2, 10]
    tr.late[[1]] = [3]
    tr.untimed[[1, 3]] = [1, 4]
    np.testing.assert_array_equal(tr.paired_rows(), [57, 9, 40, 4, 0, 0, 0, 0])
    # the same-service rows (a -> a, b -> b) are left out
    np.testing.assert_array_equal(tr.per_service("early"), [10, 2])
    np.testing.assert_array_equal(tr.per_service("untimed"), [0, 1])
    np.testing.assert_array_equal(tr.per_service("paired"), [40, 9])
    np.testing.assert_array_equal(tr.per_service("request.count"), [30, 6])
    np.testing.assert_array_equal(tr.per_service("response.sum_us"), [400, 100])
    with pytest.raises(ValueError):
        tr.per_service("request.p99_us")
    with pytest.raises(ValueError):
        tr.per_service("calls")
    np.testing.assert_array_equal(tr.skew_rate(), [10 / 40, 2 / 8])
    np.testing.assert_array_equal(tr.abandoned_rate(), [0.0, 3 / 8])
    np.testing.assert_array_equal(anomod.CallTransit.empty(["a", "b"]).skew_rate(), [0.0, 0.0])
    np.testing.assert_array_equal(anomod.CallTransit.empty(["a"]).abandoned_rate(), [0.0])
    from anomod.__main__ import call_transit_doc
    tr.calls, tr.paired = 200, 110
    doc = call_transit_doc(tr)
    assert (doc["calls"], doc["paired"]) == (200, 110) and list(doc["services"]) == ["a", "b"]
    assert doc["services"]["b"] == {
        "paired": 9, "request": {"records": 6, "mean_us": 100.0, "p99_us": 150.0},
        "response": {"records": 5, "mean_us": 20.0, "p99_us": 30.0},
        "early": 2, "late": 3, "untimed": 1}
    assert doc["services"]["a"]["request"] == {"records": 30, "mean_us": 30.0, "p99_us": 40.0}
    empty = call_transit_doc(anomod.CallTransit.empty(["a", "b"]))
    assert empty["services"]["a"]["request"] == {"records": 0, "mean_us": None, "p99_us": None}
    json.dumps(doc)
    json.dumps(empty)


def test_transit_shift_matches_rows_by_name():
    base = anomod.CallTransit.empty(["a", "b"])
    cur = anomod.CallTransit.empty(["b", "x", "a"])           # another order, one more service
    row = lambda p, c: p * 3 + c  # noqa: E731  (cur: b = 0, x = 1, a = 2)

    def put(t, r, count, p99):
        t.count[r], t.p99_us[r] = count, p99
    put(base.request, 1, 20, 100.0)                           # a -> b
    put(base.response, 1, 20, 50.0)
    put(base.request, 2, 20, 80.0)                            # b -> a
    put(base.request, 0, 20, 10.0)                            # a -> a: same service
    put(cur.request, row(2, 0), 10, 400.0)                    # a -> b request: 4 x
    put(cur.response, row(2, 0), 10, 400.0)                   # a -> b response: 8 x, the larger
    put(cur.request, row(0, 2), 10, 40.0)                     # b -> a: shrank, 0
    put(cur.request, row(1, 2), 50, 9000.0)                   # x -> a: no such row in the baseline
    put(cur.request, row(2, 2), 50, 9000.0)                   # a -> a: left out
    np.testing.assert_array_equal(_transit_shift(cur, base), [3.0, 0.0, 0.0])
    cur.response.count[row(2, 0)] = 9                         # below 10 records: the request alone
    np.testing.assert_array_equal(_transit_shift(cur, base), [2.0, 0.0, 0.0])
    base.request.p99_us[1] = 0.0                              # a baseline p99 of 0 compares nothing
    np.testing.assert_array_equal(_transit_shift(cur, base), [0.0, 0.0, 0.0])
    base.request.p99_us[1] = np.nan
    np.testing.assert_array_equal(_transit_shift(cur, base), [0.0, 0.0, 0.0])


# ------------------------------------------------------------------ features
class TransitContext(RepeatsContext):
    def call_transit(self, spans, with_hist=True, per_span=False):
        return as_call_transit(transit_ref(spans), spans.services, with_hist)


def test_features_transit_on_the_host():
    base = transit_set(200, 3)
    cur = transit_set(200, 3, slow="b", d_req=20_000, d_resp=5_000, abandon=0.25)
    b = 1
    e_base, e_cur = (anomod.Experiment(n, s, None, None, {}) for n, s in (("b", base), ("c", cur)))
    # a context that cannot compute the tables is an error: nothing falls back
    with pytest.raises(AttributeError, match="call_transit"):
        anomod.features(e_cur, HostContext(), transit=True)
    ctx = TransitContext()
    fb = anomod.features(e_base, ctx, transit=True)
    plain_b = anomod.features(e_base, ctx)
    assert fb.transit is not None and "transit_shift" not in fb.params["components"]
    np.testing.assert_array_equal(fb.service_scores, plain_b.service_scores)
    for k, v in plain_b.params["components"].items():
        np.testing.assert_array_equal(fb.params["components"][k], v)
    off = anomod.features(e_cur, ctx, baseline=fb)
    on = anomod.features(e_cur, ctx, baseline=fb, transit=True)
    assert off.transit is None and not {"abandoned_rate", "skew_rate", "transit_shift"} & \
        set(off.params["components"])
    comp = on.params["components"]
    shift = comp["transit_shift"]
    assert shift[b] > 0 and not np.delete(shift, b).any()
    np.testing.assert_array_equal(shift, _transit_shift(on.transit, fb.transit))
    np.testing.assert_array_equal(on.service_scores, off.service_scores + 0.25 * _squash(shift))
    assert comp["latency"][b] == 0.0                 # the callee's own duration did not move
    r = transit_ref(cur)
    want = r.late[b] / (r.response["count"][b] + r.late[b])      # row a -> b = 0 * 4 + 1
    assert comp["abandoned_rate"][b] == want > 0 and not np.delete(comp["abandoned_rate"], b).any()
    assert not comp["skew_rate"].any()
    # the term comes last in the sum: after the repeat term
    rep_cur, _ = add_repeats(cur, "b", 0.5, 3, np.random.default_rng(5), fail_first=False)
    e_rep = anomod.Experiment("r", rep_cur, None, None, {})
    fb2 = anomod.features(e_base, ctx, transit=True, repeats=True)
    both = anomod.features(e_rep, ctx, baseline=fb2, transit=True, repeats=True)
    only_rep = anomod.features(e_rep, ctx, baseline=fb2, repeats=True)
    assert both.params["components"]["repeat_shift"][b] > 0
    t_shift = both.params["components"]["transit_shift"]
    np.testing.assert_array_equal(both.service_scores,
                                  only_rep.service_scores + 0.25 * _squash(t_shift))
    # a baseline without the tables: the components, no term
    plain = anomod.features(e_cur, ctx, baseline=plain_b, transit=True)
    assert "transit_shift" not in plain.params["components"]
    assert "abandoned_rate" in plain.params["components"]
    np.testing.assert_array_equal(plain.service_scores,
                                  anomod.features(e_cur, ctx, baseline=plain_b).service_scores)


def test_features_transit_needs_start_times():
    sp = transit_set(5, 1)
    sp.start_us = None
    exp = anomod.Experiment("x", sp, None, None, {})

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError(f"features() called ctx.{name} before checking the option")
    with pytest.raises(ValueError, match="start_us"):
        anomod.features(exp, Untouched(), transit=True)
    with pytest.raises(ValueError, match="start_us"):
        anomod.Context.call_transit(object(), sp)

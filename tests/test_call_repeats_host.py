"""Call repeats, host side (no GPU): the C entry point's export and NULL
handling, the reference model (tests/call_repeats_ref.py) on a hand-made trace,
against a brute-force restatement on random trees and its invariants on
synthetic sets, the add_repeats input helper, the helpers of CallRepeats, the
score terms of features(repeats=True) on a stand-in context, and the CLI flag."""
import ctypes as C
import inspect
import json
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import _repeat_components, _repeat_shift, _squash
from anomod.spans import EdgeTable
from conftest import PKG_DIR
from oracle import native

from call_repeats_ref import (TABLES, add_repeats, assert_invariants, bucket, build, group_members,
                              hand_made, repeats_ref, star)
from self_time_ref import NO_PARENT, parents_ref
from test_gpu_self_time import _random_tree
from test_self_time_host import FAULTS, synth

ERR = anomod.FLAG_ERROR


# ------------------------------------------------------------------ surface
def test_library_exports_the_entry_point():
    assert "anomod_call_repeats_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    cs = L.CallRepeatsC(1)
    assert lib.anomod_call_repeats_spans(None, None, C.byref(cs)) == L.EINVAL
    assert b"anomod_call_repeats_spans" in lib.anomod_last_error(None)


def test_python_surface():
    p = inspect.signature(anomod.features).parameters
    assert "repeats" in p and p["repeats"].default is False
    assert "repeats" in anomod.Features.__dataclass_fields__
    q = inspect.signature(anomod.Context.call_repeats).parameters
    assert list(q)[1:] == ["spans", "per_span"] and q["per_span"].default is False
    assert [f for f, _ in L.CallRepeatsC._fields_][:4] == ["n_services", "max_size", "timed",
                                                           "grouped_spans"]


def test_cli_lists_the_flag():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--repeats" in r.stdout


# ------------------------------------------------------------------ the model
def test_reference_on_the_hand_made_trace():
    sp, size, want = hand_made()
    par = parents_ref(sp)
    assert par.tolist() == [-1, 0, 0, 0, 1, -1, -1, 3, 3, 7, 7, 7]
    r = repeats_ref(sp, par)
    assert r.span_group_size.tolist() == size
    E = r.groups.shape[0]
    for k, rows in want.items():
        dense = np.zeros(E, np.int64)
        dense[list(rows)] = list(rows.values())
        np.testing.assert_array_equal(getattr(r, k), dense, err_msg=k)
    assert (r.grouped_spans, r.max_size, r.timed) == (9, 2, False)
    assert not r.after_error.any() and not r.span_after_error.any()
    assert_invariants(r, sp, par)


def _brute_force(sp, par):
    """The definition once more, without a dict: a span with a parent counts
    the spans of its trace with the same parent and service (O(n^2) per
    trace); the group is taken at its least member."""
    S = sp.n_services
    E = (S + 2) * S
    tab = {k: np.zeros(E, np.int64) for k in TABLES if k != "size_hist"}
    hist = np.zeros((E, 8), np.int64)
    size = np.zeros(sp.n_spans, np.int64)
    after = np.zeros(sp.n_spans, np.int64)
    err = (sp.flags & ERR) != 0
    ptr = sp.trace_ptr.tolist()
    for t in range(sp.n_traces):
        for i in range(ptr[t], ptr[t + 1]):
            if par[i] == NO_PARENT:
                continue
            mem = [m for m in range(ptr[t], ptr[t + 1])
                   if par[m] == par[i] and sp.svc[m] == sp.svc[i]]
            n, e = len(mem), int(err[mem].sum())
            size[i] = n
            if sp.start_us is not None:
                ends = [int(sp.start_us[m]) + max(int(sp.dur_us[m]), 1) for m in mem
                        if err[m] and sp.start_us[m] != 0]
                after[i] = bool(ends) and sp.start_us[i] != 0 and int(sp.start_us[i]) >= min(ends)
            r = int(sp.svc[par[i]]) * S + int(sp.svc[i])
            tab["after_error"][r] += after[i]
            if mem[0] != i:
                continue
            tab["groups"][r] += 1
            tab["repeats"][r] += n - 1
            tab["repeated"][r] += n >= 2
            tab["retried"][r] += n >= 2 and e >= 1
            tab["recovered"][r] += n >= 2 and 1 <= e < n
            tab["exhausted"][r] += n >= 2 and e == n
            tab["size_max"][r] = max(tab["size_max"][r], n)
            hist[r, bucket(n)] += 1
    return tab, hist, size, after


@pytest.mark.parametrize("timed", [False, True])
def test_reference_equals_the_brute_force_restatement(timed):
    rng = np.random.default_rng(11)
    sp = _random_tree(rng, np.r_[rng.integers(1, 40, 30), [120]], S=4, self_ref=0.03)
    sp.flags = ((rng.random(sp.n_spans) < 0.3) * ERR).astype(np.uint16)
    if timed:    # few distinct values: zeros, ties and zero durations all occur
        sp.start_us = rng.integers(0, 6, sp.n_spans).astype(np.uint64)
        sp.dur_us = rng.integers(0, 3, sp.n_spans).astype(np.uint32)
    par = parents_ref(sp)
    r = repeats_ref(sp, par)
    tab, hist, size, after = _brute_force(sp, par)
    for k, v in tab.items():
        np.testing.assert_array_equal(getattr(r, k), v, err_msg=k)
    np.testing.assert_array_equal(r.size_hist, hist)
    np.testing.assert_array_equal(r.span_group_size, size)
    np.testing.assert_array_equal(r.span_after_error, after)
    assert r.timed == timed and r.max_size >= 3 and int(r.retried.sum()) > 0
    assert bool(r.after_error.any()) == timed
    assert_invariants(r, sp, par)


@pytest.mark.parametrize("topo", ["SN", "TT"])
def test_reference_invariants_on_synthetic_sets(topo):
    sp = synth(topo, 1500)
    par = parents_ref(sp)
    r = repeats_ref(sp, par)
    assert_invariants(r, sp, par)
    S = sp.n_services
    # no self-reference in these sets: the edge table's count on the first S * S rows
    np.testing.assert_array_equal((r.groups + r.repeats)[:S * S],
                                  native.edge_aggregate(sp)["count"][:S * S])
    assert int(r.groups.sum()) > 0 and not r.timed and not r.after_error.any()


def test_star_helper():
    sp = build(4, [star(10, 3, flagged=True)])
    r = repeats_ref(sp)
    assert sorted(len(m) for m in r.members.values()) == [3, 3, 3]
    assert r.exhausted.tolist()[:4] == [0, 1, 1, 1] and int(r.groups.sum()) == 3


@pytest.mark.parametrize("fail_first", [True, False])
def test_add_repeats_yields_the_groups_it_claims(fail_first):
    base = synth("SN", 400)
    c = base.services.index(FAULTS["SN"])
    before = group_members(base)
    sp, made = add_repeats(base, FAULTS["SN"], 0.5, 3, np.random.default_rng(3), fail_first)
    after = group_members(sp)
    n_svc = sum(1 for (_, s) in before if s == c)
    assert 0 < made.shape[0] < n_svc and len(after) == len(before)    # no group made or lost
    assert sp.n_spans == base.n_spans + 2 * made.shape[0] and sp.n_traces == base.n_traces
    assert sp.check_unique_ids()
    grown = {key: m for key, m in after.items() if m[0] in set(made.tolist())}
    assert len(grown) == made.shape[0] and all(s == c for _, s in grown)
    # size by size: every drawn group gained two members, every other none
    drawn = set(made.tolist())
    undone = sorted(len(m) - (2 if m[0] in drawn else 0) for m in after.values())
    assert undone == sorted(len(m) for m in before.values())
    assert all(len(m) >= 3 for m in grown.values())
    r = repeats_ref(sp)
    r0 = repeats_ref(base)
    rec = lambda x: int(x.recovered.reshape(-1, sp.n_services)[:, c].sum())  # noqa: E731
    if fail_first:
        assert sp.start_us is not None and r.timed
        assert rec(r) == rec(r0) + made.shape[0]
        # the attempts lie end to end: both later attempts follow the first failure
        for m in grown.values():
            lead = m[:3]                                   # the drawn run: its three attempts
            assert (sp.flags[lead] & ERR).tolist() == [1, 1, 0]
            assert r.span_after_error[lead].tolist() == [0, 1, 1]
            d = max(int(sp.dur_us[lead[0]]), 1)
            assert np.diff(sp.start_us[lead].astype(np.int64)).tolist() == [d, d]
    else:
        assert sp.start_us is None and rec(r) == rec(r0)
        assert int(r.repeats.sum()) == int(r0.repeats.sum()) + 2 * made.shape[0]
        for m in grown.values():
            assert len(set(sp.flags[m[:3]].tolist())) == 1


# ------------------------------------------------------------------ helpers
def test_call_repeats_helpers():
    cr = anomod.CallRepeats.empty(["a", "b"])
    E = 8
    assert all(getattr(cr, k).shape[0] == E for k in cr.TABLES) and cr.span_group_size is None
    assert cr.size_hist.shape == (E, 8) and cr.size_max.dtype == np.uint32 and not cr.timed
    cr.groups[[0, 1, 2]] = [10, 4, 5]          # rows p * 2 + c: a -> a, a -> b, b -> a
    cr.repeats[[0, 1]] = [5, 8]
    cr.retried[[0, 1]] = [2, 1]
    cr.size_max[[0, 1, 2]] = [3, 9, 1]
    np.testing.assert_array_equal(cr.amplification(), [1.5, 3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    np.testing.assert_array_equal(cr.per_service("groups"), [15, 4])
    np.testing.assert_array_equal(cr.per_service("size_max"), [3, 9])
    assert cr.per_service("size_hist").shape == (2, 8)
    amp, rate = _repeat_components(cr)
    np.testing.assert_array_equal(amp, [0.5, 0.0])        # a -> b has fewer than 10 groups
    np.testing.assert_array_equal(rate, [2 / 15, 1 / 4])
    with_rows = anomod.CallRepeats.empty(["b", "a", "x"], n_spans=3)
    assert with_rows.span_group_size.shape == (3,) and with_rows.span_after_error.dtype == np.uint8
    from anomod.__main__ import call_repeats_doc
    cr.grouped_spans, cr.max_size, cr.timed = 32, 9, True
    doc = call_repeats_doc(cr)
    assert doc["timed"] is True and doc["max_size"] == 9 and doc["grouped_spans"] == 32
    assert doc["services"]["a"] == {"groups": 15, "repeats": 5, "retried": 2, "recovered": 0,
                                    "exhausted": 0, "after_error": 0, "size_max": 3}
    json.dumps(doc)


def test_repeat_shift_matches_rows_by_name():
    base = anomod.CallRepeats.empty(["a", "b"])
    cur = anomod.CallRepeats.empty(["b", "x", "a"])          # another order, one more service
    base.groups[1], base.repeats[1] = 20, 0                  # a -> b: 1.0
    base.groups[2], base.repeats[2] = 20, 20                 # b -> a: 2.0
    row = lambda p, c: p * 3 + c  # noqa: E731  (cur: b = 0, x = 1, a = 2)
    cur.groups[row(2, 0)], cur.repeats[row(2, 0)] = 10, 30   # a -> b: 4.0, grew 4 x
    cur.groups[row(0, 2)], cur.repeats[row(0, 2)] = 10, 0    # b -> a: 1.0, shrank: 0
    cur.groups[row(1, 2)], cur.repeats[row(1, 2)] = 50, 50   # x -> a: no such row in the baseline
    np.testing.assert_array_equal(_repeat_shift(cur, base), [2.0, 0.0, 0.0])
    cur.groups[row(2, 0)] = 9                                # below 10 groups: not compared
    cur.repeats[row(2, 0)] = 27
    np.testing.assert_array_equal(_repeat_shift(cur, base), [0.0, 0.0, 0.0])


# ------------------------------------------------------------------ features
class HostContext:
    """Stand-in for Context built on the CPU references: what features() calls."""

    def edge_aggregate(self, spans, with_hist=True):
        ref = native.finalize(native.edge_aggregate(spans))
        return EdgeTable(list(spans.services), ref["count"], ref["errors"], ref["sum_us"],
                         ref["min_us"], ref["max_us"], ref["p50_us"], ref["p99_us"],
                         ref["hist"] if with_hist else None)


class RepeatsContext(HostContext):
    def call_repeats(self, spans, per_span=False):
        r = repeats_ref(spans)
        return anomod.CallRepeats(list(spans.services), *(getattr(r, k) for k in TABLES),
                                  r.grouped_spans, r.max_size, r.timed)


def test_features_repeats_on_the_host():
    fault = FAULTS["SN"]
    base = synth("SN", 300)
    cur, made = add_repeats(base, fault, 0.5, 3, np.random.default_rng(5))
    c = base.services.index(fault)
    e_base, e_cur = (anomod.Experiment(n, s, None, None, {}) for n, s in (("b", base), ("c", cur)))
    # a context that cannot compute the table is an error: nothing falls back
    with pytest.raises(AttributeError, match="call_repeats"):
        anomod.features(e_cur, HostContext(), repeats=True)
    ctx = RepeatsContext()
    fb = anomod.features(e_base, ctx, repeats=True)
    assert fb.repeats is not None and "repeat_shift" not in fb.params["components"]
    np.testing.assert_array_equal(fb.service_scores, anomod.features(e_base, ctx).service_scores)
    off = anomod.features(e_cur, ctx, baseline=fb)
    on = anomod.features(e_cur, ctx, baseline=fb, repeats=True)
    assert off.repeats is None and not {"amplification", "retry_rate", "repeat_shift"} & \
        set(off.params["components"])
    comp = on.params["components"]
    shift = comp["repeat_shift"]
    assert shift[c] > 0 and not np.delete(shift, c).any()
    np.testing.assert_array_equal(on.service_scores, off.service_scores + 0.25 * _squash(shift))
    assert comp["amplification"][c] > 0 and comp["retry_rate"][c] > 0
    np.testing.assert_array_equal(shift, _repeat_shift(on.repeats, fb.repeats))
    # a baseline without the table: the components, no term
    plain = anomod.features(e_cur, ctx, baseline=anomod.features(e_base, ctx), repeats=True)
    assert "repeat_shift" not in plain.params["components"]
    np.testing.assert_array_equal(
        plain.service_scores,
        anomod.features(e_cur, ctx, baseline=anomod.features(e_base, ctx)).service_scores)

"""Critical path, host side (no GPU): the C entry point's export and NULL
handling, the features() flag and the CLI flag, the reference helper
(tests/critical_path_ref.py) on hand-made traces with hand-written results,
conservation on nested sets, and the evidence for the latency term on the
fan-out topology."""
import ctypes as C
import inspect
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import _latency_shift
from conftest import PKG_DIR
from oracle import native

from critical_path_ref import (FANOUT_SERVICES, HAND_CASES, cp_table_ref, critical_path_ref,
                               fanout_set, hand_set, nested_set, random_starts, select_literal)
from self_time_ref import (NO_PARENT, as_edge_table, parents_ref, self_table_ref)

# p_seq of nested_set per topology (start at 1/2; the non-degeneracy test
# below is the condition on it)
P_SEQ = {"SN": 0.5, "TT": 0.5, "LONG": 0.5}


def synth(topo, n_traces=3000):
    return anomod.synth_generate_host(anomod.SynthSpec(topo, seed=1, p_orphan_ppm=2000), n_traces)


@pytest.fixture(scope="module", params=["SN", "TT"])
def nested(request):
    sp = synth(request.param)
    par = parents_ref(sp)
    ns = nested_set(sp, par, P_SEQ[request.param], seed=7)
    return request.param, ns, par, critical_path_ref(ns, par)


# ------------------------------------------------------------------ C ABI, flags
def test_library_exports_critical_path_entry_point():
    assert "anomod_edge_critical_path_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    assert hasattr(lib, "anomod_edge_critical_path_spans")
    table = anomod.EdgeTable.empty(["a"], with_hist=False)
    cs = table.c_struct()
    rc = lib.anomod_edge_critical_path_spans(None, None, 1, C.byref(cs), None, None)
    assert rc == L.EINVAL
    assert b"anomod_edge_critical_path_spans" in lib.anomod_last_error(None)


def test_features_accepts_the_flag():
    p = inspect.signature(anomod.features).parameters
    assert "critical_path" in p and p["critical_path"].default is False
    assert "cp_edges" in anomod.Features.__dataclass_fields__
    assert hasattr(anomod.Context, "critical_path") and hasattr(anomod, "CriticalPath")


def test_cli_lists_critical_path_flag():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--critical-path" in r.stdout


def test_service_share():
    t = anomod.EdgeTable.empty(["a", "b"], with_hist=False)
    assert anomod.CriticalPath(t).service_share().tolist() == [0.0, 0.0]
    t.sum_us[:] = [1, 2, 3, 4, 5, 6, 7, 12]      # rows p * 2 + c
    np.testing.assert_allclose(anomod.CriticalPath(t).service_share(), [16 / 40, 24 / 40])


# ------------------------------------------------------------------ hand-made traces
def test_reference_hand_made_traces():
    sp, want_on, want_cp = hand_set()
    cp, on, _ = critical_path_ref(sp)
    ptr = sp.trace_ptr.astype(np.int64)
    for t, case in enumerate(HAND_CASES):
        a, b = ptr[t], ptr[t + 1]
        assert on[a:b].tolist() == want_on[a:b].tolist(), case[0]
        assert cp[a:b].tolist() == want_cp[a:b].tolist(), case[0]
    # the literal loop of the definition gives the same
    cp2, on2, _ = critical_path_ref(sp, select=select_literal)
    np.testing.assert_array_equal(cp2, cp)
    np.testing.assert_array_equal(on2, on)
    # the table: the on-path spans, in the rows the edge table gives them
    tab = cp_table_ref(sp, cp, on)
    rows = native.span_edges(sp, sp.n_services).astype(np.int64)
    cnt = np.bincount(rows[on == 1], minlength=tab["count"].shape[0])
    np.testing.assert_array_equal(tab["count"], cnt)
    tot = np.bincount(rows[on == 1], weights=cp[on == 1], minlength=cnt.shape[0])
    np.testing.assert_array_equal(tab["sum_us"], tot.astype(np.uint64))


def test_reference_literal_and_sorted_selection_agree_on_random_starts():
    sp = synth("SN", 300)
    rs = random_starts(sp, seed=3)
    a = critical_path_ref(rs)
    b = critical_path_ref(rs, select=select_literal)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert 0 < a[1].sum() < rs.n_spans


# ------------------------------------------------------------------ nested sets
def test_nested_children_lie_inside_their_parents(nested):
    _, ns, par, _ = nested
    c = np.nonzero(par != NO_PARENT)[0]
    s, e = ns.start_us.astype(np.int64), ns.start_us.astype(np.int64) + ns.dur_us
    assert (s[c] >= s[par[c]]).all() and (e[c] <= e[par[c]]).all()


def test_nested_conservation(nested):
    """Sum of cp_us over a trace == sum of its heads' durations."""
    _, ns, par, (cp, on, _) = nested
    t_of = ns.trace_of_span()
    got = np.bincount(t_of, weights=cp.astype(np.float64), minlength=ns.n_traces)
    head = par == NO_PARENT
    want = np.bincount(t_of[head], weights=ns.dur_us[head].astype(np.float64),
                       minlength=ns.n_traces)
    np.testing.assert_array_equal(got, want)
    assert (cp[on == 0] == 0).all() and (cp <= ns.dur_us).all()


def test_nested_input_is_not_degenerate(nested):
    """A condition on the helper: on-path and off-path spans each >= 5 % of
    the spans, >= 1 % of the parents select two children or more."""
    topo, ns, par, (_, on, nsel) = nested
    share_on = float(on.mean())
    has_child = np.zeros(ns.n_spans, bool)
    has_child[par[par != NO_PARENT]] = True
    multi = float((nsel[has_child] >= 2).mean())
    print(topo, "on-path share", round(share_on, 3), "parents selecting >= 2", round(multi, 3),
          "largest selection", int(nsel.max()))
    assert share_on >= 0.05 and 1.0 - share_on >= 0.05
    assert multi >= 0.01


# ------------------------------------------------------------------ evidence (fan-out)
def _terms(cur, base):
    """(critical-path, self-time, inclusive) latency terms of cur against base."""
    out = []
    for sp in (cur, base):
        cp, on, _ = critical_path_ref(sp)
        out.append((as_edge_table(cp_table_ref(sp, cp, on), sp.services),
                    as_edge_table(self_table_ref(sp), sp.services),
                    as_edge_table(native.finalize(native.edge_aggregate(sp)), sp.services)))
    return [_latency_shift(c, b) for c, b in zip(*out)]


def test_evidence_gateway_own_work():
    """+50 ms on the gateway's own work: only the critical-path term names the
    gateway alone; its self time is saturated before and after."""
    base, cur = fanout_set(200, seed=5), fanout_set(200, seed=5, gateway_extra_us=50_000)
    g = FANOUT_SERVICES.index("gateway")
    crit, self_, inc = _terms(cur, base)
    assert crit[g] > 0 and (np.delete(crit, g) == 0.0).all()
    assert self_[g] == 0.0
    assert inc[g] > 0


def test_evidence_shorter_sibling():
    """+20 ms on sibling b, still shorter than a: self time fires for b, the
    critical path for nobody."""
    base, cur = fanout_set(200, seed=5), fanout_set(200, seed=5, b_extra_us=20_000)
    assert (cur.dur_us[3::5] < cur.dur_us[2::5]).all()
    b = FANOUT_SERVICES.index("b")
    crit, self_, _ = _terms(cur, base)
    assert self_[b] > 0
    assert (crit == 0.0).all()

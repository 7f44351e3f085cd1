"""Self time, host side (no GPU): the C entry point's export and NULL
handling, the reference helper's own properties (tests/self_time_ref.py), the
propagated-fault invariant at the table level, and the CLI flag."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import _latency_shift
from conftest import PKG_DIR
from oracle import native

from self_time_ref import (INT_FIELDS, NO_PARENT, add_delay, ancestors_and_descendants,
                           as_edge_table, class_shares, parents_ref, self_table_ref, self_us_ref)

DELAY_US = 50_000
FAULTS = {"SN": "home-timeline-service", "TT": "ts-order-service"}


def synth(topo, n_traces=3000, **kw):
    return anomod.synth_generate_host(anomod.SynthSpec(topo, seed=1, p_orphan_ppm=2000, **kw),
                                      n_traces)


@pytest.fixture(scope="module", params=["SN", "TT"])
def topo_set(request):
    sp = synth(request.param)
    par = parents_ref(sp)
    return request.param, sp, par, self_us_ref(sp, par)


# ------------------------------------------------------------------ C ABI
def test_library_exports_self_time_entry_point():
    assert "anomod_edge_self_time_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    assert hasattr(lib, "anomod_edge_self_time_spans")
    table = anomod.EdgeTable.empty(["a"], with_hist=False)
    cs = table.c_struct()
    rc = lib.anomod_edge_self_time_spans(None, None, 1, C.byref(cs), None)
    assert rc == L.EINVAL
    assert b"anomod_edge_self_time_spans" in lib.anomod_last_error(None)


# ------------------------------------------------------------------ reference
def test_reference_conservation(topo_set):
    _, sp, par, su = topo_set
    assert su.dtype == np.uint32 and (su <= sp.dur_us).all()
    has_child = np.zeros(sp.n_spans, bool)
    has_child[par[par != NO_PARENT]] = True
    leaf = ~has_child
    assert leaf.any() and has_child.any()
    np.testing.assert_array_equal(su[leaf], sp.dur_us[leaf])
    # the child sums account for every duration that has a parent
    child_sum = np.zeros(sp.n_spans, np.int64)
    np.add.at(child_sum, par[par != NO_PARENT], sp.dur_us[par != NO_PARENT].astype(np.int64))
    np.testing.assert_array_equal(
        su.astype(np.int64), sp.dur_us.astype(np.int64) - np.minimum(sp.dur_us, child_sum))


def test_reference_classes_are_not_degenerate(topo_set):
    topo, sp, _, su = topo_set
    shares = class_shares(sp, su)
    print(topo, "self == 0 / 0 < self < dur / self == dur:", np.round(shares, 3))
    assert min(shares) >= 0.10


def test_reference_parent_rule_is_the_edge_tables(topo_set):
    """Row of every span from the reference's parents == native.span_edges."""
    _, sp, par, _ = topo_set
    S = sp.n_services
    svc = sp.svc.astype(np.int64)
    # a self-reference keeps its own service as the parent service
    self_ref = (sp.parent_span_id != 0) & (sp.parent_span_id == sp.span_id) & (par == NO_PARENT)
    prow = np.where(sp.parent_span_id == 0, S,
                    np.where(par != NO_PARENT, svc[np.maximum(par, 0)],
                             np.where(self_ref, svc, S + 1)))
    np.testing.assert_array_equal(prow * S + svc, native.span_edges(sp, S).astype(np.int64))
    assert (prow == S + 1).any()  # orphans present


def test_reference_hand_made():
    """Child before parent, duplicated id (first carrier wins), self-reference,
    orphan, saturation."""
    ids = [10, 20, 30, 20, 40, 50, 60]
    pids = [20, 0, 20, 20, 40, 999, 30]
    durs = [5, 100, 7, 50, 9, 11, 30]
    sp = anomod.SpanSet(["a", "b"], [0, 7], [1] * 7, ids, pids, [0, 1, 0, 1, 0, 1, 0], [0] * 7,
                        durs)
    par = parents_ref(sp)
    assert par.tolist() == [1, -1, 1, 1, -1, -1, 2]
    # span 1 (id 20, first carrier) gets 5 + 7 + 50; span 3 (second carrier) none
    assert self_us_ref(sp, par).tolist() == [5, 100 - 62, 0, 50, 9, 11, 30]
    rows = native.span_edges(sp, 2)
    assert rows[4] == 0 * 2 + 0      # the self-reference: its own service as parent
    assert rows[5] == 3 * 2 + 1      # ORPHAN -> b


def test_propagated_fault_invariant(topo_set):
    """A delay on one service, propagated to its ancestors' inclusive
    durations, changes the self-time table only in that service's columns, and
    the self-time latency shift is exactly 0 off the faulted service."""
    topo, base, par, su = topo_set
    fault = FAULTS[topo]
    anc, desc = ancestors_and_descendants(base, fault, par)
    # (SN: a service in mid-path; the TT generator's order service calls nothing)
    assert anc and (desc or topo == "TT")
    cur = add_delay(base, fault, DELAY_US, par)
    S, c = base.n_services, base.services.index(fault)
    changed = {base.services[k] for k in np.unique(base.svc[cur.dur_us != base.dur_us]).tolist()}
    assert changed == {fault} | {base.services[k] for k in anc}
    tb, tc = self_table_ref(base, su), self_table_ref(cur)
    other = np.arange((S + 2) * S) % S != c
    for k in INT_FIELDS + ("p50_us", "p99_us"):
        np.testing.assert_array_equal(tc[k][other], tb[k][other], err_msg=k)
    hit = ~other & (tb["count"] > 0)
    assert hit.any() and (tc["sum_us"][hit] > tb["sum_us"][hit]).all()
    np.testing.assert_array_equal(tc["count"], tb["count"])
    lat = _latency_shift(as_edge_table(tc, cur.services), as_edge_table(tb, base.services))
    assert lat[c] > 0
    assert (np.delete(lat, c) == 0.0).all()
    # the inclusive tables raise the term for at least one other service
    inc = _latency_shift(
        as_edge_table(native.finalize(native.edge_aggregate(cur)), cur.services),
        as_edge_table(native.finalize(native.edge_aggregate(base)), base.services))
    assert (np.delete(inc, c) > 0).any()


# ------------------------------------------------------------------ CLI
def test_cli_lists_self_time_flag():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--self-time" in r.stdout

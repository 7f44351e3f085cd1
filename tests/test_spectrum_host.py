"""Trace spectrum, host side (no GPU): the C entry point's export and NULL
handling, the reference helper (tests/spectrum_ref.py) against a brute-force
loop and its invariants, the ranking property on the reference alone,
spectrum_thresholds, and the CLI flags."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from conftest import PKG_DIR
from oracle import native

from self_time_ref import add_delay
from spectrum_ref import (U32_MAX, oracle_table, rows_ref, service_ochiai_ref, spectrum_ref)

DELAY_US = 50_000
FAULTS = {"SN": "home-timeline-service", "TT": "ts-order-service"}


def synth(topo, n_traces=3000, **kw):
    return anomod.synth_generate_host(anomod.SynthSpec(topo, seed=1, p_orphan_ppm=2000, **kw),
                                      n_traces)


# ------------------------------------------------------------------ C ABI
def test_library_exports_trace_spectrum_entry_point():
    assert "anomod_trace_spectrum_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    assert hasattr(lib, "anomod_trace_spectrum_spans")
    cs = L.TraceSpectrumC(1, 1, None, (0, 0), None, None, None, None)
    assert lib.anomod_trace_spectrum_spans(None, None, C.byref(cs)) == L.EINVAL
    assert b"anomod_trace_spectrum_spans" in lib.anomod_last_error(None)
    assert lib.anomod_trace_spectrum_spans(None, None, None) == L.EINVAL
    assert b"anomod_trace_spectrum_spans" in lib.anomod_last_error(None)


# ------------------------------------------------------------------ reference
def _brute_force(sp, rows, thr, use_errors):
    """The definition, one trace at a time over Python sets."""
    S = sp.n_services
    E = (S + 2) * S
    out = {"n_traces": [0, 0], "svc_traces": np.zeros((2, S), np.uint64),
           "edge_traces": np.zeros((2, E), np.uint64), "bad_spans": np.zeros(E, np.uint64),
           "trace_abnormal": np.zeros(sp.n_traces, np.uint8)}
    ptr = sp.trace_ptr.tolist()
    for t in range(sp.n_traces):
        seen_rows, seen_svc, abnormal = set(), set(), False
        for i in range(ptr[t], ptr[t + 1]):
            r = int(rows[i])
            bad = int(sp.dur_us[i]) > int(thr[r]) or (use_errors and bool(int(sp.flags[i]) & 1))
            if bad:
                out["bad_spans"][r] += 1
                abnormal = True
            seen_rows.add(r)
            seen_svc.add(int(sp.svc[i]))
        k = 1 if abnormal else 0
        out["n_traces"][k] += 1
        out["trace_abnormal"][t] = k
        for r in seen_rows:
            out["edge_traces"][k, r] += 1
        for s in seen_svc:
            out["svc_traces"][k, s] += 1
    out["n_traces"] = np.asarray(out["n_traces"], np.uint64)
    return out


@pytest.mark.parametrize("use_errors", [True, False])
def test_reference_against_brute_force(use_errors):
    sp = synth("SN", 200, fault_service=FAULTS["SN"])
    # an empty trace in the middle and at the end
    lens = np.diff(sp.trace_ptr).astype(np.int64)
    lens = np.r_[lens[:100], 0, lens[100:], 0]
    ptr = np.zeros(lens.shape[0] + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    sp = anomod.SpanSet(sp.services, ptr, sp.trace_hash, sp.span_id, sp.parent_span_id, sp.svc,
                        sp.flags, sp.dur_us)
    rows = rows_ref(sp)
    thr = anomod.spectrum_thresholds(oracle_table(synth("SN", 200)), sp.services, rows="all")
    ref = spectrum_ref(sp, thr, use_errors, rows)
    brute = _brute_force(sp, rows, thr, use_errors)
    for k, v in brute.items():
        np.testing.assert_array_equal(ref[k], v, err_msg=k)
    assert ref["n_traces"].min() > 0 and ref["bad_spans"].sum() > 0
    assert ref["trace_abnormal"][100] == 0 and ref["trace_abnormal"][-1] == 0


@pytest.mark.parametrize("topo", ["SN", "TT"])
def test_reference_rows_and_invariants(topo):
    sp = synth(topo, 1000, fault_service=FAULTS[topo])
    rows = rows_ref(sp)
    S = sp.n_services
    E = (S + 2) * S
    count = native.edge_aggregate(sp)["count"]
    np.testing.assert_array_equal(np.bincount(rows, minlength=E), count)
    thr = anomod.spectrum_thresholds(oracle_table(synth(topo, 1000)), sp.services, rows="all")
    for use_errors in (True, False):
        ref = spectrum_ref(sp, thr, use_errors, rows)
        assert int(ref["n_traces"].sum()) == sp.n_traces
        assert (ref["svc_traces"] <= ref["n_traces"][:, None]).all()
        assert (ref["edge_traces"] <= ref["n_traces"][:, None]).all()
        assert (ref["edge_traces"][0] + ref["edge_traces"][1] <= count).all()
        assert (ref["bad_spans"] <= count).all()
        assert int(ref["trace_abnormal"].sum()) == int(ref["n_traces"][1])
    none = spectrum_ref(sp, None, False, rows)
    assert none["n_traces"].tolist() == [sp.n_traces, 0] and not none["bad_spans"].any()


@pytest.mark.parametrize("topo", ["SN", "TT"])
@pytest.mark.parametrize("use_errors", [False, True])
def test_reference_ranks_the_delayed_service_first(topo, use_errors):
    """A 50 ms delay on one service, propagated to its ancestors; thresholds on
    the ROOT rows from the un-delayed run's p99: the delayed service has the
    largest Ochiai coefficient (measured: SN 0.997 against 0.822, TT 0.994
    against 0.773 without error flags)."""
    fault = FAULTS[topo]
    base = synth(topo)
    cur = add_delay(base, fault, DELAY_US)
    thr = anomod.spectrum_thresholds(oracle_table(base), cur.services, rows="root")
    S = cur.n_services
    assert (thr[: S * S] == U32_MAX).all() and (thr[S * S: S * S + S] != U32_MAX).any()
    och = service_ochiai_ref(spectrum_ref(cur, thr, use_errors))
    order = np.argsort(-och, kind="stable")
    print(topo, "errors", use_errors, "top:", cur.services[order[0]], och[order[0]],
          "runner-up:", cur.services[order[1]], och[order[1]])
    assert cur.services[order[0]] == fault
    assert och[order[0]] > och[order[1]]


# ------------------------------------------------------------------ thresholds
def _table(services, rows: dict) -> anomod.EdgeTable:
    """rows: (parent name | 'ROOT' | 'ORPHAN', child name) -> (count, p99)."""
    t = anomod.EdgeTable.empty(services, with_hist=False)
    S = len(services)
    for (p, c), (n, q) in rows.items():
        pi = S if p == "ROOT" else S + 1 if p == "ORPHAN" else services.index(p)
        r = pi * S + services.index(c)
        t.count[r] = n
        t.p99_us[r] = q
    return t


def test_spectrum_thresholds():
    base = _table(["a", "b", "c"], {("ROOT", "a"): (50, 1234.9), ("ROOT", "b"): (9, 77.0),
                                    ("a", "b"): (20, 10.5), ("b", "c"): (30, float("nan")),
                                    ("ORPHAN", "c"): (12, 5e12), ("ROOT", "c"): (10, 0.0)})
    cur = ["b", "x", "a", "c"]   # another order, a service the baseline never saw
    S = 4

    def row(p, c):
        pi = S if p == "ROOT" else S + 1 if p == "ORPHAN" else cur.index(p)
        return pi * S + cur.index(c)

    root = anomod.spectrum_thresholds(base, cur)
    assert root.dtype == np.uint32 and root.shape == ((S + 2) * S,)
    want = {row("ROOT", "a"): 1234, row("ROOT", "c"): 0}     # ROOT -> b: 9 spans < min_count
    for r in range((S + 2) * S):
        assert root[r] == want.get(r, U32_MAX), r
    every = anomod.spectrum_thresholds(base, cur, rows="all")
    want.update({row("a", "b"): 10, row("ORPHAN", "c"): U32_MAX})   # (p99 beyond u32 saturates)
    for r in range((S + 2) * S):
        assert every[r] == want.get(r, U32_MAX), r
    low = anomod.spectrum_thresholds(base, cur, rows="all", min_count=5)
    assert low[row("ROOT", "b")] == 77
    assert low[row("b", "c")] == U32_MAX                            # no finite p99
    with pytest.raises(ValueError):
        anomod.spectrum_thresholds(base, cur, rows="leaf")


def test_ochiai_of_a_hand_made_spectrum():
    sp = anomod.TraceSpectrum(["a", "b", "c"], np.array([6, 4], np.uint64),
                              np.array([[6, 0, 0], [4, 2, 0]], np.uint64),
                              np.zeros((2, 15), np.uint64), np.zeros(15, np.uint64), None, None)
    np.testing.assert_array_equal(sp.ochiai(), [4 / np.sqrt(4.0 * 10), 2 / np.sqrt(4.0 * 2), 0.0])
    assert not sp.edge_ochiai().any()
    none = anomod.TraceSpectrum(["a"], np.array([3, 0], np.uint64), np.array([[3], [0]], np.uint64),
                                np.zeros((2, 3), np.uint64), np.zeros(3, np.uint64), None, None)
    assert none.ochiai().tolist() == [0.0]


# ------------------------------------------------------------------ CLI
def test_cli_lists_spectrum_flags():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--spectrum" in r.stdout and "--baseline" in r.stdout

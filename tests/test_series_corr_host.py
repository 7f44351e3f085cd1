"""Series correlation, host side: the model against numpy, the inputs of the
GPU tests against the bound they rely on, EdgeWindows.symptom and walk_graph on
hand-worked tables, the header and the bindings.  No GPU."""
import re

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import EdgeTable, EdgeWindows
from conftest import ROOT
from series_corr_ref import (BOUND_MAX, K_CASES, S_CASES, T_CASES, adversarial_case,
                             correlate_ref, min_pairs_of, random_case)


# ---- the model --------------------------------------------------------------
def test_model_equals_corrcoef_on_complete_data():
    rng = np.random.default_rng(2)
    X = (100 + rng.standard_normal((200, 7))).astype(np.float32)
    Y = (X[:, :2] * [1.5, -0.5] + rng.standard_normal((200, 2))).astype(np.float32)
    m = correlate_ref(X, Y)
    full = np.corrcoef(np.concatenate([Y, X], axis=1).astype(np.float64), rowvar=False)
    np.testing.assert_allclose(m["r"], full[:2, 2:], rtol=0, atol=1e-13)
    assert (m["n"] == 200).all()
    assert m["r"][0, 0] > 0.7 and m["r"][1, 1] < -0.3


def test_model_is_pairwise_complete():
    """Every (k, s) against numpy on just its own pair set."""
    X, Y = random_case(65, 5, 2)
    m = correlate_ref(X, Y, 3)
    for k in range(2):
        for s in range(5):
            pair = np.isfinite(X[:, s]) & np.isfinite(Y[:, k])
            assert m["n"][k, s] == pair.sum()
            want = np.corrcoef(X[pair, s].astype(np.float64), Y[pair, k].astype(np.float64))[0, 1]
            assert abs(m["r"][k, s] - want) < 1e-12


def test_model_nan_rules():
    X = np.array([[1, 5, np.nan, 1, np.inf],
                  [2, 5, np.nan, 2, 1],
                  [3, 5, np.nan, np.nan, 2],
                  [4, 5, np.nan, np.nan, -np.inf]], np.float32)
    y = np.array([1, 2, 4, np.nan], np.float32)
    m = correlate_ref(X, y, min_pairs=3)
    np.testing.assert_array_equal(m["n"][0], [3, 3, 0, 2, 2])
    assert m["r"][0, 0] == pytest.approx(np.corrcoef([1, 2, 3], [1, 2, 4])[0, 1], abs=1e-15)
    assert np.isnan(m["r"][0, 1:]).all()        # constant; no sample; below min_pairs; +-inf
    # two pairs are enough at min_pairs <= 2 (never fewer than 2)
    assert correlate_ref(X, y, min_pairs=0)["r"][0, 3] == pytest.approx(1.0)
    assert correlate_ref(X, y, min_pairs=2)["r"][0, 4] == pytest.approx(1.0)
    one = correlate_ref(X[:1], y[:1], min_pairs=0)
    assert one["n"][0, 0] == 1 and np.isnan(one["r"]).all()
    # a constant target
    assert np.isnan(correlate_ref(X, np.full(4, 3.0, np.float32))["r"]).all()


def test_bound_formula():
    X, Y = random_case(97, 65, 2)
    m = correlate_ref(X, Y)
    T = 97
    fin = np.isfinite(m["kx"]) & np.isfinite(m["ky"])
    assert fin.sum() > 100
    # k >= 1 (the mean minimises the sum of squares), = 1 + n (p - mean)^2 / sxx
    assert (m["kx"][fin] >= 1 - 1e-12).all() and (m["ky"][fin] >= 1 - 1e-12).all()
    np.testing.assert_array_equal(
        m["bound"][fin], 8.0 * T * 2.0 ** -53 * np.maximum(m["kx"], m["ky"])[fin] + 2.0 ** -50)
    s = 3
    pair = np.isfinite(X[:, s]) & np.isfinite(Y[:, 0])
    x = X[pair, s].astype(np.float64)
    px = X[np.isfinite(X[:, s]), s][0].astype(np.float64)
    want = 1 + x.size * (px - x.mean()) ** 2 / ((x - x.mean()) ** 2).sum()
    assert m["kx"][0, s] == pytest.approx(want, rel=1e-9)
    # a pivot at the mean: k = 1, the bound is its floor
    sym = correlate_ref(np.array([[0], [-1], [1]], np.float32), np.array([0, -2, 2], np.float32))
    assert sym["kx"][0, 0] == 1 and sym["ky"][0, 0] == 1
    assert sym["bound"][0, 0] == 8 * 3 * 2.0 ** -53 + 2.0 ** -50


def test_gpu_inputs_stay_inside_the_bound_they_assume():
    """The GPU comparison needs bound <= 1e-6 wherever the model gives an r
    (k <= 2^16, T <= 4096): checked here from the model alone."""
    worst = 0.0
    for T in T_CASES:
        for S in S_CASES:
            for K in K_CASES:
                X, Y = random_case(T, S, K)
                m = correlate_ref(X, Y, min_pairs_of(T))
                have = ~np.isnan(m["r"])
                if have.any():
                    worst = max(worst, float(m["bound"][have].max()))
                    assert max(m["kx"][have].max(), m["ky"][have].max()) <= 2.0 ** 16, (T, S, K)
    assert 0 < worst <= BOUND_MAX
    X, Y, cols = adversarial_case()
    m = correlate_ref(X, Y, 4)
    have = ~np.isnan(m["r"])
    assert m["bound"][have].max() <= BOUND_MAX
    # the series at 1e9: the pivot keeps k small (mean^2 / variance is ~1e13)
    assert m["kx"][0, cols["large_level"]] < 16


# ---- EdgeWindows.symptom -----------------------------------------------------
def test_symptom_on_a_hand_written_table():
    win = EdgeWindows.empty(["a", "b"], 0, 1_000_000, 5)
    S = 2
    root_a, root_b = S * S, S * S + 1
    win.count[0, root_a], win.sum_us[0, root_a] = 3, 300
    win.count[0, root_b], win.sum_us[0, root_b] = 2, 700       # 5 spans, mean 200
    win.count[1, root_a], win.sum_us[1, root_a] = 4, 4000      # below min_count
    win.count[3, root_b], win.sum_us[3, root_b] = 10, 10230    # mean 1023
    win.count[4, root_a], win.sum_us[4, root_a] = 5, 0         # mean 0
    win.count[:, 1], win.sum_us[:, 1] = 1000, 10 ** 9          # a -> b: not a ROOT row
    win.count[2, (S + 1) * S], win.sum_us[2, (S + 1) * S] = 50, 5000   # ORPHAN: not ROOT
    y = win.symptom(5)
    assert y.dtype == np.float32 and y.shape == (5,)
    np.testing.assert_array_equal(
        y, np.array([np.log2(201.0), np.nan, np.nan, 10.0, 0.0], np.float32))
    y4 = win.symptom(4)
    assert y4[1] == np.float32(np.log2(1001.0)) and np.isnan(y4[2])
    # min_count 0 still needs one span
    assert np.isnan(win.symptom(0)[2]) and win.symptom(0)[1] == y4[1]
    # a run whose traces hold no ROOT span
    win.count[:, root_a:root_b + 1] = 0
    win.sum_us[:, root_a:root_b + 1] = 0
    assert np.isnan(win.symptom(1)).all()


# ---- walk_graph --------------------------------------------------------------
def _edges(services, calls):
    e = EdgeTable.empty(services, with_hist=False)
    S = len(services)
    for (p, c), n in calls.items():
        e.count[p * S + c] = n
    return e


def test_walk_graph_on_a_hand_worked_graph():
    # a -> b -> c; a calls itself and is the entry (ROOT row): neither is an edge
    e = _edges(["a", "b", "c"], {(0, 1): 5, (1, 2): 2, (0, 0): 9, (3, 0): 7})
    corr = np.array([0.5, 0.2, 0.8])
    row_ptr, col, w = anomod.walk_graph(e, corr, 0.5)
    assert row_ptr.dtype == np.uint32 and col.dtype == np.uint32 and w.dtype == np.float32
    # c = corr + 0.01.  a: self 0.51 - 0.21, forward to b 0.21.
    # b: back to a 0.5 * 0.51, forward to c 0.81, self max(0, 0.21 - 0.81) = 0: dropped.
    # c: back to b 0.5 * 0.21, calls nobody: self 0.81.
    np.testing.assert_array_equal(row_ptr, [0, 2, 4, 6])
    np.testing.assert_array_equal(col, [0, 1, 0, 2, 1, 2])
    np.testing.assert_array_equal(
        w, np.array([0.51 - 0.21, 0.21, 0.5 * 0.51, 0.81, 0.5 * 0.21, 0.81], np.float32))


def test_walk_graph_adds_coinciding_edges_and_keeps_zero_back_edges():
    # a <-> b: a -> b is forward (c[b]) and the back edge of b -> a (rho * c[b])
    e = _edges(["a", "b"], {(0, 1): 1, (1, 0): 1})
    row_ptr, col, w = anomod.walk_graph(e, np.array([0.39, 0.09]), 0.25)
    np.testing.assert_array_equal(row_ptr, [0, 2, 3])
    np.testing.assert_array_equal(col, [0, 1, 0])
    np.testing.assert_array_equal(
        w, np.array([0.4 - 0.1, 0.1 + 0.25 * 0.1, 0.4 + 0.25 * 0.4], np.float32))
    # rho = 0: the back edge stays, with weight 0; an isolated node keeps its self edge
    e = _edges(["a", "b", "c"], {(0, 1): 3})
    row_ptr, col, w = anomod.walk_graph(e, np.zeros(3), 0.0)
    np.testing.assert_array_equal(row_ptr, [0, 1, 3, 4])
    np.testing.assert_array_equal(col, [1, 0, 1, 2])
    np.testing.assert_array_equal(w, np.array([0.01, 0.0, 0.01, 0.01], np.float32))
    with pytest.raises(ValueError):
        anomod.walk_graph(e, np.zeros(2))
    with pytest.raises(ValueError):
        anomod.walk_graph(e, np.zeros(3), -1.0)


# ---- header, bindings, argument checks ----------------------------------------
def test_header_and_bindings():
    text = (ROOT / "include" / "anomod.h").read_text()
    assert "#define ANOMOD_CORR_MAX_TARGETS 8" in text
    assert "#define ANOMOD_ABI_VERSION 2" in text and L.ABI_VERSION == 2
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = anomod.lib()
    for name in ("anomod_series_correlate", "anomod_correlate"):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert L.CORR_MAX_TARGETS == 8 and L.STAGE_SERIES_CORR == 16
    # the contract is stated where the symbols are declared
    for phrase in ("2^-50", "pairwise-complete", "max(min_pairs, 2)"):
        assert phrase in text, phrase
    assert hasattr(anomod.Context, "correlate") and hasattr(anomod.DeviceSeries, "correlate")


def _feats(symptom_corr=None):
    e = _edges(["a", "b"], {(0, 1): 4})
    return anomod.Features("x", e, None, None, np.array([0.0, 1.0]), symptom_corr=symptom_corr)


def test_rank_correlation_walk_needs_symptom_corr():
    with pytest.raises(ValueError, match="symptom_corr"):
        anomod.rank(_feats(), walk="correlation")
    with pytest.raises(ValueError, match="walk"):
        anomod.rank(_feats(), walk="counts")


def test_features_symptom_corr_needs_a_step():
    exp = anomod.load_experiment(anomod.SynthSpec("SN", seed=1), n_traces=20, metric_steps=0)
    with pytest.raises(ValueError, match="trace_step_s"):
        anomod.features(exp, symptom_corr=True)


def test_symptom_correlation_top():
    sc = anomod.SymptomCorrelation(
        ["a"], np.zeros(3, np.float32), [("edge_mean_us", (("child", "a"),)), ("edge_p99_us", ())],
        np.array([0.5, np.nan]), np.array([9, 0], np.uint32), np.array([0.5]), "regular",
        (0, 2), np.zeros(3, np.float32), [("cpu", (("pod", "a-1"),)), ("mem", ())],
        np.array([-0.9, 0.2]), np.array([3, 3], np.uint32), np.array([0.9]))
    top = sc.top(2)
    assert [(t["kind"], t["key"][0], t["r"], t["n"]) for t in top] == [
        ("metric", "cpu", -0.9, 3), ("trace", "edge_mean_us", 0.5, 9)]
    assert len(sc.top(10)) == 3 and sc.top(0) == []

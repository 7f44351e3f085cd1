"""Host checks of the PageRank reference helper (tests/pagerank_ref.py) that
the GPU solves are compared with: against the C oracle and the networkx
golden (f64 weights), the size of the float-weight rounding, f64 against long
double, zero-weight rows, and the shapes of the shared graph cases."""
import numpy as np
import pytest

from oracle import native
from pagerank_ref import (ALPHA, EPS52, HUB_NODE, IN_DEGREES, TOL_GUARD, assert_elementwise,
                          case_names, edge_model, elementwise_bound, graph_case,
                          pagerank_ref, personalization_sum, personalizations, pick_tol, ref_tol)

CASES = case_names()
ITERS = (1, 2, 50)


def _oracle(g, p, iters, tol=0.0):
    return native.pagerank(g.row_ptr, g.col, g.w, p, ALPHA, iters=iters, tol=tol)


@pytest.mark.parametrize("name", CASES)
def test_f64_weights_equal_the_oracle(name):
    """round_weights=False is the oracle's model: elementwise within
    iters * (max in-degree + 16) * 2^-52, zeros exact."""
    g = graph_case(name)
    for label, p in personalizations(name):
        for iters in ITERS:
            x, errs = pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, iters, round_weights=False)
            xo, ito = _oracle(g, p, iters)
            assert ito == len(errs) == iters
            assert_elementwise(x, xo, elementwise_bound(g, iters), f"{name} {label} {iters}")


@pytest.mark.parametrize("name", CASES)
def test_float_weights_stay_within_their_rounding(name):
    """Each float weight is off by at most 2^-24 relative and the terms are
    non-negative, so an iteration adds at most 2^-24 to the relative error of
    every entry: (iters + 1) * 2^-23 bounds it with room for the f64 noise."""
    g = graph_case(name)
    for label, p in personalizations(name):
        for iters in ITERS:
            x, _ = pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, iters)
            xo, _ = _oracle(g, p, iters)
            assert_elementwise(x, xo, (iters + 1) * 2.0 ** -23, f"{name} {label} {iters}")


@pytest.mark.parametrize("name", CASES)
def test_f64_and_long_double_agree(name):
    """The reference's own rounding is far inside the bound the GPU solves
    are held to (both runs use the float weights)."""
    g = graph_case(name)
    worst = 0.0
    for label, p in personalizations(name):
        a, ea = pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, 50)
        b, eb = pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, 50, dtype=np.longdouble)
        assert b.dtype == np.longdouble
        nz = b != 0
        assert (a[~nz] == 0).all()
        ratio = np.abs(a[nz] - b[nz]) / (np.longdouble(elementwise_bound(g, 50)) * b[nz])
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        # the L1 changes (differences of nearly equal vectors): absolutely close
        np.testing.assert_allclose(np.asarray(ea, np.float64), np.asarray(eb, np.float64),
                                   rtol=0, atol=1e-13)
    assert worst <= 1.0, worst


def test_networkx_golden(golden):
    """The f64-weight reference run to a far tighter tolerance lies within
    the golden's own convergence: networkx stopped at an L1 change below
    N * tol, which leaves at most alpha / (1 - alpha) * N * tol to the fixed
    point (the iteration contracts L1 by alpha)."""
    g = np.load(golden / "pagerank_networkx.npz")
    N, alpha, nx_tol = g["p"].shape[0], float(g["alpha"]), 1e-12
    x, errs = pagerank_ref(g["row_ptr"], g["col"], g["w"], g["p"], alpha, 1000, tol=1e-17,
                           round_weights=False)
    assert len(errs) < 1000
    assert np.abs(x - g["x"]).sum() <= alpha / (1 - alpha) * N * nx_tol
    xo, _ = native.pagerank(g["row_ptr"], g["col"], g["w"], g["p"], alpha, iters=len(errs), tol=0.0)
    indeg = int(np.bincount(g["col"], minlength=N).max())
    assert_elementwise(x, xo, len(errs) * (indeg + 16) * EPS52, "golden")


@pytest.mark.parametrize("N", [1, 2, 12, 257])
def test_zero_weight_rows_are_dangling(N):
    """A row whose weights are all 0.0 behaves as a row without edges in the
    oracle and in both models of the reference; everything stays finite."""
    g = graph_case(f"zero-{N}")
    zero_rows = g.meta["zero_rows"]
    assert zero_rows.size and (g.w == 0).any()
    src, wn, dangling = edge_model(g.row_ptr, g.col, g.w)
    assert dangling[zero_rows].all() and np.isfinite(wn).all()
    assert (wn[np.isin(src, zero_rows)] == 0).all()
    if N > 2:
        assert ((g.w == 0) & ~dangling[src]).any()      # a zero edge inside a normal row
    keep = ~np.isin(src, zero_rows)                    # the same graph with those edges dropped
    rp = np.zeros(N + 1, np.uint32)
    np.cumsum(np.bincount(src[keep], minlength=N), out=rp[1:])
    for label, p in personalizations(g.name):
        for rw in (True, False):
            x, _ = pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, 50, round_weights=rw)
            xd, _ = pagerank_ref(rp, g.col[keep], g.w[keep], p, ALPHA, 50, round_weights=rw)
            # (float weights of a row need not add up to exactly 1)
            assert np.isfinite(x).all() and abs(x.sum() - 1.0) < (51 * 2.0 ** -23 if rw else 1e-12)
            np.testing.assert_array_equal(x, xd)
        xo, _ = _oracle(g, p, 50)
        assert np.isfinite(xo).all()
        assert_elementwise(pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, 50,
                                        round_weights=False)[0], xo,
                           elementwise_bound(g, 50), f"{g.name} {label}")


def test_case_shapes():
    """The graph cases hold what their names promise."""
    for name in CASES:
        g = graph_case(name)
        assert g.row_ptr[-1] == g.col.shape[0] == g.w.shape[0]
        indeg = np.bincount(g.col, minlength=g.N)
        src, wn, dangling = edge_model(g.row_ptr, g.col, g.w)
        kind = name.split("-")[0]
        if kind == "indeg":
            for v, d in g.meta["targets"].items():
                assert indeg[v] == d, (name, v)
            assert g.N - 1 in g.meta["targets"]
            if g.N >= 8:
                assert sorted(g.meta["targets"].values()) == sorted(IN_DEGREES)
                assert g.meta["targets"][g.N - 1] == 9
        elif kind == "hub":
            assert indeg[HUB_NODE] == int(name.split("-")[1])
            assert np.unique(src[g.col == HUB_NODE]).size == indeg[HUB_NODE]
        elif kind == "dangling":
            assert g.col.size == 0 and dangling.all()
        elif kind == "ring":
            assert not dangling.any() and (indeg == 1).all()
        elif kind == "loops":
            assert (src == g.col).any()
            pairs = src * g.N + g.col
            assert np.unique(pairs).size < pairs.size
        elif kind == "wide":
            for u in np.unique(src):
                wu = g.w[g.row_ptr[u]:g.row_ptr[u + 1]]
                assert wu.min() == 1.0 and wu.max() == 2.0 ** 24
        elif kind == "random" and g.N >= 3:
            assert dangling.any() and (indeg == 0).any() and not dangling.all()
    labels = {l for n in CASES for l, _ in personalizations(n)}
    assert labels == {"dense", "half", "onehot_dangling", "onehot_no_in_edge"}


def test_personalization_sum_order():
    rng = np.random.default_rng(3)
    for n in (1, 7, 8, 9, 1279):
        p = rng.random(n)
        a = [0.0] * 8
        for i, v in enumerate(p.tolist()):
            a[i & 7] += v
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))
        assert personalization_sum(p) == s


@pytest.mark.parametrize("name", ["random-257", "ring-12", "dangling-46", "hub-4999", "zero-1"])
def test_tolerance_choice_clears_the_guard_band(name):
    """ref_tol's tolerance leaves no L1 change of the reference's sequence
    within TOL_GUARD of N * tol, and the oracle (f64 weights, its changes
    differ by the float rounding of the weights) is not asked to agree on the
    iteration — only the reference's own sequence is judged."""
    g = graph_case(name)
    for pi, (label, p) in enumerate(personalizations(name)):
        tol, stop, x = ref_tol(name, pi)
        x2, errs = pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, 1000, tol)
        assert len(errs) == stop
        np.testing.assert_array_equal(x, x2)
        thr = g.N * tol
        assert errs[-1] < thr and all(e >= thr for e in errs[:-1])
        assert all(abs(e - thr) > TOL_GUARD * thr for e in errs)
    with pytest.raises(AssertionError):
        pick_tol(lambda tol: (1, [[1.0, tol * (1 - 1e-7)]]))

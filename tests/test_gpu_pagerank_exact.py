"""Every PageRank path against an exact model of its arithmetic, per node.

Each GPU solve is compared with tests/pagerank_ref.py (float weights, f64),
elementwise:

    |x_gpu[i] - x_ref[i]| <= iters * (max_in_degree + 16) * 2^-52 * x_ref[i]
    x_ref[i] == 0  =>  x_gpu[i] == 0 exactly

The bound is derived, not measured.  Every term of the update
y = alpha * (sum_e x[src(e)] * w(e) + dsum * p) + (1 - alpha) * p is
non-negative, so nothing cancels and a relative error of the inputs passes to
the output without growing.  What one iteration adds to the relative error of
an entry is one rounding (2^-53) per in-edge fma on the GPU and two (product,
sum) per in-edge in the reference — together below 2^-52 * in-degree in
all but the worst alignment of every rounding, which a sum of d terms does
not reach — plus a constant for the row formula (two fmas, (1 - alpha) * p),
the division of p by its sum and the tree sums of the dangling mass on both
sides: 16 * 2^-52 holds them.  The dangling mass reaches the kernels through
a 2^-62 fixed-point accumulator: each 256-row block rounds its share to
2^-63 absolute, i.e. the term alpha * dsum * p[i] is off by at most
alpha * blocks * 2^-63 * p[i] while x[i] >= (1 - alpha) * p[i] — a relative
alpha / (1 - alpha) * blocks * 2^-63 < 1e-15 for the 20 blocks of the largest
graph here.  After `iters` iterations the bounds add up.

Tolerance mode: the reference runs first, and its tolerance is chosen (on
the reference alone) so that no L1 change of its sequence lies within 1e-6
relative of N * tol; the GPU then has to stop at exactly the reference's
iteration and match it there.

The graphs (tests/pagerank_ref.py: graph_case) are the shapes where a pull
SpMV goes wrong: N below, at and just above the 256-row block, the product's
12 and 46 services, in-degrees around the 8-wide edge batch, hubs, rings,
all-dangling, self-loops, parallel edges, weights over 24 binades, and rows
whose weights are all zero."""
import numpy as np
import pytest

import anomod
from pagerank_ref import (ALPHA, TOL_ITERS, assert_elementwise, case_names, elementwise_bound,
                          graph_case, personalizations, ref_fixed, ref_tol, ref_tol_batch)

pytestmark = pytest.mark.gpu

CASES = case_names()
SHARD_CASES = case_names(sizes=(257, 513), hubs=False)
FIXED_ITERS = (1, 2, 50)
EXTRA = 16                      # random personalizations after the named ones (fill a batch)
KNOBS = ("ANOMOD_PPR_MODE", "ANOMOD_PPR_SUB", "ANOMOD_PPR_RING", "ANOMOD_PPR_SPLIT",
         "ANOMOD_PPR_BSUB", "ANOMOD_PPR_SPIN")

# path -> environment; the solve's path is confirmed with last_solve()
SINGLE_PATHS = {"per_launch": {"ANOMOD_PPR_MODE": "1"}, "persistent": {}}
SINGLE_PATHS.update({f"persistent-sub{s}-ring{r}": {"ANOMOD_PPR_SUB": str(s),
                                                     "ANOMOD_PPR_RING": str(r)}
                     for s in (1, 2, 4) for r in (0, 1)})
BATCH_PATHS = {"K1": (1, {}), "K3": (3, {}), "K16-split": (16, {}),
               "K16-nosplit": (16, {"ANOMOD_PPR_SPLIT": "0"}),
               "K3-per_launch": (3, {"ANOMOD_PPR_MODE": "1"}),
               "K16-per_launch": (16, {"ANOMOD_PPR_MODE": "1"})}

_worst = {"ratio": 0.0, "where": ""}


@pytest.fixture(scope="module", autouse=True)
def report_largest_ratio():
    yield
    print(f"\npagerank exact: largest |x - x_ref| / bound = {_worst['ratio']:.4g} "
          f"({_worst['where']})")


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check(x, xr, g, iters, what):
    r = assert_elementwise(x, xr, elementwise_bound(g, iters), what)
    if r > _worst["ratio"]:
        _worst.update(ratio=r, where=what)


def _named(name):
    """[(index, label, p)] of the graph's named personalizations."""
    n = len(personalizations(name))
    return [(pi, label, p) for pi, (label, p) in enumerate(personalizations(name, EXTRA)[:n])]


def _single_cases(name, solve, what):
    """Fixed-iteration and tolerance solves of every named personalization
    through solve(p, iters, tol) -> (x, iterations done)."""
    g = graph_case(name)
    for pi, label, p in _named(name):
        for iters in FIXED_ITERS:
            x, done = solve(p, iters, 0.0)
            assert done == iters
            _check(x, ref_fixed(name, pi, iters, EXTRA), g, iters, f"{what} {name} {label} {iters}")
        tol, stop, xr = ref_tol(name, pi, EXTRA)
        x, done = solve(p, TOL_ITERS, tol)
        assert done == stop, f"{what} {name} {label} tol={tol}: stopped at {done}, reference {stop}"
        _check(x, xr, g, stop, f"{what} {name} {label} tol={tol}")


@pytest.mark.parametrize("name", CASES)
def test_one_shot(ctx, monkeypatch, name):
    """Context.pagerank: graph build, solve (default path) and release per call."""
    _set_env(monkeypatch, {})
    g = graph_case(name)
    _single_cases(name, lambda p, iters, tol: ctx.pagerank(g.row_ptr, g.col, g.w, p, ALPHA,
                                                           iters=iters, tol=tol), "one_shot")


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("path", list(SINGLE_PATHS))
def test_device_graph(ctx, monkeypatch, path, name):
    """DeviceGraph.pagerank per launch (hipGraph replay for fixed iterations,
    a read-back per launch in tolerance mode) and persistent, with 1, 2 or 4
    256-row blocks per workgroup, with and without the vector ring."""
    _set_env(monkeypatch, SINGLE_PATHS[path])
    g = graph_case(name)
    dg = anomod.DeviceGraph(ctx, g.row_ptr, g.col, g.w)
    assert (dg.N, dg.nnz) == (g.N, g.col.shape[0])

    def solve(p, iters, tol):
        out = dg.pagerank(p, ALPHA, iters=iters, tol=tol)
        expect = "persistent" if path != "per_launch" else "readback" if tol > 0 else "graph"
        assert dg.last_solve() == (expect, 0)
        return out

    try:
        _single_cases(name, solve, path)
    finally:
        dg.free()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("path", list(BATCH_PATHS))
def test_batch(ctx, monkeypatch, path, name):
    """pagerank_batch: every row of X against its own reference solve.  K = 16
    runs the split kernel, the two-block form (ANOMOD_PPR_SPLIT=0) and the
    per-launch loop; in tolerance mode every vector stops (is frozen) at its
    own reference iteration and the batch reports the latest."""
    K, env = BATCH_PATHS[path]
    _set_env(monkeypatch, env)
    g = graph_case(name)
    pis = tuple(range(K))
    P = np.stack([personalizations(name, EXTRA)[pi][1] for pi in pis])
    per_launch = env.get("ANOMOD_PPR_MODE") == "1"
    dg = anomod.DeviceGraph(ctx, g.row_ptr, g.col, g.w)
    try:
        for iters in FIXED_ITERS:
            X, done = dg.pagerank_batch(P, ALPHA, iters=iters)
            assert done == iters
            assert dg.last_solve() == ("graph" if per_launch else "persistent", 0)
            for k in pis:
                _check(X[k], ref_fixed(name, k, iters, EXTRA), g, iters,
                       f"batch-{path} {name} vector {k} {iters}")
        tol, stops, xs = ref_tol_batch(name, pis, EXTRA)
        X, done = dg.pagerank_batch(P, ALPHA, iters=TOL_ITERS, tol=tol)
        assert dg.last_solve() == ("readback" if per_launch else "persistent", 0)
        assert done == max(stops), f"batch-{path} {name} tol={tol}: {done} vs {stops}"
        for k in pis:
            _check(X[k], xs[k], g, stops[k], f"batch-{path} {name} vector {k} tol={tol}")
    finally:
        dg.free()


@pytest.mark.parametrize("name", SHARD_CASES)
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded(ctx, monkeypatch, shards, name):
    """pagerank_sharded over virtual row shards: 2 and 3 blocks split 2 and 3
    ways (one block per shard, two in one, an empty shard)."""
    _set_env(monkeypatch, {})
    g = graph_case(name)
    dg = anomod.DeviceGraph(ctx, g.row_ptr, g.col, g.w)
    try:
        _single_cases(name, lambda p, iters, tol: dg.pagerank_sharded(
            p, ALPHA, iters=iters, tol=tol, virtual_shards=shards), f"sharded-{shards}")
    finally:
        dg.free()

"""Reference for the PageRank solves (a plain helper, not a conftest).

pagerank_ref restates in numpy the arithmetic csrc/pagerank.hip documents:

* out-weights are summed in f64; a row whose out-weight is 0 (no edges, or
  only zero-weight edges) is dangling and its edges contribute nothing;
* every other edge weight is float32(float64(w) / outw), widened back
  (round_weights=False is the C oracle's model: the f64 quotient, and the
  dangling mass added up row after row as its loop does — with n dangling
  rows that running sum alone may be off by n roundings, more than the
  bound the two are compared under; the kernel's model sums it pairwise, as
  the kernels' reduction trees do);
* p is divided by its sum (eight interleaved add chains joined by a fixed
  tree, the order every solve entry uses), x0 = 1/N;
* y = alpha * (A^T x + dsum * p) + (1 - alpha) * p, dsum = the sum of x over
  the dangling rows; a row's in-edges are added in caller order;
* the L1 change of every iteration is kept, and a tolerance solve stops after
  the first iteration whose change is below N * tol.

The graphs and personalizations the host and GPU tests share are built here
from seeded generators (graph_case, personalizations)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

EPS52 = 2.0 ** -52
ALPHA = 0.85
TOL_ITERS = 150                      # most iterations a tolerance solve is given
TOL_CANDIDATES = (1e-6, 3e-7, 1e-7, 3e-8, 1e-8)
TOL_GUARD = 1e-6                     # no L1 change within this (relative) of N * tol


def edge_model(row_ptr, col, w, round_weights=True):
    """(src, wn, dangling): the caller of every edge, its normalised weight
    as an f64 array, and the dangling mask of the rows."""
    row_ptr = np.asarray(row_ptr, np.int64)
    N = row_ptr.shape[0] - 1
    w64 = np.asarray(w, np.float32).astype(np.float64)
    src = np.repeat(np.arange(N), np.diff(row_ptr))
    outw = np.zeros(N)
    np.add.at(outw, src, w64)        # f64, in edge order
    dangling = outw == 0.0
    wn = np.zeros(w64.shape[0])
    ok = ~dangling[src]
    wn[ok] = w64[ok] / outw[src[ok]]
    if round_weights:
        wn = wn.astype(np.float32).astype(np.float64)
    return src, wn, dangling


def personalization_sum(p, dtype=np.float64):
    """Sum of p in the order of the solve entries: chain j adds p[j], p[j + 8],
    ... in turn; the eight chains are joined by a fixed tree."""
    p = np.asarray(p, dtype)
    a = []
    for j in range(8):
        c = p[j::8]
        a.append(np.add.accumulate(c, dtype=dtype)[-1] if c.size else dtype(0))
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def pagerank_ref(row_ptr, col, w, p, alpha=ALPHA, iters=100, tol=0.0, dtype=np.float64,
                 round_weights=True):
    """(x, errs): the vector after len(errs) iterations and the L1 change of
    every iteration; stops early once errs[-1] < N * tol (tol > 0)."""
    N = len(row_ptr) - 1
    col = np.asarray(col, np.int64)[: int(row_ptr[-1])]
    src, wn, dangling = edge_model(row_ptr, col, np.asarray(w)[: col.shape[0]], round_weights)
    wn = wn.astype(dtype)
    p = np.asarray(p, np.float64).astype(dtype)
    p = p / personalization_sum(p, dtype)
    a = dtype(alpha)
    x = np.full(N, dtype(1) / dtype(N), dtype)
    errs = []
    for _ in range(iters):
        t = x[src] * wn
        if dtype is np.float64:      # sequential in edge order, like np.add.at
            s = np.bincount(col, weights=t, minlength=N) if col.size else np.zeros(N)
        else:
            s = np.zeros(N, dtype)
            np.add.at(s, col, t)
        if not dangling.any():
            dsum = dtype(0)
        elif round_weights:
            dsum = x[dangling].sum(dtype=dtype)
        else:                        # the oracle's running sum, row after row
            dsum = np.add.accumulate(x[dangling], dtype=dtype)[-1]
        y = a * (s + dsum * p) + (dtype(1) - a) * p
        errs.append(np.abs(y - x).sum(dtype=dtype))
        x = y
        if tol > 0.0 and errs[-1] < dtype(N) * dtype(tol):
            break
    return x, errs


def max_in_degree(g) -> int:
    return int(np.bincount(g.col, minlength=g.N).max()) if g.col.size else 0


def elementwise_bound(g, iters) -> float:
    """Relative bound per entry after `iters` iterations: one rounding per
    in-edge fma plus a constant for the row formula and the normalisation,
    every iteration (all terms are non-negative, so nothing cancels)."""
    return iters * (max_in_degree(g) + 16) * EPS52


def clears_guard(N, errs, tol) -> bool:
    """A tolerance solve with these L1 changes stopped before TOL_ITERS and
    none of its changes lies within TOL_GUARD (relative) of N * tol."""
    thr = N * tol
    e = np.asarray(errs, np.float64)
    return bool(len(errs) < TOL_ITERS and e[-1] < thr and (np.abs(e - thr) > TOL_GUARD * thr).all())


def pick_tol(errs_of):
    """The first candidate tolerance that clears the guard band for every
    sequence of L1 changes errs_of(tol) -> (N, [errs, ...]) returns: a
    condition on the reference's own sequences, so that a solve whose changes
    differ from them by rounding stops at the same iterations."""
    for tol in TOL_CANDIDATES:
        N, seqs = errs_of(tol)
        if all(clears_guard(N, errs, tol) for errs in seqs):
            return tol
    raise AssertionError("no tolerance candidate clears the guard band")


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
Graph = namedtuple("Graph", "name N row_ptr col w meta")

SIZES = (1, 2, 12, 46, 255, 256, 257, 513, 1024, 1279)
IN_DEGREES = (0, 1, 7, 8, 9, 16, 17)   # around the 8-wide edge batch
HUB_N = 5000
HUB_NODE = 777
KINDS = ("random", "indeg", "dangling", "ring", "loops", "wide", "zero")


def _csr(N, src, dst, w):
    """CSR of the edge list, rows by caller, a row's edges in list order."""
    src = np.asarray(src, np.int64)
    order = np.argsort(src, kind="stable")
    row_ptr = np.zeros(N + 1, np.uint32)
    np.cumsum(np.bincount(src, minlength=N), out=row_ptr[1:])
    return (row_ptr, np.asarray(dst, np.int64)[order].astype(np.uint32),
            np.asarray(w, np.float32)[order])


def _random_edges(rng, N, lo=1, hi=12, dangling=0.05):
    deg = rng.integers(lo, hi, N)
    deg[rng.random(N) < dangling] = 0
    if N >= 2:
        deg[rng.integers(N)] = 0     # at least one dangling row
    src = np.repeat(np.arange(N), deg)
    dst = rng.integers(0, N, src.size)
    if N >= 3:                       # at least one node nobody calls
        z = int(rng.integers(N))
        dst[dst == z] = (z + 1) % N
    return src, dst, rng.integers(1, 1000, src.size).astype(np.float32)


def _build(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    kind, _, arg = name.partition("-")
    meta = {}
    if kind == "hub":                # every caller of the hub is a distinct node
        N, indeg = HUB_N, int(arg)
        callers = np.delete(np.arange(N), HUB_NODE)[:indeg]
        src, dst, w = _random_edges(rng, N, 0, 5, 0.0)
        dst[dst == HUB_NODE] = HUB_NODE + 1
        src = np.r_[src, callers]
        dst = np.r_[dst, np.full(indeg, HUB_NODE)]
        w = np.r_[w, rng.integers(1, 1000, indeg).astype(np.float32)]
        meta["hub"] = (HUB_NODE, indeg)
        return Graph(name, N, *_csr(N, src, dst, w), meta)
    N = int(arg.split("-")[0])
    if kind == "random":
        src, dst, w = _random_edges(rng, N)
    elif kind == "indeg":
        # target nodes with an exact in-degree (parallel edges where N is
        # small); the last row of the last block always is one.  N >= 8: all
        # of IN_DEGREES in one graph; below, one graph per in-degree.
        if N >= 8:
            others = rng.permutation(N - 1)[: len(IN_DEGREES) - 1]
            targets = dict(zip(np.r_[N - 1, others].tolist(),
                               (9,) + tuple(d for d in IN_DEGREES if d != 9)))
        else:
            targets = {N - 1: int(arg.split("-")[1])}
        src, dst = [], []
        for v in range(N):
            d = targets.get(v, int(rng.integers(0, 4)))
            src += rng.integers(0, N, d).tolist()
            dst += [v] * d
        w = rng.integers(1, 1000, len(src)).astype(np.float32)
        meta["targets"] = targets
    elif kind == "dangling":
        src, dst, w = [], [], []
    elif kind == "ring":
        src, dst = np.arange(N), (np.arange(N) + 1) % N
        w = rng.integers(1, 1000, N).astype(np.float32)
    elif kind == "loops":            # self-loops and duplicated (u, v) edges
        src, dst, w = _random_edges(rng, N)
        loops = np.nonzero(rng.random(N) < 0.5)[0] if N > 1 else np.arange(1)
        first = np.unique(src, return_index=True)[1]   # each row's first edge, twice more
        src = np.r_[src, loops, src[first], src[first]]
        dst = np.r_[dst, loops, dst[first], dst[first]]
        w = np.r_[w, rng.integers(1, 1000, loops.size + 2 * first.size).astype(np.float32)]
    elif kind == "wide":             # weights from 1 to 2^24 in one row
        src, dst, w = _random_edges(rng, N, 2, 12)
        w = np.exp2(rng.integers(0, 25, src.size)).astype(np.float32)
        first = np.unique(src, return_index=True)[1]
        w[first], w[first + 1] = 1.0, 2.0 ** 24
    elif kind == "zero":
        # rows whose weights are all 0.0 among normal rows, and a zero-weight
        # edge inside a normal row
        src, dst, w = _random_edges(rng, N, 2, 12)
        rows, first = np.unique(src, return_index=True)
        zero_rows = rows[rng.random(rows.size) < 0.25]
        if rows.size:
            zero_rows = np.union1d(zero_rows, rows[:1])
        w[np.isin(src, zero_rows)] = 0.0
        normal = first[~np.isin(rows, zero_rows)]
        w[normal] = 0.0              # the first edge of every normal row
        meta["zero_rows"] = zero_rows
    else:
        raise KeyError(name)
    return Graph(name, N, *_csr(N, src, dst, w), meta)


@functools.lru_cache(maxsize=None)
def graph_case(name) -> Graph:
    g = _build(name)
    for a in (g.row_ptr, g.col, g.w):
        a.setflags(write=False)
    return g


def case_names(sizes=SIZES, hubs=True):
    out = []
    for N in sizes:
        for kind in KINDS:
            if kind == "indeg" and N < 8:
                out += [f"indeg-{N}-{d}" for d in IN_DEGREES]
            else:
                out.append(f"{kind}-{N}")
    if hubs:
        out += ["hub-4096", "hub-4999"]
    return out


@functools.lru_cache(maxsize=None)
def personalizations(name, extra=0):
    """[(label, p)]: dense, half zeros, one-hot on a dangling node and on a
    node without in-edges (where the graph has one), then `extra` more random
    vectors with 30 % zeros (to fill a batch)."""
    g = graph_case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    dense = rng.random(g.N) + 1e-3
    out = [("dense", dense)]
    if g.N > 1:
        half = dense.copy()
        half[rng.permutation(g.N)[: (g.N + 1) // 2]] = 0.0
        out.append(("half", half))
    _, _, dangling = edge_model(g.row_ptr, g.col, g.w)
    indeg = np.bincount(g.col, minlength=g.N)
    for label, nodes in (("onehot_dangling", np.nonzero(dangling)[0]),
                         ("onehot_no_in_edge", np.nonzero(indeg == 0)[0])):
        if nodes.size:
            q = np.zeros(g.N)
            q[nodes[-1]] = 1.0
            out.append((label, q))
    for k in range(extra):
        q = rng.random(g.N) + 1e-3
        q[rng.random(g.N) < 0.3] = 0.0
        q[rng.integers(g.N)] = 0.5
        out.append((f"extra{k}", q))
    for _, q in out:
        q.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ref_fixed(name, pi, iters, extra=0):
    """The float-weight f64 reference after `iters` iterations."""
    g = graph_case(name)
    x, _ = pagerank_ref(g.row_ptr, g.col, g.w, personalizations(name, extra)[pi][1], ALPHA, iters)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_tol_batch(name, pis, extra=0):
    """(tol, stopping iterations, vectors there) of the float-weight f64
    reference for the personalizations `pis` under one tolerance, chosen by
    pick_tol on all their sequences."""
    g = graph_case(name)
    ps = [personalizations(name, extra)[pi][1] for pi in pis]
    runs = {}

    def errs_of(tol):
        runs[tol] = [pagerank_ref(g.row_ptr, g.col, g.w, p, ALPHA, TOL_ITERS, tol) for p in ps]
        return g.N, [errs for _, errs in runs[tol]]

    tol = pick_tol(errs_of)
    for x, _ in runs[tol]:
        x.setflags(write=False)
    return tol, tuple(len(errs) for _, errs in runs[tol]), tuple(x for x, _ in runs[tol])


def ref_tol(name, pi, extra=0):
    """(tol, stopping iteration, x there) for one personalization."""
    tol, stops, xs = ref_tol_batch(name, (pi,), extra)
    return tol, stops[0], xs[0]


def assert_elementwise(x, xr, bound, what=""):
    """|x - xr| <= bound * xr per entry, exact zeros where xr is zero; NaN
    fails.  Returns the largest |x - xr| / (bound * xr)."""
    x, xr = np.asarray(x, np.float64), np.asarray(xr, np.float64)
    assert x.shape == xr.shape, what
    zero = xr == 0.0
    bad = np.nonzero(zero & ~(x == 0.0))[0]
    assert bad.size == 0, f"{what}: x[{bad[0]}] = {x[bad[0]]!r} where the reference is 0"
    nz = ~zero
    ratio = np.abs(x[nz] - xr[nz]) / (bound * xr[nz])
    ok = ratio <= 1.0                # NaN compares false
    if not ok.all():
        i = np.nonzero(nz)[0][np.nonzero(~ok)[0][0]]
        raise AssertionError(f"{what}: x[{i}] = {x[i]!r}, reference {xr[i]!r}, "
                             f"|diff| / bound = {abs(x[i] - xr[i]) / (bound * xr[i])!r} "
                             f"({int((~ok).sum())} entries over the bound)")
    return float(ratio.max()) if ratio.size else 0.0

"""EWMA/z reference in double-double, the error bound the kernels are held to,
and the adversarial series matrix (events at the kernels' borders).

Recurrence (oracle/spec.py ewma_state + window_scores_from_state, the C
oracle's oracle_ewma_z): a NaN sample is missing (state carried, z = 0); the
first valid sample starts the state (m = x, v = 0, z = 0); otherwise
    d = x - m,  z = d / sqrt(v + eps),  m += alpha d,  v = (1 - alpha)(v + alpha d^2)
and a window's score is max |z| over its W steps.

Reference.  (m, v) are kept as unevaluated sums hi + lo of two f64 (error-free
transformations: Knuth two-sum, Dekker/Veltkamp two-product — numpy has no
fma), ~106 bits, vectorised over the series.  The mean is held as its offset
from the series' first sample r (m = r + mu, mu' = mu + alpha d, d = (x - r) -
mu with x - r exact): the same recurrence, but d keeps its 106 bits relative
to the signal around r, not to a large mean it cancels against (at a mean of
1e7 and d ~ 1 a double-double m would leave d, and so v, at 1e-25 relative).
The inputs are what the C ABI
receives: the f32 samples widened exactly, alpha = f64(f32(alpha)),
eps = f64(f32(eps)); 1 - alpha is carried as a double-double (exact).  z is
formed in f64 from the rounded d and v + eps, a few 2^-53 relative — noise
beside the f32 bound below.  tests/test_ewma_ref_host.py holds the state to
1e-25 relative against a 60-digit mpmath run of the same recurrence.

Bound.  Per step, u32 = 2^-24 (f32 unit roundoff), u64 = 2^-53:

    |z_kernel - z_ref| <= C1 u32 |z_ref| + C2 (u64/alpha) xmax_t / sqrt(v_ref + eps) + tiny

xmax_t = the largest |x| of the series up to and including step t (m is a
convex combination of the samples, so |m| <= xmax_t and |d| <= 2 xmax_t),
tiny = 2^-126 (the smallest normal f32; below it f32 results may be flushed).

C1 = 5, the f32 part, z = (float)d * rsq((float)v + eps) (ewma.hip zscale), in
units of u32 relative to |z|:
    (float)d                          1     one rounding of d
    (float)v                          1/2   one rounding of v, halved by the
                                            exponent -1/2 of the rsqrt
    the f32 add (float)v + eps        1/2   one rounding, halved likewise
    v_rsq_f32, 1 ulp = 2 u32          2     (the kernel's comment: 1 ulp)
    the f32 multiply                  1
Every entry needs its operand normal in f32: |d| <= 2^63 and v <= 2^126 <
FLT_MAX on the documented domain |x| <= 2^62, and (float)v + eps >= eps >=
2^-126 by the entry point's precondition; (float)v itself may be denormal,
its absolute rounding error 2^-150 is then <= u32 eps, the same 1/2 entry.

C2 = 4, the f64 part.  One step rounds d = x - m (<= u64 |d| <= 2 u64 xmax)
and m' = fma(alpha, d, m) (<= u64 |m'| <= u64 xmax); through m' = m + alpha d
the rounding of d enters scaled by alpha, so a step adds at most
u64 xmax (1 + 2 alpha) <= 3 u64 xmax to the error of m, and the error already
there is multiplied by beta = 1 - alpha per step: the accumulated error of m is
at most 3 u64 xmax / alpha.  The time-parallel fold rounds M, A delta and the
sum once more per sub-chunk (terms of the size of the signal around x_f), one
further u64 xmax that decays like the rest: C2 = 4.  The error of m is an
error of d of the same size, divided by sqrt(v + eps) in z.  The same error
reaches v through d^2 and v's own roundings add O(u64/alpha) relative; both
change z by a relative O(u64/alpha) (xmax/sqrt(v)) |z| — second order next to
the two terms wherever the second term is below |z|, and left to them.
The constants come from this arithmetic, not from a GPU run; the host tests
hold f64 emulations of both kernel forms to the bound on every family.

A window's bound is the maximum of its steps' bounds: |max a - max b| <=
max |a - b|.
"""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass, field

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
C1 = 5.0
C2 = 4.0
TINY = 2.0 ** -126
S_COLS = 130  # two full 64-lane strips and a 2-lane partial wave

_SPLIT = 134217729.0  # 2^27 + 1


# ---------------------------------------------------------------- double-double
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fast_two_sum(a, b):  # |a| >= |b|
    s = a + b
    return s, b - (s - a)


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ah, al, bh, bl):
    s, e = _two_sum(ah, bh)
    t, f = _two_sum(al, bl)
    s, e = _fast_two_sum(s, e + t)
    return _fast_two_sum(s, e + f)


def dd_mul(ah, al, bh, bl):
    p, e = _two_prod(ah, bh)
    return _fast_two_sum(p, e + (ah * bl + al * bh))


# ------------------------------------------------------------------- reference
@dataclass
class Ref:
    z: np.ndarray        # [T][S] f64 per-step z (0 where the step scores nothing)
    Z: np.ndarray        # [T/W][S] window maxima of |z| (non-finite once a step is)
    upd: np.ndarray      # [T][S] bool: the step scored (valid sample on a started state)
    v_prev: np.ndarray   # [T][S] v entering the step (hi part)
    xmax: np.ndarray     # [T][S] largest |x| seen up to and including the step
    m_hi: np.ndarray     # [T][S] state after the step, hi + lo (NaN before the first sample)
    m_lo: np.ndarray
    v_hi: np.ndarray
    v_lo: np.ndarray
    alpha: float
    eps: float
    W: int


def abi_f32(x: float) -> float:
    """The f64 value of the f32 the C ABI receives for a Python float."""
    with np.errstate(over="ignore", under="ignore"):
        return float(np.float32(x))


def ewma_ref(X: np.ndarray, alpha: float, W: int, eps: float = 1e-12,
             f32_args: bool = True) -> Ref:
    """f32_args: alpha and eps as the kernels' C ABI rounds them (f32); False
    for the f64 oracles, which take them as given."""
    X = np.asarray(X)
    assert X.dtype == np.float32 and X.ndim == 2 and X.shape[0] % W == 0
    T, S = X.shape
    a = abi_f32(alpha) if f32_args else float(alpha)
    e = abi_f32(eps) if f32_args else float(eps)
    bh, bl = _two_sum(1.0, -a)  # 1 - alpha, exact
    r = np.zeros(S)   # the series' first sample; the state holds m - r
    mh = np.zeros(S)
    ml = np.zeros(S)
    vh = np.zeros(S)
    vl = np.zeros(S)
    started = np.zeros(S, bool)
    xm = np.zeros(S)
    out = {k: np.empty((T, S)) for k in ("z", "v_prev", "xmax", "m_hi", "m_lo", "v_hi", "v_lo")}
    upd_all = np.empty((T, S), bool)
    zero = np.zeros(S)
    with np.errstate(all="ignore"):
        for t in range(T):
            x = X[t].astype(np.float64)
            valid = x == x
            upd = valid & started
            init = valid & ~started
            xm = np.where(valid, np.maximum(xm, np.abs(x)), xm)
            xh, xl = _two_sum(x, -r)  # exact
            dh, dl = dd_add(xh, xl, -mh, -ml)
            sh, _ = dd_add(vh, vl, e, 0.0)
            out["z"][t] = np.where(upd, (dh + dl) / np.sqrt(sh), 0.0)
            out["v_prev"][t] = vh
            out["xmax"][t] = xm
            upd_all[t] = upd
            adh, adl = dd_mul(dh, dl, a, 0.0)
            m1h, m1l = dd_add(mh, ml, adh, adl)
            qh, ql = dd_mul(adh, adl, dh, dl)
            th, tl = dd_add(vh, vl, qh, ql)
            v1h, v1l = dd_mul(th, tl, bh, bl)
            r = np.where(init, x, r)
            mh = np.where(init, 0.0, np.where(upd, m1h, mh))
            ml = np.where(init, 0.0, np.where(upd, m1l, ml))
            vh = np.where(init, 0.0, np.where(upd, v1h, vh))
            vl = np.where(init, 0.0, np.where(upd, v1l, vl))
            started = started | valid
            fh, fl = dd_add(r, zero, mh, ml)
            out["m_hi"][t] = np.where(started, fh, np.nan)
            out["m_lo"][t] = np.where(started, fl, np.nan)
            out["v_hi"][t] = np.where(started, vh, np.nan)
            out["v_lo"][t] = np.where(started, vl, np.nan)
        Z = np.abs(out["z"]).reshape(T // W, W, S).max(axis=1)  # NaN/inf propagate
    return Ref(z=out["z"], Z=Z, upd=upd_all, v_prev=out["v_prev"], xmax=out["xmax"],
               m_hi=out["m_hi"], m_lo=out["m_lo"], v_hi=out["v_hi"], v_lo=out["v_lo"],
               alpha=a, eps=e, W=W)


def step_bound(ref: Ref, c1: float = C1, c2: float = C2) -> np.ndarray:
    """[T][S] bound on |z_kernel - z_ref| per step (NaN where z_ref is non-finite)."""
    with np.errstate(all="ignore"):
        f64 = c2 * U64 / ref.alpha * ref.xmax / np.sqrt(ref.v_prev + ref.eps)
        b = np.where(ref.upd, c1 * U32 * np.abs(ref.z) + f64, 0.0) + TINY
    return np.where(np.isfinite(ref.z), b, np.nan)


def window_bound(ref: Ref, c1: float = C1, c2: float = C2) -> np.ndarray:
    """[T/W][S]: the largest step bound of each window (NaN: a non-finite step)."""
    b = step_bound(ref, c1, c2)
    T, S = b.shape
    return b.reshape(T // ref.W, ref.W, S).max(axis=1)


def compare(got: np.ndarray, want: np.ndarray, bound: np.ndarray):
    """(worst error/bound over the compared cells, mask of the cells left out).
    A cell is left out only where the reference (or its bound) is non-finite;
    a non-finite `got` in a compared cell gives ratio inf."""
    got = np.asarray(got, np.float64)
    skip = ~(np.isfinite(want) & np.isfinite(bound))
    with np.errstate(all="ignore"):
        r = np.abs(got - want) / bound
    r = np.where(np.isfinite(got), r, np.inf)
    r = np.where(skip, 0.0, r)
    return r, skip


# ------------------------------------------------------------ kernel geometry
def tp_sub_chunk(W: int) -> int:
    """U of the time-parallel kernel: the most whole windows in its register block."""
    assert 1 <= W <= 128
    cap = 64 if W <= 64 else 128
    return W * (cap // W)


TP_WAVES = 12


def borders(mode: int, W: int, T: int, seg: int = 960, layout: str = "mixed") -> tuple[int, ...]:
    """Steps below T at which the kernel of `mode` changes tile, load block,
    launch segment, sub-chunk or super-chunk (the first of each kind, every
    launch segment / super-chunk start, and the start of a partial last block).
    The first load block of a series is never dense (it holds the first
    sample), so the "dense" layout takes the tile border at 80 (inside the
    second block) and the block border at 128 instead of 16 and 64."""
    if mode == 1:
        b = ({80, 128} if layout == "dense" else {16, 64}) | set(range(seg, T, seg))
        if T % 64:
            b.add(T // 64 * 64)
    elif mode == 3:
        b = {32, 64}
        if T % 32:
            b.add(T // 32 * 32)
    else:  # time-parallel (auto picks it at S_COLS series)
        U = tp_sub_chunk(W)
        b = {U} | set(range(TP_WAVES * U, T, TP_WAVES * U))
    return tuple(sorted(x for x in b if 1 < x < T - 1))


# --------------------------------------------------------------- input builder
EVENT_FAMILIES = ("outlier", "shift", "const_step", "first_late", "nan_run_start", "nan_run_end",
                  "inf")
PLAIN_FAMILIES = ("benign", "mean1e7", "scale1e-20", "scale1e15", "alt2^62", "nan60", "all_nan")
FAMILIES = PLAIN_FAMILIES + EVENT_FAMILIES
NAN_RUN = 131  # longer than the largest sub-chunk (128)


@dataclass
class Matrix:
    X: np.ndarray                    # [T][S_COLS] f32
    family: list = field(default_factory=list)   # per column
    event: list = field(default_factory=list)    # per column: event step or None
    borders: tuple = ()

    def cols(self, fam: str) -> np.ndarray:
        return np.array([i for i, f in enumerate(self.family) if f == fam], np.int64)


def _column(fam: str, p, T: int, rng) -> np.ndarray:
    mu = float(rng.uniform(-50.0, 1000.0))
    sg = float(rng.uniform(0.5, 30.0))
    g = rng.standard_normal(T)
    x = mu + sg * g
    if fam == "benign":
        pass
    elif fam == "mean1e7":  # integers near 1e7: every sample on the f32 grid (spacing 1)
        x = 1.0e7 + np.rint(3.0 * g)
    elif fam == "scale1e-20":
        x = 1e-20 * (0.5 + g)
    elif fam == "scale1e15":
        x = 1e15 * (0.5 + g)
    elif fam == "alt2^62":  # the edge of the documented domain
        x = 2.0 ** 62 * np.where(np.arange(T) % 2 == 0, 1.0, -1.0)
    elif fam == "nan60":
        x[rng.random(T) < 0.6] = np.nan
    elif fam == "all_nan":
        x[:] = np.nan
    elif fam == "outlier":
        x[p] = mu + 1e6 * sg
    elif fam == "shift":
        x[p:] += 1e5 * sg
    elif fam == "const_step":  # v = 0 until the step
        x = np.where(np.arange(T) < p, mu, mu + 7.0 * sg)
    elif fam == "first_late":
        x[:p] = np.nan
    elif fam == "nan_run_start":
        x[p:p + NAN_RUN] = np.nan
    elif fam == "nan_run_end":  # the first sample after the run is step p
        x[max(p - NAN_RUN, 1):p] = np.nan
    elif fam == "inf":
        x[p] = np.inf
    else:
        raise ValueError(fam)
    return x.astype(np.float32)


NAN_FREE_PLAIN = ("mean1e7", "scale1e-20", "scale1e15", "alt2^62", "benign")
DENSE_EVENTS = ("outlier", "shift", "const_step", "inf")   # no NaN: the block stays dense
SWITCH_EVENTS = ("nan_run_start", "nan_run_end")           # a NaN run: dense -> general -> dense


def _extra(f: str, i: int, places: list):
    return (f, places[(3 * i + 1) % len(places)] if f in EVENT_FAMILIES else None)


def _plan_mixed(places: list, rot: int) -> list:
    """Lanes of one wave diverge: one column of every family, then for every
    placement the seven event families side by side, then the plain families;
    a plan shorter than 128 starts over (fresh noise), so every family sits in
    both strips.  The partial wave holds families 2 rot, 2 rot + 1 (mod 14)."""
    plan = [_extra(f, i, places) for i, f in enumerate(FAMILIES)]
    plan += [(f, p) for p in places for f in EVENT_FAMILIES]
    plan += [(f, None) for f in PLAIN_FAMILIES]
    assert len(plan) <= 128, len(plan)  # up to five borders
    plan = [plan[i % len(plan)] for i in range(128)]
    return plan + [_extra(FAMILIES[(2 * rot + k) % len(FAMILIES)], rot + k, places)
                   for k in (0, 1)]


def _plan_dense(places: list, rot: int) -> list:
    """Homogeneous strips for the tiled kernel's dense path (taken by a
    64-step block when every lane of the wave has started and none holds a
    NaN).  Strip 0: NaN-free families only, their events at every placement,
    so the dense step scores them.  Strip 1: the only NaNs are the NaN runs
    that start or end at the placements (benign otherwise), so the wave
    leaves the dense path around every border and returns to it.  The
    partial wave holds two NaN-free plain families."""
    s0 = [(f, p) for f in DENSE_EVENTS for p in places]
    s0 += [(f, None) for f in NAN_FREE_PLAIN[:64 - len(s0)]]
    s1 = [(f, p) for f in SWITCH_EVENTS for p in places]
    assert len(s0) <= 64 and len(s1) <= 64
    s0 += [("benign", None)] * (64 - len(s0))
    s1 += [("benign", None)] * (64 - len(s1))
    return s0 + s1 + [(NAN_FREE_PLAIN[(2 * rot + k) % len(NAN_FREE_PLAIN)], None) for k in (0, 1)]


@functools.lru_cache(maxsize=None)
def build_matrix(bord: tuple, T: int, rot: int = 0, layout: str = "mixed",
                 seed: int = 0) -> Matrix:
    """One [T][130] matrix, a column per (family, placement): every event of
    the layout's families at b - 1, b and b + 1 for every border b."""
    places = [b + k for b in bord for k in (-1, 0, 1)]
    assert all(0 < p < T for p in places)
    plan = {"mixed": _plan_mixed, "dense": _plan_dense}[layout](places, rot)
    assert len(plan) == S_COLS
    rng = np.random.default_rng(1000 * seed + 7 * T + rot + (500 if layout == "dense" else 0))
    X = np.stack([_column(f, p, T, rng) for f, p in plan], axis=1)
    return Matrix(X=np.ascontiguousarray(X), family=[f for f, _ in plan],
                  event=[p for _, p in plan], borders=tuple(bord))


def launches(T: int, seg: int) -> list:
    """(start, steps) of the tiled kernel's launches over T (seg = 0: one)."""
    seg = seg or T
    return [(t0, min(seg, T - t0)) for t0 in range(0, T, seg)]


def dense_blocks(X: np.ndarray, runs: list) -> np.ndarray:
    """ewma_zt_kernel's dense predicate restated: [waves][T // 64] int8, 1 where
    the 64-step block runs the dense step, 0 the general one, -1 where the
    block is not a whole block of its launch.  `runs` = launches (start a
    multiple of 64); the state carries from one to the next.  A block is dense
    when every lane of the wave has seen a sample before it and no lane's f32
    sum of the block is NaN (a NaN sample, or +inf and -inf together)."""
    T, S = X.shape
    nw = (S + 63) // 64
    out = np.full((nw, T // 64), -1, np.int8)
    nan = np.isnan(X)
    seen_before = np.vstack([np.zeros((1, S), bool), np.cumsum(~nan, axis=0)[:-1] > 0])
    for t0, Ts in runs:
        assert t0 % 64 == 0
        for b0 in range(t0, t0 + Ts - 63, 64):
            blk = X[b0:b0 + 64]
            bad = nan[b0:b0 + 64].any(axis=0) | ((blk == np.inf).any(axis=0)
                                                 & (blk == -np.inf).any(axis=0))
            for w in range(nw):
                ln = slice(64 * w, min(64 * w + 64, S))
                out[w, b0 // 64] = seen_before[b0, ln].all() and not bad[ln].any()
    return out


@functools.lru_cache(maxsize=None)
def scaled_matrix(scale: float, T: int, seed: int = 0) -> Matrix:
    """130 noise series of magnitude `scale` (1e-21: v ~ 1e-42, an f32
    denormal), every fourth with 30 % of its samples missing."""
    rng = np.random.default_rng(77 + seed)
    x = scale * (rng.uniform(-2.0, 2.0, S_COLS) + rng.uniform(0.5, 2.0, S_COLS)
                 * rng.standard_normal((T, S_COLS)))
    x[:, ::4] = np.where(rng.random((T, (S_COLS + 3) // 4)) < 0.3, np.nan, x[:, ::4])
    return Matrix(X=np.ascontiguousarray(x.astype(np.float32)), family=["tiny"] * S_COLS,
                  event=[None] * S_COLS, borders=())


def expected_skips(mx: Matrix, W: int | None = None) -> np.ndarray:
    """Per column, the number of cells whose reference is non-finite: none,
    except from the inf of the inf family on (steps, or windows when W is given)."""
    T = mx.X.shape[0]
    out = np.zeros(len(mx.family), np.int64)
    for i, (f, p) in enumerate(zip(mx.family, mx.event)):
        if f == "inf":
            out[i] = T - p if W is None else T // W - p // W
    return out


# ------------------------------------------------ the cases of the GPU tests
@dataclass(frozen=True)
class Case:
    name: str
    mode: int
    W: int
    T: int
    alpha: float
    eps: float
    rot: int
    seg: int = 960      # ANOMOD_EWMA_SEG of a tiled run (a multiple of lcm(W, 64), or >= T)
    scale: float = 0.0  # != 0: the tiny-magnitude matrix instead of the families
    layout: str = "mixed"

    @property
    def borders(self):
        return borders(self.mode, self.W, self.T, self.seg, self.layout)

    def matrix(self) -> Matrix:
        if self.scale:
            return scaled_matrix(self.scale, self.T, self.rot)
        return build_matrix(self.borders, self.T, self.rot, self.layout)


_GEOM = {1: 2400, 2: 1920, 3: 1920, 0: 1920}
MODE_CASES = tuple(
    Case(f"mode{m}-eps{e:g}", m, 60, _GEOM[m], 2 / 61, e, rot)
    for rot, (m, e) in enumerate((m, e) for m in (1, 2, 3, 0) for e in (1e-12, 1e-2)))
BLOCK_CASES = tuple(
    Case(f"W{W}", 2, W, T, 2 / (W + 1) if W > 1 else 0.3, 1e-2 if W == 6 else 1e-12, rot)
    for rot, (W, T) in enumerate(((1, 1920), (6, 1920), (33, 1980), (64, 1920), (65, 1950),
                                  (96, 1920), (128, 3840))))
ALPHA_CASES = tuple(
    Case(f"mode{m}-alpha{a:g}", m, 60, _GEOM[m], a, 1e-12, rot)
    for rot, (m, a) in enumerate((m, a) for m in (1, 2) for a in (1e-4, 0.9, 1.0)))
# the tiled kernel above the time-parallel kernel's W: one launch (lcm(150, 64) = 4800 > T),
# windows that end inside a float4 (W % 4 != 0: the window end is checked at every step)
W150_CASES = tuple(Case(f"W150-{lay}", 1, 150, 2400, 2 / 151, 1e-12, 5, seg=4800, layout=lay)
                   for lay in ("mixed", "dense"))
# the dense layout for every tiled case
DENSE_CASES = tuple(dataclasses.replace(c, name=c.name + "-dense", layout="dense")
                    for c in MODE_CASES + ALPHA_CASES if c.mode == 1)
TILED_CASES = tuple(c for c in MODE_CASES + ALPHA_CASES if c.mode == 1) + DENSE_CASES + W150_CASES
BOUND_CASES = MODE_CASES + BLOCK_CASES + ALPHA_CASES + DENSE_CASES + W150_CASES
# v + eps at the edge of the entry point's precondition eps >= 2^-126: (float)v
# is an f32 denormal, the sum the smallest normal
EPS_MIN = 2.0 ** -126
DENORMAL_CASES = tuple(Case(f"tiny-mode{m}-eps2^-126", m, 60, 960, 2 / 61, EPS_MIN, m, scale=1e-21)
                       for m in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def case_ref(case: Case):
    """(matrix, reference, window bound) of a case, computed once per process."""
    mx = case.matrix()
    ref = ewma_ref(mx.X, case.alpha, case.W, case.eps)
    return mx, ref, window_bound(ref)


# ------------------------------------------- f64 emulations of the kernel forms
# Plain f64 without fma, f32 1/sqrt: the arithmetic of ewma.hip restated in
# numpy, vectorised over the series.  They are evidence for the bound on a
# machine without a GPU (the reference alone stays inside it, the transfer
# algebra included), not a model of the kernels' bits.
def _emu_step(m, v, n, x32, a, b, eps32):
    """ewma_step_bf.  Returns z (f32) and the new (m, v, n)."""
    valid = x32 == x32
    init = valid & (n == 0)
    upd = valid & (n != 0)
    xd = x32.astype(np.float64)
    d = xd - m
    zr = d.astype(np.float32) * (np.float32(1.0) / np.sqrt(v.astype(np.float32) + eps32))
    z = np.where(upd, zr, np.float32(0.0))
    m1 = m + a * d
    v1 = b * (v + (a * d) * d)
    m = np.where(init, xd, np.where(upd, m1, m))
    v = np.where(init, 0.0, np.where(upd, v1, v))
    return z, m, v, n + valid


def _emu_windows(z: np.ndarray, W: int) -> np.ndarray:
    T, S = z.shape  # fmaxf drops a NaN operand
    return np.fmax.reduce(np.abs(z).reshape(T // W, W, S), axis=1, initial=np.float32(0.0))


def emulate_sequential(X: np.ndarray, alpha: float, W: int, eps: float, state=np.float64):
    """The sequential kernels (tiles, rows): per-step z [T][S] f32 and windows.
    state=np.float32 is a deliberately wrong kernel (for the bound's own test)."""
    T, S = X.shape
    a = abi_f32(alpha)
    b = 1.0 - a
    eps32 = np.float32(eps)
    m, v, n = np.zeros(S), np.zeros(S), np.zeros(S, np.int64)
    z = np.empty((T, S), np.float32)
    with np.errstate(all="ignore"):
        for t in range(T):
            z[t], m, v, n = _emu_step(m, v, n, X[t], a, b, eps32)
            m, v = m.astype(state).astype(np.float64), v.astype(state).astype(np.float64)
        return z, _emu_windows(z, W)


def emulate_time_parallel(X: np.ndarray, alpha: float, W: int, eps: float, q1_sign=-2.0):
    """ewma_tp_kernel: phase A (the transfer of every sub-chunk of U steps),
    the fold (apply_transfer) in time order, phase C from the folded state.
    q1_sign != -2 is a deliberately wrong algebra (for the bound's own test)."""
    T, S = X.shape
    U = tp_sub_chunk(W)
    a = abi_f32(alpha)
    b = 1.0 - a
    eps32 = np.float32(eps)
    m, v, n = np.zeros(S), np.zeros(S), np.zeros(S, np.int64)
    z = np.empty((T, S), np.float32)
    with np.errstate(all="ignore"):
        for tw in range(0, T, U):
            cnt = min(U, T - tw)
            # phase A
            xf, M, A = np.zeros(S), np.zeros(S), np.ones(S)
            Q0, Q1, Q2 = np.zeros(S), np.zeros(S), np.zeros(S)
            c = np.zeros(S, np.int64)
            seen = np.zeros(S, bool)
            for u in range(cnt):
                xv = X[tw + u]
                valid = xv == xv
                upd = valid & seen
                first = valid & ~seen
                xd = xv.astype(np.float64)
                d = xd - M
                ad = a * d
                q0 = b * (ad * d + Q0)
                q1 = b * ((q1_sign * ad) * A + Q1)
                q2 = b * ((a * A) * A + Q2)
                Q0 = np.where(upd, q0, Q0)
                Q1 = np.where(upd, q1, Q1)
                Q2 = np.where(upd, q2, Q2)
                M = np.where(first, xd, np.where(upd, M + ad, M))
                xf = np.where(first, xd, xf)
                A = np.where(upd, A * b, A)
                c = c + upd
                seen = seen | valid
            # phase C from the state entering the sub-chunk
            mc, vc, nc = m, v, n
            for u in range(cnt):
                z[tw + u], mc, vc, nc = _emu_step(mc, vc, nc, X[tw + u], a, b, eps32)
            # apply_transfer
            fresh = n == 0
            d = xf - m
            m1 = m + a * d
            v1 = np.where(fresh, 0.0, b * (v + (a * d) * d))
            delta = np.where(fresh, 0.0, m1 - xf)
            mn = M + A * delta
            vn = A * v1 + ((Q2 * delta + Q1) * delta + Q0)
            m = np.where(seen, mn, m)
            v = np.where(seen, vn, v)
            n = np.where(seen, n + 1 + c, n)
        return z, _emu_windows(z, W)

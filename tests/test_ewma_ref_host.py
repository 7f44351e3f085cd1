"""EWMA/z reference, host side (no GPU): tests/ewma_ref.py against a 60-digit
mpmath run of the same recurrence, the existing oracles tied to it, f64
emulations of both kernel forms held to the bound on every case of
tests/test_gpu_ewma_bound.py, and the premises its matrix builder claims."""
import math

import mpmath
import numpy as np
import pytest

import ewma_ref as R
from oracle import native, spec


def _ids(cases):
    return [c.name for c in cases]


def _family_worst(mx, ratio):
    """Worst ratio per family (for the failure message)."""
    fam = np.array(mx.family)
    return {f: float(ratio[..., fam == f].max()) for f in sorted(set(mx.family))}


# ------------------------------------------------- reference against mpmath
def _mp_run(x, alpha, dps=60):
    """(m, v) after every step of one series, mpmath at `dps` digits."""
    with mpmath.workdps(dps):
        a = mpmath.mpf(alpha)
        b = 1 - a
        m = v = None
        out = []
        for xv in x:
            xv = float(xv)
            if not math.isnan(xv):
                if m is None:
                    m, v = mpmath.mpf(xv), mpmath.mpf(0)
                else:
                    d = mpmath.mpf(xv) - m
                    m = m + a * d
                    v = b * (v + a * d * d)
            out.append((m, v))
        return out


@pytest.mark.parametrize("alpha", [2 / 61, 1e-4, 0.9, 1.0])
def test_reference_equals_mpmath_60_digits(alpha):
    """One column per family, 600 steps: hi + lo of the double-double state
    within 1e-25 relative of the 60-digit run.  The floor 1e-290 is the f64
    range: at alpha = 0.9 a constant series' v decays below it (the lo part
    underflows), far under anything the bound or a score can see."""
    mx = R.build_matrix((60, 300), 600, rot=3)
    cols = [int(mx.cols(f)[0]) for f in R.FAMILIES]
    X = np.ascontiguousarray(mx.X[:, cols])
    ref = R.ewma_ref(X, alpha, 60, 1e-12)
    a = R.abi_f32(alpha)
    checked = 0
    for j, f in enumerate(R.FAMILIES):
        stop = mx.event[cols[j]] if f == "inf" else 600  # state is non-finite from the inf on
        run = _mp_run(X[:stop, j], a)
        with mpmath.workdps(60):
            for t, (m, v) in enumerate(run):
                if m is None:
                    assert math.isnan(ref.m_hi[t, j]) and math.isnan(ref.v_hi[t, j])
                    continue
                gm = mpmath.mpf(float(ref.m_hi[t, j])) + mpmath.mpf(float(ref.m_lo[t, j]))
                gv = mpmath.mpf(float(ref.v_hi[t, j])) + mpmath.mpf(float(ref.v_lo[t, j]))
                assert abs(gm - m) <= mpmath.mpf("1e-25") * abs(m) + mpmath.mpf("1e-290"), (f, t)
                assert abs(gv - v) <= mpmath.mpf("1e-25") * abs(v) + mpmath.mpf("1e-290"), (f, t)
                checked += 1
    all_nan = 600
    inf_tail = 600 - mx.event[cols[R.FAMILIES.index("inf")]]
    late = sum(int(np.isnan(X[:, j]).argmin()) for j, f in enumerate(R.FAMILIES)
               if f not in ("all_nan",))
    assert checked == 600 * len(R.FAMILIES) - all_nan - inf_tail - late


def test_reference_z_equals_mpmath_z():
    """The per-step z and the window maxima the bound is measured from."""
    mx = R.build_matrix((60, 300), 600, rot=3)
    cols = [int(mx.cols(f)[0]) for f in ("benign", "mean1e7", "const_step", "alt2^62")]
    X = np.ascontiguousarray(mx.X[:, cols])
    for eps in (1e-12, 1e-2):
        ref = R.ewma_ref(X, 2 / 61, 60, eps)
        a, e = R.abi_f32(2 / 61), R.abi_f32(eps)
        for j in range(len(cols)):
            run = _mp_run(X[:, j], a)
            with mpmath.workdps(60):
                for t in range(1, 600):
                    m, v = run[t - 1]
                    z = (mpmath.mpf(float(X[t, j])) - m) / mpmath.sqrt(v + mpmath.mpf(e))
                    assert abs(mpmath.mpf(float(ref.z[t, j])) - z) <= 8 * R.U64 * abs(z), (j, t)
        np.testing.assert_array_equal(ref.Z, np.abs(ref.z).reshape(10, 60, -1).max(axis=1))


# -------------------------------------- the existing oracles tied to the model
def test_c_oracle_and_pandas_golden_within_the_f64_term(golden):
    """native.ewma_z (f64 state, f64 z, cast to f32) and the pandas state
    through spec.window_scores_from_state lie within the bound's f64 term of
    the reference, plus one u32 for the oracle's final cast (C1 = 1) and none
    for the f64 scores (C1 = 0; the f64 division and sqrt are part of C2's
    slack: 3 u64 |z| < u64/alpha xmax/sqrt(v) whenever |d| <= 2 xmax)."""
    g = np.load(golden / "ewma_pandas.npz")
    X, M, V, a = g["X"], g["mean"], g["var"], float(g["alpha"])
    W, eps = 60, 1e-12
    # the oracles take alpha and eps as f64 (the kernels' C ABI rounds them to f32)
    refd = R.ewma_ref(X, a, W, eps, f32_args=False)
    assert np.isfinite(refd.z).all()
    r, skip = R.compare(native.ewma_z(X, a, W, eps), refd.Z, R.window_bound(refd, c1=1.0))
    assert not skip.any() and r.max() <= 1.0, r.max()
    r, skip = R.compare(spec.window_scores_from_state(X, M, V, W, eps), refd.Z,
                        R.window_bound(refd, c1=0.0))
    assert not skip.any() and r.max() <= 1.0, r.max()


def test_c_oracle_within_the_f64_term_on_the_adversarial_matrix():
    case = R.MODE_CASES[0]
    mx, ref, _ = R.case_ref(case)
    a = R.abi_f32(case.alpha)
    r, skip = R.compare(native.ewma_z(mx.X, a, case.W, R.abi_f32(case.eps)), ref.Z,
                        R.window_bound(ref, c1=1.0))
    assert (skip.sum(axis=0) == R.expected_skips(mx, case.W)).all()
    assert r.max() <= 1.0, _family_worst(mx, r)


# ------------------------------------- emulations of the kernels within bound
@pytest.mark.parametrize("case", R.BOUND_CASES + R.DENORMAL_CASES,
                         ids=_ids(R.BOUND_CASES + R.DENORMAL_CASES))
def test_emulated_kernels_within_bound(case):
    """Plain-f64 restatements of (a) the sequential step and (b) phase A, the
    transfer fold and phase C with the kernel's U, per step and per window,
    on every family / alpha / eps the GPU tests use; the only cells left out
    are the inf family's from its inf on."""
    mx, ref, wb = R.case_ref(case)
    sb = R.step_bound(ref)
    # the time-parallel form is not taken above W = 128
    emus = (R.emulate_sequential, R.emulate_time_parallel) if case.W <= 128 else \
        (R.emulate_sequential,)
    for emu in emus:
        z, Z = emu(mx.X, case.alpha, case.W, case.eps)
        r, skip = R.compare(z, ref.z, sb)
        assert (skip.sum(axis=0) == R.expected_skips(mx)).all()
        assert r.max() <= 1.0, (emu.__name__, _family_worst(mx, r))
        r, skip = R.compare(Z, ref.Z, wb)
        assert (skip.sum(axis=0) == R.expected_skips(mx, case.W)).all()
        assert r.max() <= 1.0, (emu.__name__, _family_worst(mx, r))


def test_time_parallel_emulation_takes_another_route_than_the_sequential_one():
    """The fold is not the sequential recurrence restated: its f64 state
    differs in the last bits (so the agreement above is not an identity), and
    the bound notices an algebra slip (Q1 with the wrong sign of its term)."""
    case = R.MODE_CASES[2]
    mx, ref, _ = R.case_ref(case)
    zs, _ = R.emulate_sequential(mx.X, case.alpha, case.W, case.eps)
    zt, _ = R.emulate_time_parallel(mx.X, case.alpha, case.W, case.eps)
    fin = np.isfinite(ref.z)
    assert (zs[fin] != zt[fin]).any()
    zb, _ = R.emulate_time_parallel(mx.X, case.alpha, case.W, case.eps, q1_sign=+2.0)
    r, _ = R.compare(zb, ref.z, R.step_bound(ref))
    assert r.max() > 10.0


def test_bound_has_teeth():
    """An f32 state, or a z off by 8 u32, is outside the bound."""
    case = R.MODE_CASES[0]
    mx, ref, _ = R.case_ref(case)
    sb = R.step_bound(ref)
    z, _ = R.emulate_sequential(mx.X, case.alpha, case.W, case.eps)
    r, _ = R.compare(z.astype(np.float64) * (1 + 8 * R.U32), ref.z, sb)
    assert r.max() > 1.0
    z32, _ = R.emulate_sequential(mx.X, case.alpha, case.W, case.eps, state=np.float32)
    r, _ = R.compare(z32, ref.z, sb)
    assert r[:, mx.cols("mean1e7")].max() > 100.0


# ----------------------------------------------------- the builder's premises
def _check_events(mx):
    """The events are where the plan says."""
    for i, (f, p) in enumerate(zip(mx.family, mx.event)):
        x = mx.X[:, i]
        if f == "outlier":
            assert np.abs(x).argmax() == p
        elif f == "shift":
            assert np.median(x[p:]) - np.median(x[:p]) > 1e4 * np.std(x[:p]) and p >= 15
        elif f == "const_step":
            assert (x[:p] == x[0]).all() and (x[p:] == x[p]).all() and x[p] != x[0]
        elif f == "first_late":
            assert np.isnan(x[:p]).all() and not np.isnan(x[p:]).any()
        elif f == "nan_run_start":
            assert not np.isnan(x[:p]).any() and np.isnan(x[p:p + R.NAN_RUN]).all()
            assert not np.isnan(x[p + R.NAN_RUN:]).any() and R.NAN_RUN > 128
        elif f == "nan_run_end":
            lo = max(p - R.NAN_RUN, 1)
            assert np.isnan(x[lo:p]).all() and not np.isnan(x[p:]).any()
            assert not np.isnan(x[:lo]).any()
        elif f == "inf":
            assert np.isinf(x[p]) and np.isfinite(np.delete(x, p)).all()
        elif f == "all_nan":
            assert np.isnan(x).all()
        elif f == "alt2^62":
            assert (np.abs(x) == 2.0 ** 62).all() and (x[1:] == -x[:-1]).all()
        elif f == "mean1e7":
            assert (x == np.rint(x)).all() and abs(x.mean() - 1e7) < 10
        if f in ("benign", "mean1e7", "scale1e-20", "scale1e15", "alt2^62", "outlier", "shift",
                 "const_step"):
            assert np.isfinite(x).all()


MIXED_CASES = tuple(c for c in R.BOUND_CASES if c.layout == "mixed")
DENSE_CASES = tuple(c for c in R.BOUND_CASES if c.layout == "dense")


@pytest.mark.parametrize("case", MIXED_CASES, ids=_ids(MIXED_CASES))
def test_mixed_layout_places_every_event_at_every_border(case):
    mx = case.matrix()
    assert mx.X.shape == (case.T, R.S_COLS) and mx.X.dtype == np.float32
    assert len(case.borders) >= 2 and all(0 < b < case.T for b in case.borders)
    places = {b + k for b in case.borders for k in (-1, 0, 1)}
    for f in R.EVENT_FAMILIES:
        assert places <= {mx.event[i] for i in mx.cols(f)}, f
    for f in R.FAMILIES:
        strips = [int(i) // 64 for i in mx.cols(f) if i < 128]
        assert {0, 1} <= set(strips), f                       # across the full waves
        if f in R.EVENT_FAMILIES:
            assert max(strips.count(w) for w in (0, 1)) >= 3, f   # and inside one
    _check_events(mx)


@pytest.mark.parametrize("case", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_dense_layout_is_scored_by_the_dense_step(case):
    """The tiled kernel's dense predicate, evaluated on the matrix with the
    case's launch segments.  Strip 0 (NaN-free families, every event at every
    border): every whole block but the series' first is dense, so each event
    is scored by the dense step with dense blocks on both sides.  Strip 1
    (NaN runs only): general around every border, dense before and after."""
    assert case.mode == 1 and R.DENSE_CASES and R.W150_CASES[1] in DENSE_CASES
    mx = case.matrix()
    _check_events(mx)
    places = {b + k for b in case.borders for k in (-1, 0, 1)}
    for strip, fams in ((0, R.DENSE_EVENTS), (1, R.SWITCH_EVENTS)):
        for f in fams:
            cols = mx.cols(f)
            assert (cols // 64 == strip).all() and places == {mx.event[i] for i in cols}, f
    assert set(R.DENSE_EVENTS) | set(R.NAN_FREE_PLAIN[:4]) <= set(mx.family[:64]) \
        <= set(R.DENSE_EVENTS) | set(R.NAN_FREE_PLAIN)
    assert set(mx.family[64:128]) == set(R.SWITCH_EVENTS) | {"benign"}
    assert set(mx.family[128:]) <= set(R.NAN_FREE_PLAIN)
    d = R.dense_blocks(mx.X, R.launches(case.T, case.seg))
    whole = case.T // 64
    assert (d[:, :whole] >= 0).all()                 # segments are whole blocks
    assert d[0, 0] == 0 and (d[0, 1:whole] == 1).all() and (d[2, 1:whole] == 1).all()
    for p in places:                                 # strip 0: dense at, before and after
        blocks = [k for k in (p // 64 - 1, p // 64, p // 64 + 1) if 1 <= k < whole]
        assert blocks and (p // 64 in blocks or p >= whole * 64), p
    # strip 1: the blocks a NaN run touches are general, and between two
    # borders that lie more than two runs apart the wave is dense again
    general = set()
    for p in places:
        general |= set(range(max(p - R.NAN_RUN, 1) // 64, (p + R.NAN_RUN - 1) // 64 + 1))
    for k in range(1, whole):
        assert d[1, k] == (0 if k in general else 1), k
    flips = int((np.diff(d[1, 1:whole]) != 0).sum())
    far = [b for a, b in zip(case.borders, case.borders[1:]) if b - a > 2 * R.NAN_RUN + 128]
    assert flips >= 2 * len(far) >= 2


def test_streamed_dense_layout_starts_dense_at_the_cut():
    """The two-upload run of the GPU test: the second upload's first block
    (the events at the cut) is dense in strip 0, the state carried."""
    mx = R.build_matrix((240, 720, 960), 1920, 1, "dense")
    d = R.dense_blocks(mx.X, [(0, 960), (960, 960)])
    assert d[0, 0] == 0 and (d[0, 1:] == 1).all() and d[0, 960 // 64] == 1
    assert 0 in d[1, 1:] and 1 in d[1, 1:]
    one = R.dense_blocks(mx.X, [(0, 1920)])
    np.testing.assert_array_equal(d, one)


def test_cases_put_every_family_in_the_partial_wave():
    for group in (R.MODE_CASES, R.BLOCK_CASES):
        seen = set()
        for c in group:
            seen |= set(c.matrix().family[128:])
        assert seen == set(R.FAMILIES)


def test_geometry_matches_the_issue_table():
    assert [R.tp_sub_chunk(W) for W in (1, 6, 33, 60, 64, 65, 96, 128)] == \
        [64, 60, 33, 60, 64, 65, 96, 128]
    assert R.borders(1, 60, 2400) == (16, 64, 960, 1920, 2368)
    assert R.borders(2, 60, 1920) == (60, 720, 1440)
    assert R.borders(2, 65, 1950) == (65, 780, 1560)
    assert R.borders(2, 128, 3840) == (128, 1536, 3072)
    assert R.borders(3, 60, 1920) == (32, 64)
    assert R.borders(1, 60, 2400, layout="dense") == (80, 128, 960, 1920, 2368)
    assert R.borders(1, 150, 2400, seg=4800) == (16, 64, 2368)  # lcm(150, 64) > T: one launch
    assert 80 % 64 == 16 and 128 % 64 == 0 and 960 % 64 == 0 and math.lcm(150, 64) == 4800


@pytest.mark.parametrize("case", R.BOUND_CASES, ids=_ids(R.BOUND_CASES))
def test_reference_is_finite_except_from_the_inf_on(case):
    """No comparison silently leaves cells out: the reference and its bound
    are finite everywhere but in the inf family, and there non-finite exactly
    from the inf on (per step and per window)."""
    mx, ref, wb = R.case_ref(case)
    bad = ~np.isfinite(ref.z) | ~np.isfinite(R.step_bound(ref))
    badw = ~np.isfinite(ref.Z) | ~np.isfinite(wb)
    for i, (f, p) in enumerate(zip(mx.family, mx.event)):
        if f == "inf":
            assert (np.flatnonzero(bad[:, i]) == np.arange(p, case.T)).all()
            assert (np.flatnonzero(badw[:, i]) == np.arange(p // case.W, case.T // case.W)).all()
        else:
            assert not bad[:, i].any() and not badw[:, i].any(), f
    assert (ref.Z[:, mx.cols("all_nan")] == 0).all()

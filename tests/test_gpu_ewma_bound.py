"""GPU: the three EWMA/z kernels against the double-double reference within
the derived bound (tests/ewma_ref.py), on the adversarial matrix whose events
sit on each kernel's own borders; bit-equality between the kernels, chunkings
and uploads on the same matrix; argument handling at the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest

import anomod
import ewma_ref as R
from anomod import _lib as L

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.name for c in cases]


def _set_mode(monkeypatch, mode, seg=None):
    monkeypatch.setenv("ANOMOD_EWMA_MODE", str(mode))
    if seg is not None:
        monkeypatch.setenv("ANOMOD_EWMA_SEG", str(seg))


def _assert_within_bound(Z, case):
    """Every window within its bound; nothing left out but the inf family's
    windows from its inf on.  Prints the worst error/bound per family."""
    mx, ref, wb = R.case_ref(case)
    assert Z.shape == ref.Z.shape
    r, skip = R.compare(Z, ref.Z, wb)
    assert (skip.sum(axis=0) == R.expected_skips(mx, case.W)).all()
    fam = np.array(mx.family)
    worst = {f: float(r[:, fam == f].max()) for f in sorted(set(mx.family))}
    print(case.name, " ".join(f"{f}={v:.3f}" for f, v in worst.items()))
    assert r.max() <= 1.0, worst
    # the windows the comparison leaves out: the kernel's score there is the
    # inf itself or a max that dropped the NaNs after it, never a NaN
    assert not np.isnan(Z).any()


def _run(ctx, case):
    mx = case.matrix()
    return ctx.ewma_z(mx.X, case.alpha, case.W, case.eps)


@pytest.mark.parametrize("case", R.MODE_CASES, ids=_ids(R.MODE_CASES))
def test_every_mode_within_bound(ctx, monkeypatch, case):
    """W = 60, alpha = 2/61, both eps.  Tiles: 960-step launch segments, T =
    2400 (2.5 segments, a partial last load block); time-parallel and auto:
    T = 1920 = two super-chunks of 720 and one with four idle waves; rows:
    32-step load blocks."""
    _set_mode(monkeypatch, case.mode, case.seg if case.mode == 1 else None)
    _assert_within_bound(_run(ctx, case), case)


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=_ids(R.BLOCK_CASES))
def test_time_parallel_register_block_borders(ctx, monkeypatch, case):
    """U = 64, 60, 33, 64, 65 (the 128-step register block), 96, 128; W = 6,
    alpha = 2/7, eps = 1e-2 is the product's trace-window setting."""
    _set_mode(monkeypatch, 2)
    assert R.tp_sub_chunk(case.W) == {1: 64, 6: 60, 33: 33, 64: 64, 65: 65, 96: 96,
                                      128: 128}[case.W]
    _assert_within_bound(_run(ctx, case), case)


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=_ids(R.DENSE_CASES))
def test_tiles_dense_path_within_bound(ctx, monkeypatch, case):
    """The dense layout: strip 0 holds NaN-free families only, so the dense
    step (window end checked once per float4, W % 4 == 0) scores every event
    at the tile, load-block, segment and last-block borders; strip 1 leaves
    the dense path around each border (NaN runs) and returns to it
    (test_dense_layout_is_scored_by_the_dense_step holds the premise)."""
    _set_mode(monkeypatch, 1, case.seg)
    _assert_within_bound(_run(ctx, case), case)


@pytest.mark.parametrize("case", R.W150_CASES, ids=_ids(R.W150_CASES))
def test_time_parallel_not_taken_above_128(ctx, monkeypatch, case):
    """W = 150 under mode 2 runs the tiled kernel: mode 1's bits, within
    bound.  One launch (lcm(150, 64) > T); W % 4 != 0, so the dense layout
    runs the dense step that checks the window end at every step."""
    out = []
    for mode in (2, 1):
        _set_mode(monkeypatch, mode, case.seg)
        out.append(_run(ctx, case))
    np.testing.assert_array_equal(out[0], out[1])
    _assert_within_bound(out[0], case)


@pytest.mark.parametrize("case", R.ALPHA_CASES, ids=_ids(R.ALPHA_CASES))
def test_alpha_sweep_within_bound(ctx, monkeypatch, case):
    """alpha = 1e-4 (the f64 term of the bound dominates), 0.9, and 1 (beta =
    0: A = 0 after one sample, v = 0 throughout)."""
    _set_mode(monkeypatch, case.mode, case.seg if case.mode == 1 else None)
    _assert_within_bound(_run(ctx, case), case)


@pytest.mark.parametrize("case", R.TILED_CASES + (R.MODE_CASES[4],),
                         ids=_ids(R.TILED_CASES + (R.MODE_CASES[4],)))
def test_tiles_and_rows_bit_equal_on_the_adversarial_matrix(ctx, monkeypatch, case):
    """The dense path of the tiled kernel claims the general step's roundings:
    modes 1 and 3 give the same bits.  The dense-layout matrices are the ones
    whose events the dense step scores (both window-end forms: W = 60 and
    W = 150); on the mixed layout only the partial wave is ever dense, the
    full strips run the general step in both kernels.  The last case is the
    rows kernel's own matrix (events at its 32-step load blocks)."""
    assert case.mode == 3 or case.W in (60, 150)
    mx = case.matrix()
    out = []
    for mode in (1, 3):
        _set_mode(monkeypatch, mode, case.seg)
        out.append(ctx.ewma_z(mx.X, case.alpha, case.W, case.eps))
    np.testing.assert_array_equal(out[0], out[1])


# cuts of the chunked one-shot call (lcm(U, 16) = 240 and three of them) and of
# the two uploads (960), with every event family on each of them
CUT_BORDERS, CUT_T = (240, 720, 960), 1920


@pytest.mark.parametrize("layout", ["mixed", "dense"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_chunked_and_streamed_bit_equal_on_the_adversarial_matrix(ctx, monkeypatch, mode, layout):
    """Under mode 1 the dense layout puts the events at the cuts into blocks
    the dense step scores (the second upload starts dense: host test)."""
    _set_mode(monkeypatch, mode)
    mx = R.build_matrix(CUT_BORDERS, CUT_T, mode, layout)
    W, a = 60, 2 / 61
    assert math.lcm(R.tp_sub_chunk(W), 16) == 240
    for eps in (1e-12, 1e-2):
        one = ctx.ewma_z(mx.X, a, W, eps)
        for chunk in (240, 720):
            monkeypatch.setenv("ANOMOD_EWMA_CHUNK_STEPS", str(chunk))
            np.testing.assert_array_equal(ctx.ewma_z(mx.X, a, W, eps), one)
        monkeypatch.delenv("ANOMOD_EWMA_CHUNK_STEPS")
        ser = anomod.DeviceSeries(ctx, CUT_T // 2, R.S_COLS)
        ser.upload(mx.X[: CUT_T // 2])
        z1 = ser.ewma_z(a, W, eps)
        ser.upload(mx.X[CUT_T // 2:])
        z2 = ser.ewma_z(a, W, eps)
        ser.free()
        np.testing.assert_array_equal(np.concatenate([z1, z2]), one)


# ------------------------------------------- the eps precondition of zscale
@pytest.mark.parametrize("case", R.DENORMAL_CASES, ids=_ids(R.DENORMAL_CASES))
def test_tiny_series_within_bound_at_the_smallest_eps(ctx, monkeypatch, case):
    """Series of magnitude 1e-21: v ~ 1e-42 is an f32 denormal, and with eps =
    2^-126 the argument of the reciprocal square root is the smallest normal."""
    _set_mode(monkeypatch, case.mode)
    assert case.eps == float(np.finfo(np.float32).tiny)
    mx, ref, _ = R.case_ref(case)
    v = ref.v_prev[ref.upd]
    assert 0 < np.median(v) < 2.0 ** -126 and (ref.Z[1:] > 1e-3).all()
    _assert_within_bound(_run(ctx, case), case)


@pytest.mark.parametrize("eps", [0.0, 1e-40, float(np.nextafter(np.float32(2.0 ** -126),
                                                                 np.float32(0)))],
                         ids=["0", "1e-40", "below_2^-126"])
def test_eps_below_the_smallest_normal_is_refused(ctx, ewma_any_mode, eps):
    """The hardware reciprocal square root reads a denormal v + eps as 0: on
    these series eps = 0 and eps = 1e-40 scored inf in every window of every
    kernel where the reference is O(1) (measured before the entry point
    enforced the precondition).  Such an eps is now EINVAL, naming the bound,
    at both entry points; a valid call afterwards is unaffected."""
    case = R.DENORMAL_CASES[0]
    mx = case.matrix()
    good = ctx.ewma_z(mx.X, case.alpha, case.W, case.eps)
    with pytest.raises(L.AnomodError, match=r"eps=\S+ must be >= 2\^-126 \(1\.17549e-38\)") as ei:
        ctx.ewma_z(mx.X, case.alpha, case.W, eps)
    assert ei.value.status == L.EINVAL
    ser = anomod.DeviceSeries(ctx, case.T, R.S_COLS)
    ser.upload(mx.X)
    with pytest.raises(L.AnomodError, match=r"must be >= 2\^-126"):
        ser.ewma_z(case.alpha, case.W, eps)
    np.testing.assert_array_equal(ser.ewma_z(case.alpha, case.W, case.eps), good)
    ser.free()
    np.testing.assert_array_equal(ctx.ewma_z(mx.X, case.alpha, case.W, case.eps), good)


# ------------------------------------------------------------------ arguments
def _call(ctx, X, alpha, W, eps):
    T, S = X.shape
    Z = np.full((max(T // max(W, 1), 1), S), -1.0, np.float32)
    ctx._check(ctx._lib.anomod_ewma_z(ctx.handle, L.ptr(X, C.c_float), T, S, alpha, W, eps,
                                      L.ptr(Z, C.c_float)))
    return Z


def test_arguments_are_checked_at_the_c_abi(ctx, ewma_any_mode):
    rng = np.random.default_rng(3)
    X = np.ascontiguousarray((50 + rng.standard_normal((120, R.S_COLS))).astype(np.float32))
    good = _call(ctx, X, 0.25, 60, 1e-12)
    assert (good >= 0).all()
    refused = [(0.25, 0, 1e-12, r"T=120 must be a multiple of W=0"),
               (0.25, 7, 1e-12, r"T=120 must be a multiple of W=7"),
               (0.0, 60, 1e-12, r"alpha=0 outside \(0, 1\]"),
               (-0.1, 60, 1e-12, r"alpha=-0\.1 outside \(0, 1\]"),
               (1.0000001, 60, 1e-12, r"alpha=1 outside \(0, 1\]"),
               (math.nan, 60, 1e-12, r"alpha=-?nan outside \(0, 1\]"),
               (0.25, 60, -1e-12, r"eps=-1e-12 must be >= 2\^-126"),
               (0.25, 60, math.nan, r"eps=-?nan must be >= 2\^-126")]
    for alpha, W, eps, msg in refused:
        with pytest.raises(L.AnomodError, match=msg) as ei:
            _call(ctx, X, alpha, W, eps)
        assert ei.value.status == L.EINVAL
        np.testing.assert_array_equal(_call(ctx, X, 0.25, 60, 1e-12), good)
    # alpha = 1 is legal and scored: m = the previous sample, v = 0
    one = _call(ctx, X, 1.0, 60, 1e-12)
    ref = R.ewma_ref(X, 1.0, 60, 1e-12)
    r, skip = R.compare(one, ref.Z, R.window_bound(ref))
    assert not skip.any() and r.max() <= 1.0


@pytest.fixture(params=[1, 2, 3], ids=["tiles", "time_parallel", "rows"])
def ewma_any_mode(request, monkeypatch):
    monkeypatch.setenv("ANOMOD_EWMA_MODE", str(request.param))
    return request.param

"""GPU: the series-correlation kernel against the host model
(series_corr_ref.py) inside the bound of its accuracy contract, at the borders
of the 16-step tile, the 32-step load block and the 64-lane wave; adversarial
columns; the two layouts, repeat runs and the EWMA state; argument checks at
the C ABI."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from series_corr_ref import (BOUND_MAX, K_CASES, S_CASES, T_CASES, adversarial_case,
                             correlate_ref, min_pairs_of, random_case)

pytestmark = pytest.mark.gpu

LAYOUTS = {"tiles": "1", "rows": "3"}   # ANOMOD_EWMA_MODE that creates a series in each


def resident(ctx, monkeypatch, layout, X):
    monkeypatch.setenv("ANOMOD_EWMA_MODE", LAYOUTS[layout])
    ser = anomod.DeviceSeries(ctx, X.shape[0], X.shape[1])
    ser.upload(X)
    return ser


def assert_within_bound(r, n, m, what):
    np.testing.assert_array_equal(n, m["n"], err_msg=f"n {what}")
    np.testing.assert_array_equal(np.isnan(r), np.isnan(m["r"]), err_msg=f"NaN pattern {what}")
    have = ~np.isnan(m["r"])
    if have.any():
        assert m["bound"][have].max() <= BOUND_MAX, what
        err = np.abs(r[have] - m["r"][have])
        over = err > m["bound"][have]
        assert not over.any(), (f"{what}: {int(over.sum())} of {int(have.sum())} outside the "
                                f"bound, worst error {err.max():.3e} against "
                                f"{m['bound'][have][np.argmax(err)]:.3e}")
        assert (np.abs(r[have]) <= 1).all(), what


@pytest.fixture(scope="module")
def models():
    """The model of every (T, S, K) case, computed once."""
    out = {}
    for T in T_CASES:
        for S in S_CASES:
            for K in K_CASES:
                X, Y = random_case(T, S, K)
                out[T, S, K] = (X, Y, correlate_ref(X, Y, min_pairs_of(T)))
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("K", K_CASES)
def test_within_the_bound_at_the_kernel_borders(ctx, monkeypatch, models, layout, K):
    for T in T_CASES:
        for S in S_CASES:
            X, Y, m = models[T, S, K]
            ser = resident(ctx, monkeypatch, layout, X)
            r, n = ser.correlate(Y, min_pairs_of(T))
            ser.free()
            assert r.shape == (K, S) and n.shape == (K, S)
            assert_within_bound(r, n, m, f"T={T} S={S} K={K} {layout}")


@pytest.mark.parametrize("K", [3, 5, 7])
def test_target_counts_between_the_kernel_widths(ctx, K):
    """K that is no power of two runs the next wider kernel with padded targets."""
    X, Y = random_case(65, 65, K)
    r, n = ctx.correlate(X, Y, 3)
    assert_within_bound(r, n, correlate_ref(X, Y, 3), f"K={K}")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_adversarial_columns(ctx, monkeypatch, layout):
    mp = 4
    X, Y, cols = adversarial_case(mp)
    m = correlate_ref(X, Y, mp)
    ser = resident(ctx, monkeypatch, layout, X)
    r, n = ser.correlate(Y, mp)
    ser.free()
    assert_within_bound(r, n, m, layout)
    c = cols
    assert (n[:, c["all_nan"]] == 0).all() and np.isnan(r[:, c["all_nan"]]).all()
    assert n[0, c["only_where_y0_missing"]] == 0 and np.isnan(r[0, c["only_where_y0_missing"]])
    assert n[1, c["only_where_y0_missing"]] == 6 and not np.isnan(r[1, c["only_where_y0_missing"]])
    assert n[0, c["constant"]] == 91 and np.isnan(r[:, c["constant"]]).all()
    assert n[0, c["below_min_pairs"]] == mp - 1 and np.isnan(r[0, c["below_min_pairs"]])
    assert n[0, c["at_min_pairs"]] == mp and not np.isnan(r[0, c["at_min_pairs"]])
    assert n[0, c["infs"]] < 91 and n[0, c["infs"]] == m["n"][0, c["infs"]]
    # 1e9 + noise in steps of the f32 spacing there (64): k = 1 + n (px - mean)^2 / sxx
    # stays below 16 under the pivot, where mean^2 / variance is ~1e13
    assert m["kx"][0, c["large_level"]] < 16 and not np.isnan(r[0, c["large_level"]])
    assert abs(r[0, c["equals_y0"]] - 1.0) <= m["bound"][0, c["equals_y0"]]
    assert abs(r[0, c["equals_minus_y0"]] + 1.0) <= m["bound"][0, c["equals_minus_y0"]]
    assert n[0, c["late_start"]] == m["n"][0, c["late_start"]] > 40


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def test_layouts_and_runs_give_the_same_bits(ctx, monkeypatch):
    X, Y = random_case(97, 130, 8)
    Xa, Ya, _ = adversarial_case()
    for Xc, Yc in ((X, Y), (Xa, Ya)):
        got = {}
        for layout in LAYOUTS:
            ser = resident(ctx, monkeypatch, layout, Xc)
            got[layout] = [ser.correlate(Yc, 3) for _ in range(2)]
            ser.free()
        monkeypatch.delenv("ANOMOD_EWMA_MODE")
        got["host"] = [ctx.correlate(Xc, Yc, 3)]
        r0, n0 = got["tiles"][0]
        for name, runs in got.items():
            for r, n in runs:
                np.testing.assert_array_equal(bits(r), bits(r0), err_msg=name)
                np.testing.assert_array_equal(n, n0, err_msg=name)


def test_dense_blocks_give_the_bits_of_the_general_step(ctx, monkeypatch):
    """A wave whose samples and targets are all present takes the step without
    selects; one missing sample per block in lane 63 keeps the wave on the
    general step.  The other 63 columns must not change by a bit."""
    rng = np.random.default_rng(8)
    T, S, K = 160, 64, 8
    X = (300 + 5 * rng.standard_normal((T, S))).astype(np.float32)
    Y = (10 + rng.standard_normal((T, K))).astype(np.float32)
    Xg = X.copy()
    Xg[5::32, 63] = np.nan
    for layout in LAYOUTS:
        out = []
        for Xc in (X, Xg):
            ser = resident(ctx, monkeypatch, layout, Xc)
            out.append(ser.correlate(Y, 3))
            ser.free()
        np.testing.assert_array_equal(bits(out[0][0][:, :63]), bits(out[1][0][:, :63]))
        assert (out[0][1] == T).all() and (out[1][1][:, 63] == T - 5).all()
        assert_within_bound(out[0][0], out[0][1], correlate_ref(X, Y, 3), f"dense {layout}")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ewma_after_correlate_is_unchanged(ctx, monkeypatch, layout):
    X, Y = random_case(96, 130, 2)
    X = np.where(np.isinf(X), np.nan, X)      # EWMA's domain: NaN is the missing sample
    plain = resident(ctx, monkeypatch, layout, X)
    z_plain = [plain.ewma_z(0.1, 16), plain.ewma_z(0.1, 16)]   # the second call carries state
    plain.free()
    ser = resident(ctx, monkeypatch, layout, X)
    r1 = ser.correlate(Y, 3)
    z1 = ser.ewma_z(0.1, 16)
    r2 = ser.correlate(Y, 3)
    z2 = ser.ewma_z(0.1, 16)
    np.testing.assert_array_equal(ser.download().view(np.uint32), X.view(np.uint32))
    ser.free()
    np.testing.assert_array_equal(z1.view(np.uint32), z_plain[0].view(np.uint32))
    np.testing.assert_array_equal(z2.view(np.uint32), z_plain[1].view(np.uint32))
    np.testing.assert_array_equal(bits(r1[0]), bits(r2[0]))


def test_argument_checks_at_the_c_abi(ctx):
    lib = L.lib()
    T, S = 8, 4
    X = np.arange(T * S, dtype=np.float32).reshape(T, S)
    Y = np.ones((T, 9), np.float32)
    r = np.full((9, S), 123.0)
    n = np.full((9, S), 77, np.uint32)
    pX, pY = L.ptr(X, C.c_float), L.ptr(Y, C.c_float)
    pr, pn = L.ptr(r, C.c_double), L.ptr(n, C.c_uint32)
    nullf, nulld = C.cast(None, C.POINTER(C.c_float)), C.cast(None, C.POINTER(C.c_double))
    ser = anomod.DeviceSeries(ctx, T, S)
    ser.upload(X)
    h = ctx.handle
    for K in (0, 9):
        assert lib.anomod_correlate(h, pX, T, S, pY, K, 3, pr, pn) == L.EINVAL
        assert b"K=" in lib.anomod_last_error(h)
        assert lib.anomod_series_correlate(h, ser.handle, pY, K, 3, pr, pn) == L.EINVAL
    assert lib.anomod_series_correlate(h, None, pY, 1, 3, pr, pn) == L.EINVAL
    assert b"NULL" in lib.anomod_last_error(h)
    assert lib.anomod_series_correlate(h, ser.handle, nullf, 1, 3, pr, pn) == L.EINVAL
    assert lib.anomod_series_correlate(h, ser.handle, pY, 1, 3, nulld, pn) == L.EINVAL
    assert lib.anomod_correlate(h, nullf, T, S, pY, 1, 3, pr, pn) == L.EINVAL
    assert lib.anomod_correlate(h, pX, T, S, nullf, 1, 3, pr, pn) == L.EINVAL
    assert lib.anomod_correlate(h, pX, T, S, pY, 1, 3, nulld, pn) == L.EINVAL
    assert lib.anomod_correlate(h, pX, 1 << 32, S, pY, 1, 3, pr, pn) == L.EINVAL
    # empty input: OK, nothing written
    assert lib.anomod_correlate(h, pX, 0, S, pY, 1, 3, pr, pn) == L.OK
    assert lib.anomod_correlate(h, pX, T, 0, pY, 1, 3, pr, pn) == L.OK
    assert (r == 123.0).all() and (n == 77).all()
    # n may be NULL
    y1 = np.ascontiguousarray(X[:, 0] * 2)
    assert lib.anomod_series_correlate(h, ser.handle, L.ptr(y1, C.c_float), 1, 3, pr,
                                       C.cast(None, C.POINTER(C.c_uint32))) == L.OK
    assert r[0, 0] == 1.0 and (n == 77).all()
    ser.free()
    with pytest.raises(ValueError):
        ctx.correlate(X, np.ones(T + 1, np.float32))

"""Host model of the series correlation (include/anomod.h
anomod_series_correlate): a two-pass, mean-centred Pearson in np.longdouble
over the literal pair-set rule, with the condition numbers and the bound of the
kernel's accuracy contract; and the inputs the CPU and GPU tests share."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def correlate_ref(X, Y, min_pairs=3):
    """r f64 [K, S], n u32 [K, S], kx, ky f64 [K, S] and bound f64 [K, S] =
    8 T 2^-53 max(kx, ky) + 2^-50.

    Step t is a pair of (k, s) iff X[t][s] and Y[t][k] are both finite.  r is
    NaN when n < max(min_pairs, 2) or a side has no spread over the pair set.
    kx = sum (x - px)^2 / sum (x - mean)^2 over the pair set, px the first
    finite X[t][s] whatever Y holds (ky likewise with the first finite
    Y[t][k]); inf where the denominator is 0, NaN without a pivot."""
    X = np.asarray(X, np.float32)
    Y = np.asarray(Y, np.float32)
    if Y.ndim == 1:
        Y = Y[:, None]
    T, S = X.shape
    K = Y.shape[1]
    xf, yf = np.isfinite(X), np.isfinite(Y)
    Xl = np.where(xf, X, 0).astype(LD)
    Yl = np.where(yf, Y, 0).astype(LD)

    def pivot(V, fin):
        first = np.argmax(fin, axis=0)
        p = V[first, np.arange(V.shape[1])]
        return np.where(fin.any(axis=0), p, LD(np.nan))

    px, py = pivot(Xl, xf), pivot(Yl, yf)
    r = np.full((K, S), np.nan)
    n = np.zeros((K, S), np.uint32)
    kx = np.full((K, S), np.nan)
    ky = np.full((K, S), np.nan)
    need = max(int(min_pairs), 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            pair = xf & yf[:, k][:, None]                      # [T, S]
            cnt = pair.sum(axis=0)
            n[k] = cnt
            cl = np.maximum(cnt, 1).astype(LD)
            yk = np.broadcast_to(Yl[:, k][:, None], (T, S))
            mx = np.where(pair, Xl, 0).sum(axis=0) / cl
            my = np.where(pair, yk, 0).sum(axis=0) / cl
            dx = np.where(pair, Xl - mx, 0)
            dy = np.where(pair, yk - my, 0)
            sxx, syy, sxy = (dx * dx).sum(axis=0), (dy * dy).sum(axis=0), (dx * dy).sum(axis=0)
            ok = (cnt >= need) & (sxx > 0) & (syy > 0)
            rk = np.clip(sxy / np.sqrt(sxx * syy), -1, 1)
            r[k] = np.where(ok, rk, np.nan).astype(np.float64)
            px2 = (np.where(pair, Xl - px, 0) ** 2).sum(axis=0)
            py2 = (np.where(pair, yk - py[k], 0) ** 2).sum(axis=0)
            some = cnt > 0
            kx[k] = np.where(some, px2 / sxx, np.nan).astype(np.float64)
            ky[k] = np.where(some, py2 / syy, np.nan).astype(np.float64)
    bound = 8.0 * T * U53 * np.fmax(kx, ky) + 2.0 ** -50
    return {"r": r, "n": n, "kx": kx, "ky": ky, "bound": bound}


# ---- shared inputs ---------------------------------------------------------
# The kernel's borders: the 16-step tile, the 32-step load block, the 64-lane wave.
T_CASES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97)
S_CASES = (1, 63, 64, 65, 130)
K_CASES = (1, 2, 8)
BOUND_MAX = 1e-6


def random_case(T, S, K, seed=0):
    """X [T, S], Y [T, K]: level + noise per column (levels up to 1e4, noise
    0.1 .. 10, so the pivot leaves k a few units), ~10 % NaN and a few +-inf in
    X, ~10 % NaN in Y for T >= 4; columns and targets of the first steps stay
    so that small T still has pairs."""
    rng = np.random.default_rng(1000003 * T + 1009 * S + K + seed)
    X = (rng.uniform(0, 1e4, S) + rng.uniform(0.1, 10, S) * rng.standard_normal((T, S)))
    Y = (rng.uniform(-100, 100, K) + rng.uniform(0.1, 10, K) * rng.standard_normal((T, K)))
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    if T >= 4:
        X[rng.random((T, S)) < 0.10] = np.nan
        X[rng.random((T, S)) < 0.01] = np.inf
        X[rng.random((T, S)) < 0.01] = -np.inf
        Y[rng.random((T, K)) < 0.10] = np.nan
    if T >= 64 and S >= 64:
        # the first wave's columns complete and every target present in the
        # second load block: the kernel's dense form runs there
        X[:, :64] = np.where(np.isfinite(X[:, :64]), X[:, :64], 1.0)
        Y[32:64] = np.where(np.isfinite(Y[32:64]), Y[32:64], 0.0)
    return X, Y


def min_pairs_of(T):
    return 2 if T < 8 else 3


def adversarial_case(min_pairs=4):
    """X [97, 70], Y [97, 2] and the named columns of X (see the GPU test)."""
    rng = np.random.default_rng(97)
    T, S = 97, 70
    y0 = (50 + 5 * rng.standard_normal(T)).astype(np.float32)
    y1 = (-3 + rng.standard_normal(T)).astype(np.float32)
    y0[[4, 5, 40, 41, 42, 90]] = np.nan
    y1[10:20] = np.inf                     # a non-finite target sample is missing too
    Y = np.stack([y0, y1], axis=1)
    X = (200 + 3 * rng.standard_normal((T, S))).astype(np.float32)
    cols = {}
    cols["all_nan"] = 0
    X[:, 0] = np.nan
    cols["only_where_y0_missing"] = 1      # n = 0 against y0
    X[:, 1] = np.nan
    X[[4, 5, 40, 41, 42, 90], 1] = [1, 2, 3, 4, 5, 6]
    cols["constant"] = 2                   # sxx = 0 exactly
    X[:, 2] = 7.25
    fin0 = np.nonzero(np.isfinite(y0))[0]
    cols["below_min_pairs"] = 3            # min_pairs - 1 pairs with y0
    X[:, 3] = np.nan
    X[fin0[:min_pairs - 1], 3] = rng.standard_normal(min_pairs - 1)
    cols["at_min_pairs"] = 4               # exactly min_pairs pairs with y0
    X[:, 4] = np.nan
    X[fin0[5:5 + min_pairs], 4] = rng.standard_normal(min_pairs)
    cols["infs"] = 5                       # +-inf samples count as missing
    X[::7, 5] = np.inf
    X[3::11, 5] = -np.inf
    cols["large_level"] = 6                # 1e9 + noise of one f32 spacing (64) per unit
    X[:, 6] = (1e9 + 64.0 * np.rint(3 * rng.standard_normal(T))).astype(np.float32)
    cols["equals_y0"] = 7                  # r = 1
    X[:, 7] = y0
    cols["equals_minus_y0"] = 8            # r = -1
    X[:, 8] = -y0
    cols["late_start"] = 9                 # first finite sample in the second load block
    X[:40, 9] = np.nan
    return X, Y, cols

"""Reference for the three summary entry points (a plain helper, not a
conftest): anomod_value_summary, anomod_response_summary and
anomod_segment_summary, restated in numpy / Python integers, plus the input
builders the host and GPU tests share.

Value summary.  A value is kept when v > 0 (positive_only) or v == v.  The
kept values are ordered by the u64 key of csrc/radix.h,

  u = bits(v);  key = ~u when the sign bit is set, else u | 2^63

(-inf < ... < -0.0 < +0.0 < ... < +inf), and the five picks are read from
the sorted keys at 0, c - 1, c // 2, int(c * 0.95) and int(c * 0.99).  Picks
are bit patterns and compared bit for bit; counts are exact.

The sum is the only float that is not exact.  csrc/radix.hip adds the sorted
values in one fixed order:

  sum_chunks_kernel  one block per SUM_CHUNK = 16384 keys: each of its 256
                     lanes adds its 64 keys in turn (64 additions), then an
                     LDS tree of 8 levels (8 additions on a value's path)
  sum_parts_kernel   one block over the m = ceil(c / SUM_CHUNK) chunk sums:
                     a lane adds ceil(m / SUM_THREADS) of them in turn
                     (SUM_THREADS = 256 lanes), then the same 8-level tree

so a value passes through at most h = 64 + 8 + ceil(m / 256) + 8 additions,
each of relative error <= 2^-53 (round to nearest; sums of subnormals are
exact), and the result differs from the exact sum by at most
h * 2^-53 * sum|x| to first order.  math.fsum rounds the exact sum once,
which adds one more 2^-53 * sum|x|:

  sum_bound(c, sum_abs) = (h + 1) * 2^-53 * sum_abs

The bound is on sum|x|, not on |sum x|, so it also holds under cancellation.

Segment summary: every field is an integer and compared exactly."""
import math

import numpy as np

SUM_CHUNK = 16384      # csrc/radix.hip kSumChunk: keys per block of sum_chunks_kernel
SUM_THREADS = 256      # csrc/radix.hip kSumThreads: lanes of sum_chunks_kernel / sum_parts_kernel
SCAN_BATCH = 1024      # tiles select_scan_kernel scans before it carries a total
TILE = 4096            # values per tile of the selection and the sort
LDS_IDS = 4096         # most ids a counting kernel keeps in LDS (kCatLds, kLdsIds)
COUNT_THREADS = 1024   # threads per workgroup of the two counting kernels
MI355X_CUS = 256

SIGN = np.uint64(1 << 63)
INT32_MIN, INT64_MIN, INT64_MAX = -2**31, -2**63, 2**63 - 1
PICKS = ("min", "max", "median", "p95", "p99")


# ------------------------------------------------------------------ keys
def bits(v) -> np.ndarray:
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def f64_key_ref(v) -> np.ndarray:
    u = bits(v)
    return np.where((u >> np.uint64(63)) != 0, ~u, u | SIGN)


def key_f64_ref(k) -> np.ndarray:
    k = np.ascontiguousarray(k, np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k & ~SIGN, ~k).view(np.float64)


def sorted_selected(values, positive_only) -> np.ndarray:
    """The kept values in key order (f64)."""
    v = np.ascontiguousarray(values, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = v > 0 if positive_only else v == v
    return key_f64_ref(np.sort(f64_key_ref(v[keep])))


# ------------------------------------------------------------------ models
def value_summary_ref(values, positive_only) -> dict:
    s = sorted_selected(values, positive_only)
    c = int(s.shape[0])
    out = {"count": c, "sum": 0.0, "sum_abs": 0.0}
    out.update(dict.fromkeys(PICKS, 0))
    if c:
        rank = {"min": 0, "max": c - 1, "median": c // 2, "p95": int(c * 0.95),
                "p99": int(c * 0.99)}
        u = s.view(np.uint64)
        out.update({k: int(u[r]) for k, r in rank.items()})
        out["sum"] = math.fsum(s.tolist())
        out["sum_abs"] = math.fsum(np.abs(s).tolist())
    return out


def sum_bound(c, sum_abs) -> float:
    m = -(-int(c) // SUM_CHUNK)
    h = SUM_CHUNK // SUM_THREADS + 8 + -(-m // SUM_THREADS) + 8
    return (h + 1) * 2.0**-53 * sum_abs


def response_summary_ref(status_id, ctype_id, has_error, latency, n_status, n_ctype) -> dict:
    return {
        "status_counts": np.bincount(status_id, minlength=n_status).astype(np.uint64),
        "ctype_counts": np.bincount(ctype_id, minlength=n_ctype).astype(np.uint64),
        "error_count": int(np.count_nonzero(has_error)),
        "latency": value_summary_ref(latency, True),
    }


def segment_summary_ref(svc, ep, is_error, latency, start, ns, ne) -> dict:
    lat = np.asarray(latency, np.int64)
    st = np.asarray(start, np.int64)
    lat = lat[lat > 0]
    st = st[st != 0]
    return {
        "service_counts": np.bincount(svc, minlength=ns).astype(np.uint64),
        "endpoint_counts": np.bincount(ep, minlength=ne).astype(np.uint64),
        "total": int(np.shape(svc)[0]),
        "error_count": int(np.count_nonzero(np.asarray(is_error) == 1)),
        "latency_count": int(lat.shape[0]),
        "latency_sum": sum(lat.tolist()),
        "latency_min": int(lat.min()) if lat.shape[0] else 0,
        "latency_max": int(lat.max()) if lat.shape[0] else 0,
        "start_count": int(st.shape[0]),
        "start_min": int(st.min()) if st.shape[0] else 0,
        "start_max": int(st.max()) if st.shape[0] else 0,
    }


# ------------------------------------------------------------------ value inputs
SIZES = (1, 4095, 4096, 4097)       # one value; a tile less one, a tile, a tile and one
PERM_SMALL, PERM_LARGE = 100_001, 4_300_000
N_SPECIAL = 100_003
N_COUNT = 600_001                   # rows of the counting cases
ID_WIDTHS = (LDS_IDS, LDS_IDS + 1)  # the widest LDS table and the first global one


def mixed_values(n, seed=None) -> np.ndarray:
    """Lognormal values with about 5 % zeros (of both signs), 5 % distinct
    negatives and 2 % NaN mixed in; the first value stays positive."""
    rng = np.random.default_rng(n if seed is None else seed)
    v = rng.lognormal(3, 1.5, n)
    r = rng.random(n)
    v[r < 0.05] = 0.0
    v[r < 0.025] = -0.0
    neg = (r >= 0.05) & (r < 0.10)
    v[neg] = -v[neg]
    v[(r >= 0.10) & (r < 0.12)] = np.nan
    v[0] = abs(v[0]) if v[0] == v[0] and v[0] != 0 else 1.5
    return v


def n_dropped(c) -> int:
    return c // 50


def permutation_values(c, seed=3) -> np.ndarray:
    """A random permutation of 1..c as doubles with c // 50 values the
    positive filter drops (0.0, -0.0, -3.0, NaN) at random positions."""
    rng = np.random.default_rng(seed)
    d = n_dropped(c)
    n = c + d
    hole = np.zeros(n, bool)
    hole[rng.choice(n, d, replace=False)] = True
    v = np.empty(n, np.float64)
    v[~hole] = rng.permutation(c) + 1.0
    v[hole] = np.array([0.0, -0.0, -3.0, np.nan])[rng.integers(0, 4, d)]
    return v


def permutation_expected(c) -> dict:
    """What the positive values 1..c summarise to, exactly."""
    return {"count": c, "min": 1.0, "max": float(c), "median": float(c // 2 + 1),
            "p95": float(int(c * 0.95) + 1), "p99": float(int(c * 0.99) + 1),
            "sum": float(c * (c + 1) // 2)}


# the signed and special input: how many of each kind
SPECIAL_NAN = 1000         # half with the sign bit
SPECIAL_ZEROS = 50         # of each sign
SPECIAL_SUBNORMAL = 100    # of each sign, +-5e-324 among them
SPECIAL_INF = 3
SPECIAL_NEG = 49_452       # negatives, the subnormal ones included
# the kept count is odd and the negatives are one fewer than half of the rest,
# so the median (rank c // 2) is the last -0.0 and rank c // 2 + 1 the first +0.0


def special_values(with_inf=True, seed=11) -> np.ndarray:
    """N_SPECIAL values: normals of both signs spread over 1e-300 .. 1e300
    (distinct with probability 1), 50 zeros of each sign, 100 subnormals of
    each sign (+-5e-324 among them), 1000 NaNs (half with the sign bit, some
    with a payload) and, with_inf, three +inf (else three 1e300); no -inf."""
    rng = np.random.default_rng(seed)
    kept = N_SPECIAL - SPECIAL_NAN
    n_pos = kept - SPECIAL_NEG - 2 * SPECIAL_ZEROS
    sub = rng.integers(2, 2**52, SPECIAL_SUBNORMAL - 1, dtype=np.uint64)
    sub = np.r_[np.uint64(1), sub].view(np.float64)          # bits 1 = 5e-324
    neg = -(10.0 ** rng.uniform(-300, 300, SPECIAL_NEG - SPECIAL_SUBNORMAL))
    pos = 10.0 ** rng.uniform(-300, 300, n_pos - SPECIAL_SUBNORMAL - SPECIAL_INF)
    nan = np.full(SPECIAL_NAN, 0x7FF8000000000000, np.uint64)
    nan[::2] |= SIGN
    nan[: SPECIAL_NAN // 2] |= rng.integers(1, 2**50, SPECIAL_NAN // 2, dtype=np.uint64)
    v = np.r_[neg, -sub, np.full(SPECIAL_ZEROS, -0.0), np.zeros(SPECIAL_ZEROS), sub, pos,
              np.full(SPECIAL_INF, np.inf if with_inf else 1e300), nan.view(np.float64)]
    assert v.shape == (N_SPECIAL,)
    return v[rng.permutation(N_SPECIAL)]


def dropped_values(n=2 * TILE + 5, seed=5) -> np.ndarray:
    """Nothing the positive filter keeps: zeros, negatives, -inf and NaN."""
    rng = np.random.default_rng(seed)
    return np.array([0.0, -0.0, -1.5, -5e-324, -np.inf, np.nan])[rng.integers(0, 6, n)]


# ------------------------------------------------------------------ counting inputs
def skewed_ids(n, n_ids, rng) -> np.ndarray:
    """About 90 % of the rows on one id, the rest uniform; id 0 and the
    largest id are both present (rows 0 and n - 1)."""
    ids = rng.integers(0, n_ids, n)
    ids[rng.random(n) < 0.9] = n_ids // 3
    ids[0] = 0
    ids[-1] = n_ids - 1
    return ids.astype(np.uint32)


def response_inputs(n, n_status, n_ctype, seed=21) -> dict:
    rng = np.random.default_rng(seed)
    return {
        "status_id": skewed_ids(n, n_status, rng),
        "ctype_id": skewed_ids(n, n_ctype, rng),
        "has_error": np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, n)],
        "latency": mixed_values(n, seed + 1),
        "n_status": n_status, "n_ctype": n_ctype,
    }


def segment_inputs(n, ns, ne, seed=31) -> dict:
    """is_error from {0, 1, 2, -1, INT32_MIN}; latencies in [-10, 2^40], 5 % of
    them in [-10, 0]; start times of both signs with 5 % zeros and, from three
    rows on, one row each of INT64_MIN and INT64_MAX and a latency of 2^40."""
    rng = np.random.default_rng(seed)
    start = rng.integers(-2**62, 2**62, n)
    start[rng.random(n) < 0.05] = 0
    latency = rng.integers(1, 2**40, n, endpoint=True)
    low = rng.random(n) < 0.05
    latency[low] = rng.integers(-10, 0, int(low.sum()), endpoint=True)
    if n >= 3:
        start[n // 3] = INT64_MIN
        start[2 * n // 3] = INT64_MAX
        latency[n // 2] = 2**40
    return {
        "svc": skewed_ids(n, ns, rng),
        "ep": skewed_ids(n, ne, rng),
        "is_error": np.array([0, 1, 2, -1, INT32_MIN], np.int32)[rng.integers(0, 5, n)],
        "latency": latency,
        "start": start,
        "ns": ns, "ne": ne,
    }


def response_ref(inp: dict) -> dict:
    return response_summary_ref(inp["status_id"], inp["ctype_id"], inp["has_error"],
                                inp["latency"], inp["n_status"], inp["n_ctype"])


def segment_ref(inp: dict) -> dict:
    return segment_summary_ref(inp["svc"], inp["ep"], inp["is_error"], inp["latency"],
                               inp["start"], inp["ns"], inp["ne"])

"""Summary entry points, host side (no GPU): the reference helper
(tests/summary_ref.py) against the goldens the reference's own scripts wrote,
the key order of csrc/radix.h on a hand-written list, and the premises the GPU
cases (tests/test_gpu_summaries.py) rely on for the inputs they build."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from oracle import spec

import summary_ref as R

NEG_ZERO = 0x8000000000000000


# ------------------------------------------------------------------ C ABI
def test_library_exports_summary_entry_points():
    lib = anomod.lib()
    for name in ("anomod_value_summary", "anomod_response_summary", "anomod_segment_summary"):
        assert name in anomod.EXPORTED_SYMBOLS and hasattr(lib, name)
    out = L.ValueSummaryC()
    assert lib.anomod_value_summary(None, None, 0, 1, C.byref(out)) == L.EINVAL
    assert b"anomod_value_summary" in lib.anomod_last_error(None)
    assert C.sizeof(L.ValueSummaryC) == 7 * 8      # the GPU tests read it as 7 words


# ------------------------------------------------------------------ goldens
def test_value_model_gives_the_golden_latency_picks(golden):
    cases = json.loads((golden / "api_summary.json").read_text())
    assert cases
    for c in cases:
        lat = [r.get("latency_ms", 0) for r in c["responses"]]
        want = spec.latency_picks([x for x in lat if x > 0])
        assert want == json.loads(c["summary_json"])["latency_statistics"]
        ref = R.value_summary_ref(np.asarray(lat, np.float64), True)
        assert ref["count"] == sum(x > 0 for x in lat)
        for k in R.PICKS:
            got = float(np.uint64(ref[k]).view(np.float64))
            assert got == want[k], k
        # Python's left-to-right sum of n positive values is within n * 2^-53 of the exact one
        n = ref["count"]
        assert abs(ref["sum"] / n - want["mean"]) <= (n + 1) * 2.0**-53 * want["mean"]
        assert ref["sum_abs"] == ref["sum"]


def test_segment_model_gives_the_golden_analysis(golden):
    g = json.loads((golden / "analyze_patterns.json").read_text())
    seg = anomod.SegmentSet.from_es(g["segments"])
    ref = R.segment_summary_ref(seg.svc, seg.endpoint, seg.is_error, seg.latency, seg.start_time,
                                len(seg.services), len(seg.endpoints))
    want = g["analysis"]
    assert ref["total"] == want["total_traces"] and ref["error_count"] == want["error_traces"]
    assert dict(zip(seg.services, ref["service_counts"].tolist())) == want["service_call_counts"]
    assert dict(zip(seg.endpoints, ref["endpoint_counts"].tolist())) == \
        want["endpoint_call_counts"]
    stats = want["latency_stats"]
    assert (ref["latency_min"], ref["latency_max"], ref["latency_count"]) == \
        (stats["min"], stats["max"], stats["count"])
    assert ref["latency_sum"] / ref["latency_count"] == stats["avg"]
    assert ref["start_min"] == want["time_range"]["earliest"]
    assert ref["start_max"] == want["time_range"]["latest"]
    assert all(type(v) is int for k, v in ref.items() if not k.endswith("_counts"))


def test_segment_model_empty_selections():
    ref = R.segment_summary_ref([0, 0], [0, 0], [1, 1], [0, -4], [0, 0], 1, 1)
    assert [ref[k] for k in ("latency_count", "latency_sum", "latency_min", "latency_max",
                             "start_count", "start_min", "start_max")] == [0] * 7
    assert ref["error_count"] == 2 and ref["service_counts"].tolist() == [2]


# ------------------------------------------------------------------ key order
ORDERED = [-np.inf, -1e300, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, np.inf]


def test_key_order_of_a_hand_written_list():
    want = R.bits(ORDERED)
    assert want[4] == NEG_ZERO and want[5] == 0 and want[3] == NEG_ZERO | 1
    for seed in range(5):
        v = np.asarray(ORDERED)[np.random.default_rng(seed).permutation(len(ORDERED))]
        got = R.sorted_selected(v, 0)
        np.testing.assert_array_equal(got.view(np.uint64), want)
    keys = R.f64_key_ref(ORDERED).tolist()
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # with the positive filter only the last three are left
    np.testing.assert_array_equal(R.sorted_selected(ORDERED, 1).view(np.uint64), want[6:])


def test_key_round_trip():
    rng = np.random.default_rng(1)
    k = np.r_[rng.integers(0, 2**64, 10_000, dtype=np.uint64), R.f64_key_ref(ORDERED),
              np.array([0, 2**63 - 1, 2**63, 2**64 - 1], np.uint64)]
    np.testing.assert_array_equal(R.f64_key_ref(R.key_f64_ref(k)), k)
    v = R.special_values()
    np.testing.assert_array_equal(R.key_f64_ref(R.f64_key_ref(v)).view(np.uint64), R.bits(v))


def test_value_model_picks_of_a_small_list():
    ref = R.value_summary_ref([3.0, np.nan, -2.0, 0.0, 7.5, -0.0, 1.0], 0)
    s = [-2.0, -0.0, 0.0, 1.0, 3.0, 7.5]
    want = {"min": s[0], "max": s[5], "median": s[3], "p95": s[5], "p99": s[5]}
    assert ref["count"] == 6 and ref["sum"] == 9.5 and ref["sum_abs"] == 13.5
    assert {k: ref[k] for k in R.PICKS} == {k: int(R.bits([x])[0]) for k, x in want.items()}
    none = R.value_summary_ref([np.nan, -1.0, 0.0], 1)
    assert none == dict.fromkeys(("count", "sum", "sum_abs") + R.PICKS, 0)


def test_sum_bound():
    # one chunk: 64 + 8 + 1 + 8 additions and fsum's rounding
    assert R.sum_bound(1, 1.0) == 82 * 2.0**-53 == R.sum_bound(R.SUM_CHUNK, 1.0)
    assert R.sum_bound(R.SUM_CHUNK * R.SUM_THREADS + 1, 2.0) == 83 * 2.0**-52
    assert R.sum_bound(R.PERM_LARGE, 1.0) == 83 * 2.0**-53


# ------------------------------------------------------------------ premises: value cases
@pytest.mark.parametrize("n", R.SIZES)
def test_mixed_values_premises(n):
    v = R.mixed_values(n)
    assert v.shape == (n,) and v[0] > 0
    if n == 1:
        return
    assert np.isnan(v).any() and (v < 0).any() and (v > 0).any()
    z = R.bits(v[v == 0])
    assert (z == 0).any() and (z == NEG_ZERO).any()
    neg = v[v < 0]
    assert np.unique(neg).shape[0] == neg.shape[0] > 100
    for positive_only in (0, 1):
        ref = R.value_summary_ref(v, positive_only)
        assert 0 < ref["count"] < n


@pytest.mark.parametrize("c", [R.PERM_SMALL, R.PERM_LARGE])
def test_permutation_premises(c):
    n = c + R.n_dropped(c)
    assert c * (c + 1) // 2 < 2**53            # every partial sum is an exact integer
    if c == R.PERM_LARGE:
        assert c > R.SUM_THREADS * R.SUM_CHUNK     # sum_parts_kernel: a lane adds two chunk sums
        assert n > R.SCAN_BATCH * R.TILE           # select_scan_kernel: a second batch of tiles
    v = R.permutation_values(c)
    assert v.shape == (n,)
    keep = v > 0
    np.testing.assert_array_equal(np.sort(v[keep]), np.arange(1, c + 1, dtype=np.float64))
    drop = v[~keep]
    assert np.isnan(drop).any() and (drop == -3.0).any()
    assert (R.bits(drop) == 0).any() and (R.bits(drop) == NEG_ZERO).any()
    # dropped values lie in the first batch of tiles and after it, so the
    # carried total is not simply a tile index times the tile size
    assert (~keep[: R.TILE]).any() and (~keep[-R.TILE:]).any()
    want = R.permutation_expected(c)
    ref = R.value_summary_ref(v, True)
    assert ref["count"] == want["count"] and ref["sum"] == want["sum"] == ref["sum_abs"]
    for k in R.PICKS:
        assert ref[k] == int(R.bits([want[k]])[0]), k


def test_special_values_premises():
    v = R.special_values()
    u = R.bits(v)
    assert v.shape == (R.N_SPECIAL,)
    nan = np.isnan(v)
    assert (u[nan] >> np.uint64(63) == 1).any() and (u[nan] >> np.uint64(63) == 0).any()
    assert np.isposinf(v).sum() == R.SPECIAL_INF and not np.isneginf(v).any()
    with np.errstate(invalid="ignore"):
        sub = (np.abs(v) > 0) & (np.abs(v) < 2.0**-1022)
        neg, pos = v[v < 0], v[(v > 0) & np.isfinite(v)]
    assert (v[sub] > 0).sum() == (v[sub] < 0).sum() == R.SPECIAL_SUBNORMAL
    assert (u == 1).any() and (u == NEG_ZERO | 1).any()          # +-5e-324
    assert np.unique(neg).shape[0] == neg.shape[0] == R.SPECIAL_NEG
    assert neg.min() < -1e290 and neg[neg < -2.0**-1022].max() > -1e-290
    assert pos.max() > 1e290 and pos[pos > 2.0**-1022].min() < 1e-290
    # key order: the median is the last -0.0, the next rank the first +0.0
    s = R.sorted_selected(v, 0).view(np.uint64)
    c = s.shape[0]
    assert c == R.N_SPECIAL - R.SPECIAL_NAN
    assert s[c // 2] == NEG_ZERO and s[c // 2 + 1] == 0 and s[c // 2 - 1] == NEG_ZERO
    ref = R.value_summary_ref(v, 0)
    assert ref["median"] == NEG_ZERO and ref["sum"] == math.inf
    assert ref["max"] == int(R.bits([np.inf])[0]) and ref["min"] == int(R.bits([neg.min()])[0])
    # finite twin: the same ranks, a sum that cancels
    f = R.special_values(with_inf=False)
    assert np.isfinite(f[~np.isnan(f)]).all()
    np.testing.assert_array_equal(R.bits(f)[~np.isposinf(v)], u[~np.isposinf(v)])
    fin = R.value_summary_ref(f, 0)
    assert fin["median"] == NEG_ZERO and math.isfinite(fin["sum"])
    assert abs(fin["sum"]) < 0.9 * fin["sum_abs"]
    # positive filter: +inf and the positive subnormals stay
    p = R.value_summary_ref(v, 1)
    assert p["count"] == c - R.SPECIAL_NEG - 2 * R.SPECIAL_ZEROS
    assert p["min"] == 1 and p["max"] == int(R.bits([np.inf])[0]) and p["sum"] == math.inf


def test_dropped_values_premises():
    v = R.dropped_values()
    assert v.shape[0] > 2 * R.TILE
    assert set(R.bits(v).tolist()) == set(R.bits([0.0, -0.0, -1.5, -5e-324, -np.inf,
                                                  np.nan]).tolist())
    assert R.value_summary_ref(v, 1)["count"] == 0


# ------------------------------------------------------------------ premises: counting cases
def test_counting_sizes():
    # some thread of a grid of 2 * CUs workgroups takes a second grid-stride step
    assert R.N_COUNT > 2 * R.MI355X_CUS * R.COUNT_THREADS
    assert R.ID_WIDTHS == (R.LDS_IDS, R.LDS_IDS + 1)


@pytest.mark.parametrize("n_ids", R.ID_WIDTHS)
def test_skewed_ids_premises(n_ids):
    ids = R.skewed_ids(R.N_COUNT, n_ids, np.random.default_rng(n_ids))
    assert ids.dtype == np.uint32 and int(ids.max()) == n_ids - 1 and int(ids.min()) == 0
    count = np.bincount(ids, minlength=n_ids)
    assert 0.89 < count[n_ids // 3] / R.N_COUNT < 0.92
    assert np.count_nonzero(count) > 0.99 * n_ids
    assert R.skewed_ids(1, 1, np.random.default_rng(0)).tolist() == [0]


def test_response_inputs_premises():
    inp = R.response_inputs(R.N_COUNT, *R.ID_WIDTHS)
    assert set(np.unique(inp["has_error"]).tolist()) == {0, 1, 2, 255}
    lat = inp["latency"]
    assert np.isnan(lat).any() and (lat < 0).any() and (lat == 0).any()
    ref = R.response_ref(inp)
    assert int(ref["status_counts"].sum()) == int(ref["ctype_counts"].sum()) == R.N_COUNT
    assert ref["status_counts"].shape == (R.LDS_IDS,)
    assert ref["ctype_counts"].shape == (R.LDS_IDS + 1,)
    assert 0.7 * R.N_COUNT < ref["error_count"] < 0.8 * R.N_COUNT
    assert 0 < ref["latency"]["count"] < R.N_COUNT


def test_segment_inputs_premises():
    inp = R.segment_inputs(R.N_COUNT, *R.ID_WIDTHS)
    assert set(np.unique(inp["is_error"]).tolist()) == {0, 1, 2, -1, R.INT32_MIN}
    lat, st = inp["latency"], inp["start"]
    assert lat.dtype == np.int64 and st.dtype == np.int64
    assert int(lat.min()) == -10 and int(lat.max()) == 2**40 and (lat == 0).any()
    assert (st == R.INT64_MIN).sum() == 1 and (st == R.INT64_MAX).sum() == 1
    assert 0.04 < (st == 0).mean() < 0.06
    assert (st < 0).sum() > R.N_COUNT // 3 and (st > 0).sum() > R.N_COUNT // 3
    ref = R.segment_ref(inp)
    assert 2**53 < ref["latency_sum"] < 2**63
    assert ref["start_min"] == R.INT64_MIN and ref["start_max"] == R.INT64_MAX
    assert 0 < ref["error_count"] < R.N_COUNT
    # without the two extreme rows the minimum is still negative
    assert int(np.sort(st)[1]) < 0

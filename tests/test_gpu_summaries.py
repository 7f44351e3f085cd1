"""GPU: the three summary entry points at the C ABI against the host models of
tests/summary_ref.py — anomod_value_summary (csrc/summary.hip over the select /
sort / sum of csrc/radix.hip), anomod_response_summary (category_count_kernel)
and anomod_segment_summary (csrc/segments.hip).

Counts, picks (as bit patterns) and every integer field are compared exactly.
The one tolerance is summary_ref.sum_bound, the rounding the fixed-order sum
may show against math.fsum, derived from the kernels' addition order; each sum
case prints its error / bound ratio before it asserts.

Code paths by case:
  sizes               one value; 4095 / 4096 / 4097 values: a short tile, a
                      full tile, a second tile of one value; both filters
  permutation         the kept multiset exactly (count, ranks, integer sum);
                      at 4 300 000 kept values select_scan_kernel carries its
                      total into a second batch of 1024 tiles and a lane of
                      sum_parts_kernel adds two chunk sums
  signed and special  f64_key / key_f64 on negatives, both zeros, subnormals,
                      +inf and NaNs of both signs; the median sits on the last
                      -0.0 with the first +0.0 at the next rank
  response widths     category_count_kernel<LDS_A, LDS_B> for 4096 / 4097 ids
                      on either side: all four forms, a second grid-stride
                      step, LDS flushes of many workgroups into one counter
  segment widths      segment_summary_kernel<LDS_SVC, LDS_EP> likewise, signed
                      64-bit atomic min / max down to INT64_MIN, a latency sum
                      beyond 2^53"""
import ctypes as C
import functools
import math
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L

import summary_ref as R

pytestmark = pytest.mark.gpu

WORDS = ("count", "min", "max", "sum", "median", "p95", "p99")   # anomod_value_summary_out


# ------------------------------------------------------------------ calls
def _words(out: L.ValueSummaryC) -> dict:
    """The structure's seven 8-byte fields as unsigned integers."""
    return dict(zip(WORDS, np.frombuffer(out, np.uint64).tolist()))


def _value_summary(ctx, values, positive_only):
    v = np.ascontiguousarray(values, np.float64)
    out = L.ValueSummaryC(7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0)
    rc = ctx._lib.anomod_value_summary(ctx.handle, L.ptr(v if v.size else None, C.c_double),
                                       v.size, positive_only, C.byref(out))
    assert rc == L.OK, ctx._lib.anomod_last_error(ctx.handle)
    return _words(out), out.sum


def _assert_value(got, ref: dict, what):
    """Count and picks bit for bit (the sum is checked by _assert_sum)."""
    words, _ = got
    for k in ("count",) + R.PICKS:
        assert words[k] == ref[k], (what, k, hex(words[k]), hex(ref[k]))


def _assert_sum(got, ref: dict, what):
    _, total = got
    if math.isinf(ref["sum"]) or ref["count"] == 0:
        assert total == ref["sum"], what
        return
    err, bound = abs(total - ref["sum"]), R.sum_bound(ref["count"], ref["sum_abs"])
    print(f"sum {what}: c={ref['count']} error={err:.3e} bound={bound:.3e} "
          f"ratio={err / bound if bound else 0.0:.4f}")
    assert err <= bound, what


def _assert_all_zero(got, what):
    words, _ = got
    assert words == dict.fromkeys(WORDS, 0), what


def _response(ctx, inp, fill=0):
    n = int(inp["status_id"].shape[0])
    sc = np.full(inp["n_status"], fill, np.uint64)
    cc = np.full(inp["n_ctype"], fill, np.uint64)
    out = L.ResponseSummaryC(inp["n_status"], inp["n_ctype"], L.ptr(sc, C.c_uint64),
                             L.ptr(cc, C.c_uint64), 7, L.ValueSummaryC(7, 7.0, 7.0, 7.0, 7.0, 7.0,
                                                                       7.0))
    cols = [np.ascontiguousarray(inp[k], t) for k, t in
            (("status_id", np.uint32), ("ctype_id", np.uint32), ("has_error", np.uint8),
             ("latency", np.float64))]
    rc = ctx._lib.anomod_response_summary(
        ctx.handle, L.ptr(cols[0], C.c_uint32), L.ptr(cols[1], C.c_uint32),
        L.ptr(cols[2], C.c_uint8), L.ptr(cols[3], C.c_double), n, C.byref(out))
    return rc, sc, cc, out


def _check_response(ctx, inp, what):
    rc, sc, cc, out = _response(ctx, inp, fill=0xDEADBEEF)
    assert rc == L.OK, ctx._lib.anomod_last_error(ctx.handle)
    ref = R.response_ref(inp)
    np.testing.assert_array_equal(sc, ref["status_counts"], err_msg=what)
    np.testing.assert_array_equal(cc, ref["ctype_counts"], err_msg=what)
    assert out.error_count == ref["error_count"], what
    lat = _words(out.latency), out.latency.sum
    _assert_value(lat, ref["latency"], what)
    _assert_sum(lat, ref["latency"], what)
    return sc, cc, out


SEG_SCALARS = ("total", "error_count", "latency_count", "latency_sum", "latency_min",
               "latency_max", "start_count", "start_min", "start_max")


def _segment(ctx, inp, counts=(True, True)):
    n = int(inp["svc"].shape[0])
    sc = np.full(inp["ns"], 0xDEADBEEF, np.uint64) if counts[0] else None
    ec = np.full(inp["ne"], 0xDEADBEEF, np.uint64) if counts[1] else None
    out = L.SegmentSummaryC(inp["ns"], inp["ne"], L.ptr(sc, C.c_uint64), L.ptr(ec, C.c_uint64),
                            7, 7, 7, 7, 7, 7, 7, 7, 7)
    cols = [np.ascontiguousarray(inp[k], t) for k, t in
            (("svc", np.uint32), ("ep", np.uint32), ("is_error", np.int32),
             ("latency", np.int64), ("start", np.int64))]
    rc = ctx._lib.anomod_segment_summary(
        ctx.handle, L.ptr(cols[0], C.c_uint32), L.ptr(cols[1], C.c_uint32),
        L.ptr(cols[2], C.c_int32), L.ptr(cols[3], C.c_int64), L.ptr(cols[4], C.c_int64), n,
        C.byref(out))
    return rc, sc, ec, {k: int(getattr(out, k)) for k in SEG_SCALARS}


def _check_segment(ctx, inp, what, ref=None):
    rc, sc, ec, got = _segment(ctx, inp)
    assert rc == L.OK, ctx._lib.anomod_last_error(ctx.handle)
    ref = R.segment_ref(inp) if ref is None else ref
    np.testing.assert_array_equal(sc, ref["service_counts"], err_msg=what)
    np.testing.assert_array_equal(ec, ref["endpoint_counts"], err_msg=what)
    assert got == {k: ref[k] for k in SEG_SCALARS}, what
    return sc, ec, got


# ------------------------------------------------------------------ value summary
@pytest.mark.parametrize("positive_only", [1, 0])
@pytest.mark.parametrize("n", R.SIZES)
def test_value_sizes_and_tiling(ctx, n, positive_only):
    v = R.mixed_values(n)
    ref = R.value_summary_ref(v, positive_only)
    got = _value_summary(ctx, v, positive_only)
    _assert_value(got, ref, n)
    _assert_sum(got, ref, f"mixed n={n} positive_only={positive_only}")


@pytest.mark.parametrize("c", [R.PERM_SMALL, R.PERM_LARGE])
def test_value_permutation_exact_multiset(ctx, c):
    """1..c in random order between dropped values: the count, every rank and
    the sum (all partial sums are integers below 2^53) are known exactly."""
    words, total = _value_summary(ctx, R.permutation_values(c), 1)
    want = R.permutation_expected(c)
    assert words["count"] == want["count"]
    for k in R.PICKS:
        assert words[k] == int(R.bits([want[k]])[0]), (k, hex(words[k]), want[k])
    assert total == want["sum"]


@pytest.fixture(scope="module")
def special():
    v, f = R.special_values(), R.special_values(with_inf=False)
    return {"inf": v, "finite": f, "ref_inf": R.value_summary_ref(v, 0),
            "ref_finite": R.value_summary_ref(f, 0), "ref_positive": R.value_summary_ref(v, 1)}


def test_value_signed_and_special(ctx, special):
    got = _value_summary(ctx, special["inf"], 0)
    _assert_value(got, special["ref_inf"], "signed, +inf")
    assert got[0]["median"] == 1 << 63          # -0.0: the zeros keep their order
    assert got[1] == math.inf
    got = _value_summary(ctx, special["finite"], 0)
    _assert_value(got, special["ref_finite"], "signed, finite")
    _assert_sum(got, special["ref_finite"], "signed, finite")
    got = _value_summary(ctx, special["inf"], 1)
    _assert_value(got, special["ref_positive"], "signed, positive filter")
    assert got[0]["min"] == 1                   # 5e-324 is kept
    assert got[1] == math.inf


def test_value_nothing_kept_and_nothing_given(ctx):
    v = R.dropped_values()
    _assert_all_zero(_value_summary(ctx, v, 1), "all dropped")
    _assert_all_zero(_value_summary(ctx, np.full(R.TILE + 1, np.nan), 0), "all NaN")
    _assert_all_zero(_value_summary(ctx, np.zeros(0), 1), "n = 0, NULL")
    _assert_all_zero(_value_summary(ctx, np.zeros(0), 0), "n = 0, NULL")
    # without the filter everything but the NaNs is kept, -inf included
    ref = R.value_summary_ref(v, 0)
    got = _value_summary(ctx, v, 0)
    _assert_value(got, ref, "unfiltered")
    assert got[1] == -math.inf == ref["sum"]


def test_value_sum_same_bits_every_run(ctx, special):
    first = _value_summary(ctx, special["finite"], 0)
    again = _value_summary(ctx, special["finite"], 0)
    with anomod.Context(0) as fresh:
        other = _value_summary(fresh, special["finite"], 0)
    assert first[0]["sum"] == again[0]["sum"] == other[0]["sum"]     # the sum's bit pattern
    assert first[0] == again[0] == other[0]


# ------------------------------------------------------------------ response summary
@functools.lru_cache(maxsize=None)
def _cus() -> int:
    """The device's CU count from torch.cuda.get_device_properties, asked once
    and in a child process: torch carries a HIP runtime of its own, which
    finds no device in a process where libanomod's has already opened it."""
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return int(r.stdout.split()[-1])


@pytest.mark.parametrize("n_ctype", R.ID_WIDTHS)
@pytest.mark.parametrize("n_status", R.ID_WIDTHS)
def test_response_all_four_kernel_forms(ctx, n_status, n_ctype):
    assert R.N_COUNT > 2 * _cus() * R.COUNT_THREADS     # a second grid-stride step
    _check_response(ctx, R.response_inputs(R.N_COUNT, n_status, n_ctype),
                    f"response {n_status} x {n_ctype}")


def test_response_small_and_degenerate(ctx):
    for n in (1, R.COUNT_THREADS + 1):
        _check_response(ctx, R.response_inputs(n, 3, 5), f"response n={n}")
        sc, cc, _ = _check_response(ctx, R.response_inputs(n, 1, 1), f"response n={n}, one id")
        assert sc.tolist() == [n] and cc.tolist() == [n]
    empty = {"status_id": np.zeros(0, np.uint32), "ctype_id": np.zeros(0, np.uint32),
             "has_error": np.zeros(0, np.uint8), "latency": np.zeros(0), "n_status": 6,
             "n_ctype": R.LDS_IDS + 1}
    rc, sc, cc, out = _response(ctx, empty, fill=0xDEADBEEF)   # garbage in the count buffers
    assert rc == L.OK
    assert not sc.any() and not cc.any() and out.error_count == 0
    _assert_all_zero((_words(out.latency), 0.0), "response n = 0")


def test_response_argument_errors(ctx):
    inp = R.response_inputs(3000, 7, 9)
    lib = ctx._lib
    sc0, cc0, out0 = _check_response(ctx, inp, "before")
    for col, width, name in (("status_id", "n_status", "status id"),
                             ("ctype_id", "n_ctype", "content-type id")):
        bad = dict(inp)
        bad[col] = inp[col].copy()
        bad[col][1234] = inp[width]
        rc, _, _, _ = _response(ctx, bad)
        assert rc == L.EINVAL
        msg = lib.anomod_last_error(ctx.handle).decode()
        assert f"{name} {inp[width]} >= {width} {inp[width]}" in msg, msg
    sc1, cc1, out1 = _check_response(ctx, inp, "after")
    np.testing.assert_array_equal(sc1, sc0)
    np.testing.assert_array_equal(cc1, cc0)
    assert out1.error_count == out0.error_count
    assert _words(out1.latency) == _words(out0.latency)


# ------------------------------------------------------------------ segment summary
@pytest.mark.parametrize("ne", R.ID_WIDTHS)
@pytest.mark.parametrize("ns", R.ID_WIDTHS)
def test_segment_all_four_kernel_forms(ctx, ns, ne):
    assert R.N_COUNT > 2 * _cus() * R.COUNT_THREADS
    inp = R.segment_inputs(R.N_COUNT, ns, ne)
    _, _, got = _check_segment(ctx, inp, f"segments {ns} x {ne}")
    assert got["start_min"] == R.INT64_MIN and got["start_max"] == R.INT64_MAX
    assert got["latency_sum"] > 2**53


def test_segment_negative_start_times_only(ctx):
    """Every start time negative: the maximum is negative too, and the
    minimum is not INT64_MIN."""
    inp = R.segment_inputs(5000, 3, 4)
    inp["start"] = -np.abs(inp["start"] // 4) - 1
    _, _, got = _check_segment(ctx, inp, "negative start times")
    assert R.INT64_MIN < got["start_min"] <= got["start_max"] < 0


def test_segment_empty_selections(ctx):
    inp = R.segment_inputs(5000, 3, 4)
    inp["latency"] = -np.abs(inp["latency"]) % 11 - 10           # [-10, 0]
    inp["latency"][::7] = 0
    _, _, got = _check_segment(ctx, inp, "no positive latency")
    assert [got[k] for k in ("latency_count", "latency_sum", "latency_min",
                             "latency_max")] == [0] * 4
    assert got["start_count"] > 0
    inp = R.segment_inputs(5000, 3, 4)
    inp["start"] = np.zeros(5000, np.int64)
    _, _, got = _check_segment(ctx, inp, "no start time")
    assert [got[k] for k in ("start_count", "start_min", "start_max")] == [0] * 3
    assert got["latency_count"] > 0
    one = {"svc": np.zeros(1, np.uint32), "ep": np.zeros(1, np.uint32),
           "is_error": np.ones(1, np.int32), "latency": np.array([R.INT64_MAX], np.int64),
           "start": np.array([-1], np.int64), "ns": 1, "ne": 1}
    _, _, got = _check_segment(ctx, one, "one row")
    assert got["latency_sum"] == got["latency_min"] == got["latency_max"] == R.INT64_MAX
    assert got["start_min"] == got["start_max"] == -1 and got["error_count"] == 1
    for n in (1, R.COUNT_THREADS + 1):
        _check_segment(ctx, R.segment_inputs(n, 2, 2), f"segments n={n}")
    none = {k: v[:0] if isinstance(v, np.ndarray) else v for k, v in one.items()}
    sc, ec, got = _check_segment(ctx, none, "segments n = 0")
    assert not sc.any() and not ec.any() and not any(got.values())


@pytest.mark.parametrize("ns,ne", [(5, 9), R.ID_WIDTHS[::-1]])
def test_segment_null_count_outputs(ctx, ns, ne):
    inp = R.segment_inputs(20_000, ns, ne)
    sc, ec, full = _check_segment(ctx, inp, "both vectors")
    for counts in ((False, True), (True, False), (False, False)):
        rc, s, e, got = _segment(ctx, inp, counts)
        assert rc == L.OK, ctx._lib.anomod_last_error(ctx.handle)
        assert got == full, counts
        assert (s is None) == (not counts[0]) and (e is None) == (not counts[1])
        if s is not None:
            np.testing.assert_array_equal(s, sc)
        if e is not None:
            np.testing.assert_array_equal(e, ec)


def test_segment_argument_errors(ctx):
    inp = R.segment_inputs(3000, 7, 9)
    lib = ctx._lib
    sc0, ec0, got0 = _check_segment(ctx, inp, "before")
    for col, width, name, wname in (("svc", "ns", "service id", "n_services"),
                                    ("ep", "ne", "endpoint id", "n_endpoints")):
        bad = dict(inp)
        bad[col] = inp[col].copy()
        bad[col][1234] = inp[width]
        rc, _, _, _ = _segment(ctx, bad)
        assert rc == L.EINVAL
        msg = lib.anomod_last_error(ctx.handle).decode()
        assert f"{name} {inp[width]} >= {wname} {inp[width]}" in msg, msg
    sc1, ec1, got1 = _check_segment(ctx, inp, "after")
    np.testing.assert_array_equal(sc1, sc0)
    np.testing.assert_array_equal(ec1, ec0)
    assert got1 == got0

"""GPU: the hand-written stable LSD radix sort (csrc/radix.hip) under the exact
order-statistic paths — the exact per-edge quantiles (§8a a11) and the API
value summary (§8f row 3), both restating the reference's sorted(x)[int(n*q)]
(monitor_http_responses.py:180-190).  Checked against numpy's stable sort:
ragged sizes around the 4096-key tile, every bit range the callers use,
duplicate-heavy keys, constant digits (skipped passes), and stability (keys
equal in the sorted bits keep their input order).

Below those, the sort is held to the exact model of tests/radix_ref.py (whole
output and pass count) on the inputs random keys do not reach:
  sizes          ragged last tiles of 1 / 64 / 65 keys, 256 and 257 tiles (the
                 tile scan's block border), 513 tiles (three scan blocks)
  bit ranges     all 2145 [b, e) with bits set on both sides of the range: a
                 begin_bit off the byte grid, a partial top digit, b == e
  pass lists     the 256 subsets of varying digits: P = 0..8, both parities of
                 the buffer choice, skipped digits between digits that run
  lone variation the one differing key past the first grid step of the OR /
                 AND reduction
  skew, rows     256 keys of one digit in a wave, 64-peer ballot groups,
                 digit == lane / row and other per-row patterns
  in != out      P = 1..8 through anomod_value_summary
  arguments      refused ranges leave the context usable; n = 0"""
import ctypes as C

import numpy as np
import pytest

from anomod import _lib as L

import radix_ref as R
import summary_ref as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 2, 63, 4095, 4096, 4097, 100_003, 2_000_000])
def test_sort_full_keys(ctx, n):
    rng = np.random.default_rng(n)
    k = rng.integers(0, 2**64, n, dtype=np.uint64)
    got, passes = ctx.sort_u64(k)
    np.testing.assert_array_equal(got, np.sort(k))
    assert passes == 8 or n < 3


@pytest.mark.parametrize("end_bit", [9, 16, 40, 44, 63])
def test_sort_bit_ranges_and_duplicates(ctx, end_bit):
    rng = np.random.default_rng(end_bit)
    n = 300_001
    # edge<<32 | dur style: few distinct high parts, heavy duplicates
    k = rng.integers(0, 2**min(end_bit, 20), n, dtype=np.uint64)
    if end_bit > 32:
        k = (rng.integers(0, 2**(end_bit - 32), n, dtype=np.uint64) << np.uint64(32)) | (k & 0xFFFF)
    got, _ = ctx.sort_u64(k, 0, end_bit)
    np.testing.assert_array_equal(got, np.sort(k))


def test_sort_is_stable_on_the_sorted_bits(ctx):
    """Sort by bits [32, 48) only: keys with equal bits 32..47 keep their
    input order (the low 32 bits carry the input position)."""
    rng = np.random.default_rng(3)
    n = 500_000
    hi = rng.integers(0, 300, n, dtype=np.uint64)
    k = (hi << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    got, passes = ctx.sort_u64(k, 32, 48)
    order = np.argsort(hi, kind="stable")
    np.testing.assert_array_equal(got, k[order])
    assert passes == 2  # bits 32-39 and 40-47 vary (hi < 300 < 2^9)


def test_sort_skips_constant_digits(ctx):
    rng = np.random.default_rng(4)
    k = (np.uint64(0xABCD) << np.uint64(40)) | rng.integers(0, 256, 50_000, dtype=np.uint64)
    got, passes = ctx.sort_u64(k)
    np.testing.assert_array_equal(got, np.sort(k))
    assert passes == 1
    same, passes = ctx.sort_u64(np.full(10_000, 7, np.uint64))
    assert passes == 0 and (same == 7).all()


# ------------------------------------------------------------------ exact model
# Everything below compares the whole output with radix_ref.sort_bits_ref and
# the pass count with radix_ref.passes_ref; the builders' premises (which
# border each input sits on) are asserted in tests/test_radix_ref_host.py.
def _check(ctx, k, b, e, what):
    got, passes = ctx.sort_u64(k, b, e)
    np.testing.assert_array_equal(got, R.sort_bits_ref(k, b, e), err_msg=str(what))
    assert passes == R.passes_ref(k, b, e), what


@pytest.mark.parametrize("kind", ["random", "duplicates"])
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_on_the_tile_and_scan_borders(ctx, n, kind):
    """Ragged last tiles of 1, 64, 65 and 4095 keys; 256 and 257 tiles (one
    full scan block, a second of one tile); 513 tiles (three scan blocks)."""
    if kind == "random":
        k, (b, e) = R.random_keys(n, n), (0, 64)
    else:
        k, (b, e), _ = R.duplicate_keys(n, n)
    _check(ctx, k, b, e, (n, kind))


def test_every_bit_range(ctx):
    """All 2145 ranges 0 <= b <= e <= 64 on full 64-bit keys: bits below b and
    at or above e are set in the keys and must not affect the order; keys equal
    in the sorted bits keep their input order (b == e: the input comes back)."""
    k = R.random_keys(R.N_RANGES, 0)
    bad = []
    for b, e in R.BIT_RANGES:
        got, passes = ctx.sort_u64(k, b, e)
        if not np.array_equal(got, R.sort_bits_ref(k, b, e)) or passes != R.passes_ref(k, b, e):
            bad.append((b, e, passes))
    assert not bad, f"{len(bad)} of {len(R.BIT_RANGES)} ranges wrong, first (b, e, passes) = {bad[0]}"


def test_every_pass_list(ctx):
    """Keys varying in exactly the digits of each of the 256 masks: every pass
    count 0..8 at both parities of the buffer choice, skipped digits at the
    ends and between two digits that run."""
    bad = []
    for mask8 in range(256):
        k, (b, e), _ = R.digit_subset(mask8)
        got, passes = ctx.sort_u64(k, b, e)
        if passes != bin(mask8).count("1") or not np.array_equal(got, R.sort_bits_ref(k, b, e)):
            bad.append((mask8, passes))
    assert not bad, f"{len(bad)} of 256 masks wrong, first (mask8, passes) = {bad[0]}"


@pytest.mark.parametrize("pos", R.LONE_POSITIONS)
@pytest.mark.parametrize("digit", range(R.DIGITS))
def test_lone_variation(ctx, digit, pos):
    """One key differs, in one bit: at the last position and at the first one
    the OR / AND reduction reaches only by a grid-stride step, and at 0."""
    k, (b, e), prem = R.lone_variation(R.N_LONE, digit, pos)
    got, passes = ctx.sort_u64(k, b, e)
    assert passes == 1 == R.passes_ref(k, b, e)
    np.testing.assert_array_equal(got, R.sort_bits_ref(k, b, e))
    assert got[prem["lands"]] == k[pos]


@pytest.mark.parametrize("j", R.SKEW_BYTES)
@pytest.mark.parametrize("D", R.SKEW_DIGITS)
def test_wave_skew(ctx, D, j):
    """Waves whose 256 keys all carry one digit (the u16 wave counter reaches
    256, every ballot group has 64 peers), two strays per tile at the corners;
    sorted by that digit alone and by all 64 bits, with and without a ragged
    third tile."""
    for tail in (0, 65):
        k, (b, e), _ = R.wave_skew(2, D, j, tail)
        _check(ctx, k, b, e, (D, j, tail, "digit"))
        _check(ctx, k, 0, 64, (D, j, tail, "full"))


@pytest.mark.parametrize("name", R.ROW_PATTERNS)
def test_row_patterns(ctx, name):
    for j in R.SKEW_BYTES:
        for tail in R.ROW_TAILS:
            k, (b, e), _ = R.row_patterns(j, tail)[name]
            _check(ctx, k, b, e, (name, j, tail, "digit"))
            _check(ctx, k, 0, 64, (name, j, tail, "full"))


@pytest.mark.parametrize("P", range(1, 9))
def test_separate_output_buffer_at_each_pass_count(ctx, P):
    """anomod_value_summary sorts from one buffer into another (in != out), as
    the quantile callers do: P passes for P = 1..8, so both parities of the
    buffer choice; count and picks bit for bit, the sum within sum_bound."""
    keys = R.summary_keys(P)
    assert R.passes_ref(keys, 0, 64) == P
    v = R.with_dropped(S.key_f64_ref(keys))
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(np.sort(S.f64_key_ref(v[v > 0])), np.sort(keys))
    out = L.ValueSummaryC(7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0)
    rc = ctx._lib.anomod_value_summary(ctx.handle, L.ptr(v, C.c_double), v.size, 1, C.byref(out))
    assert rc == L.OK, ctx._lib.anomod_last_error(ctx.handle)
    ref = S.value_summary_ref(v, True)
    words = dict(zip(("count", "min", "max", "sum", "median", "p95", "p99"),
                     np.frombuffer(out, np.uint64).tolist()))
    assert ref["count"] == R.N_SUBSET
    for f in ("count",) + S.PICKS:
        assert words[f] == ref[f], (P, f, hex(words[f]), hex(ref[f]))
    err, bound = abs(out.sum - ref["sum"]), S.sum_bound(ref["count"], ref["sum_abs"])
    print(f"sum P={P}: error={err:.3e} bound={bound:.3e}")
    assert err <= bound, P


@pytest.mark.parametrize("b,e", [(9, 8), (64, 0), (0, 65), (-1, 8), (-1, 65)])
def test_bad_bit_range_is_refused_and_the_context_still_sorts(ctx, b, e):
    k = R.random_keys(R.TILE + 1, 9)
    with pytest.raises(L.AnomodError):
        ctx.sort_u64(k, b, e)
    _check(ctx, k, 0, 64, "after the refusal")
    _check(ctx, k, 3, 30, "after the refusal")


def test_no_keys(ctx):
    for b, e in ((0, 64), (5, 5), (13, 40)):
        got, passes = ctx.sort_u64(np.zeros(0, np.uint64), b, e)
        assert got.shape == (0,) and got.dtype == np.uint64 and passes == 0

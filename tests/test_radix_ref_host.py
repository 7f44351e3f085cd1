"""Radix sort reference, host side (no GPU): tests/radix_ref.py against
restatements that share no method with it (Python's sorted on Python integers,
sets of digit values), and the premises its builders claim, which the GPU
cases of tests/test_gpu_radix.py rely on."""
from pathlib import Path

import numpy as np
import pytest

import radix_ref as R
import summary_ref as S

EDGE_RANGES = ((0, 0), (64, 64), (17, 17), (0, 1), (63, 64), (31, 32), (0, 64), (1, 64), (0, 63),
               (7, 9), (8, 16), (5, 62), (56, 64), (57, 64), (0, 57))


def _sorted_py(k, b, e):
    """Stable order by the sorted bits with Python's sorted on Python ints."""
    ints = [int(x) for x in k]
    m = 1 << (e - b)
    return [ints[i] for i in sorted(range(len(ints)), key=lambda i: (ints[i] >> b) % m)]


def _passes_py(k, b, e):
    ints = [int(x) for x in k]
    return sum(len({(x >> s) % (1 << min(8, e - s)) for x in ints}) > 1 for s in range(b, e, 8))


def _small_inputs():
    rng = np.random.default_rng(1)
    yield R.random_keys(257, 2)
    yield R.random_keys(300, 3) & np.uint64(0x0303030303030303)      # heavy ties in every digit
    yield rng.integers(0, 4, 200, dtype=np.uint64) << np.uint64(62)  # only the top two bits
    yield np.full(50, 0xDEADBEEF, np.uint64)
    yield R.random_keys(1, 4)
    yield np.zeros(0, np.uint64)


# ------------------------------------------------------------------ models
def test_sort_model_equals_python_sorted():
    rng = np.random.default_rng(0)
    ranges = list(EDGE_RANGES)
    for _ in range(40):
        b = int(rng.integers(0, 65))
        ranges.append((b, int(rng.integers(b, 65))))
    for k in _small_inputs():
        for b, e in ranges:
            assert R.sort_bits_ref(k, b, e).tolist() == _sorted_py(k, b, e), (k.size, b, e)


def test_sort_model_ignores_bits_outside_the_range_and_is_stable():
    k = R.random_keys(500, 5)
    for b, e in ((8, 16), (13, 29), (0, 5), (60, 64), (20, 20)):
        inside = np.uint64(((1 << (e - b)) - 1) << b)
        got = R.sort_bits_ref(k, b, e)
        assert sorted(got.tolist()) == sorted(k.tolist())
        v = (got & inside).astype(object)
        assert all(x <= y for x, y in zip(v[:-1], v[1:]))
        # the same order whatever the outside bits hold
        flipped = R.sort_bits_ref(k ^ ~inside, b, e)
        np.testing.assert_array_equal(flipped ^ ~inside, got)


def test_pass_model_equals_the_digit_value_sets():
    rng = np.random.default_rng(6)
    ranges = list(EDGE_RANGES) + [(int(b), int(rng.integers(b, 65)))
                                  for b in rng.integers(0, 65, 40)]
    inputs = list(_small_inputs())
    inputs += [R.digit_subset(m, 64)[0] for m in (0, 1, 0x80, 0x5A, 0xFF)]
    inputs.append(R.lone_variation(100, 3, 99)[0])
    for k in inputs:
        for b, e in ranges:
            assert R.passes_ref(k, b, e) == _passes_py(k, b, e), (k.size, b, e)


def test_constants_restate_the_kernel_source():
    import anomod
    src = (Path(anomod.__file__).resolve().parents[1] / "csrc" / "radix.hip").read_text()
    for line in ("constexpr int kWv = 64;", "constexpr int kSThreads = 1024;",
                 "constexpr int kSPer = 4;", "constexpr int kScanRows = 256;",
                 "std::min<uint64_t>((n + 255) / 256, 2048)"):
        assert line in src, line
    assert (R.WAVE, R.ROWS_PER_WAVE, R.SCAN_ROWS) == (64, 4, 256)
    assert R.TILE == S.TILE == 1024 * 4 and R.WAVES == 1024 // 64
    assert R.ORAND_THREADS == 2048 * 256


def test_lane_of_restates_the_scatter_index():
    want = {}
    for t in range(2):
        for w in range(R.WAVES):
            for k in range(R.ROWS_PER_WAVE):
                for lane in range(R.WAVE):
                    want[t * R.TILE + w * 256 + k * 64 + lane] = (t, w, k, lane)
    assert sorted(want) == list(range(2 * R.TILE))
    got = R.lane_of(np.arange(2 * R.TILE))
    assert [tuple(int(x[i]) for x in got) for i in range(2 * R.TILE)] == [want[i] for i in
                                                                          range(2 * R.TILE)]
    assert R.position_of(1, 15, 3, 63) == 2 * R.TILE - 1


# ------------------------------------------------------------------ sizes
def test_sizes_sit_on_the_tile_and_scan_borders():
    tiles = [-(-n // R.TILE) for n in R.SIZES]
    assert len(R.SIZES) == len(set(R.SIZES)) == 16
    assert {R.SCAN_ROWS, R.SCAN_ROWS + 1, 2 * R.SCAN_ROWS + 1} <= set(tiles)
    assert max(-(-t // R.SCAN_ROWS) for t in tiles) == 3           # three scan blocks
    last = {n - (-(-n // R.TILE) - 1) * R.TILE for n in R.SIZES if n > R.TILE}
    assert {1, 64, 65, R.TILE - 1, R.TILE} <= last                 # keys in the ragged last tile
    assert max(R.SIZES) * 8 <= 17 * 2**20
    assert R.N_RANGES == 2 * R.TILE + 1 and R.N_SUBSET == 3 * R.TILE + 17
    assert R.BIT_RANGES[0] == (0, 0) and R.BIT_RANGES[-1] == (64, 64) and (0, 64) in R.BIT_RANGES
    assert all(0 <= b <= e <= 64 for b, e in R.BIT_RANGES) and len(set(R.BIT_RANGES)) == 2145


def test_random_keys_set_bits_on_both_sides_of_every_range():
    k = R.random_keys(R.N_RANGES, 0)
    varies = int(np.bitwise_or.reduce(k)) ^ int(np.bitwise_and.reduce(k))
    assert varies == 2**64 - 1
    assert R.passes_ref(k, 0, 64) == 8


@pytest.mark.parametrize("n", R.SIZES)
def test_duplicate_keys_premises(n):
    k, (b, e), prem = R.duplicate_keys(n, n)
    v = R.sorted_bits(k, b, e)
    assert set(v.tolist()) <= set(R.DUP_VALUES) and prem["distinct"] == 7
    if n >= R.TILE - 1:
        assert len(set(v.tolist())) == 7 and R.passes_ref(k, b, e) == 3
    np.testing.assert_array_equal(k & np.uint64((1 << b) - 1), np.arange(n, dtype=np.uint64))
    if n >= 64:
        assert (k >> np.uint64(e)).any()                           # bits above the range are set
    # the three digits of the range each tell some of the 7 values apart
    for s in range(b, e, 8):
        w = min(8, e - s)
        assert len({(x >> (s - b)) % (1 << w) for x in R.DUP_VALUES}) > 1


# ------------------------------------------------------------------ builders
@pytest.mark.parametrize("pos", R.LONE_POSITIONS)
@pytest.mark.parametrize("digit", range(R.DIGITS))
def test_lone_variation_premises(digit, pos):
    k, (b, e), prem = R.lone_variation(R.N_LONE, digit, pos)
    assert (b, e) == (0, 64) and k.shape == (R.N_LONE,)
    assert prem["or_and_blocks"] == 2048                            # the grid is at its cap
    differs = np.flatnonzero(k != np.uint64(R.LONE_BASE))
    assert differs.tolist() == [pos]
    x = int(k[pos]) ^ R.LONE_BASE
    assert x == 1 << prem["bit"] and prem["bit"] // 8 == digit
    assert R.passes_ref(k, 0, 64) == 1
    assert [j for j in range(8) if R.passes_ref(k, 8 * j, 8 * j + 8)] == [digit]
    want = R.sort_bits_ref(k, 0, 64)
    assert np.flatnonzero(want != np.uint64(R.LONE_BASE)).tolist() == [prem["lands"]]
    assert prem["lands"] == (0 if int(k[pos]) < R.LONE_BASE else R.N_LONE - 1)


def test_lone_positions_lie_past_the_first_grid_step():
    n = R.N_LONE
    assert n == R.ORAND_THREADS + 77_777 and (n + 255) // 256 > 2048
    assert R.LONE_POSITIONS == (n - 1, R.ORAND_THREADS, 0)
    # positions a thread reaches without a stride step: 0 .. ORAND_THREADS - 1
    assert R.LONE_POSITIONS[0] >= R.ORAND_THREADS and R.LONE_POSITIONS[1] >= R.ORAND_THREADS
    assert R.LONE_POSITIONS[1] - 1 < R.ORAND_THREADS and R.LONE_POSITIONS[2] < R.ORAND_THREADS


@pytest.mark.parametrize("mask8", range(256))
def test_digit_subset_premises(mask8):
    k, (b, e), prem = R.digit_subset(mask8)
    assert (b, e) == (0, 64) and k.shape == (R.N_SUBSET,)
    popcount = bin(mask8).count("1")
    assert R.passes_ref(k, 0, 64) == popcount == len(prem["digits"])
    for j in range(R.DIGITS):
        values = set(R.digit_of(k, j).tolist())
        if mask8 >> j & 1:
            assert j in prem["digits"] and len(values) >= 3 and R.passes_ref(k, 8 * j, 8 * j + 8)
        else:
            assert values == {0xA5 ^ j} and 0 not in values
            assert R.passes_ref(k, 8 * j, 8 * j + 8) == 0


@pytest.mark.parametrize("j", R.SKEW_BYTES)
@pytest.mark.parametrize("D", R.SKEW_DIGITS)
def test_wave_skew_premises(D, j):
    n_tiles, tail = 2, 65
    k, (b, e), prem = R.wave_skew(n_tiles, D, j, tail)
    assert (b, e) == (8 * j, 8 * j + 8) and k.shape == (n_tiles * R.TILE + tail,)
    d = R.digit_of(k, j)
    tile, wave, row, lane = R.lane_of(np.arange(k.size))
    per_wave = np.zeros((n_tiles + 1, R.WAVES), np.int64)
    np.add.at(per_wave, (tile[d == D], wave[d == D]), 1)
    assert prem["full_wave_count"] == 256 and per_wave.max() == 256
    assert (per_wave[:n_tiles, 1:R.WAVES - 1] == 256).all()        # the u16 counter reaches 256
    assert (per_wave[:n_tiles, [0, R.WAVES - 1]] == 255).all()
    assert per_wave[n_tiles].tolist() == [tail] + [0] * (R.WAVES - 1)
    strays = np.flatnonzero(d != D)
    assert strays.tolist() == sorted(prem["strays"]) and len(strays) == 2 * n_tiles
    corners = [(int(wave[p]), int(row[p]), int(lane[p])) for p in strays]
    assert corners == list(R.SKEW_CORNERS) * n_tiles
    assert R.SKEW_CORNERS == ((0, 0, 0), (15, 3, 63))
    assert R.passes_ref(k, b, e) == 1                               # the pass is not skipped
    _assert_position_outside(k, j)


def _assert_position_outside(k, j):
    """The input position can be read back from the bits outside byte j."""
    low = k & np.uint64((1 << (8 * j)) - 1)
    high = (k >> np.uint64(8 * j + 8)) << np.uint64(8 * j) if j < 7 else np.uint64(0)
    np.testing.assert_array_equal(low | high, np.arange(k.size, dtype=np.uint64))


@pytest.mark.parametrize("tail", R.ROW_TAILS)
@pytest.mark.parametrize("j", R.SKEW_BYTES)
def test_row_pattern_premises(j, tail):
    pats = R.row_patterns(j, tail)
    assert tuple(pats) == R.ROW_PATTERNS and len(pats) == 8
    n = R.TILE + tail
    i = np.arange(n)
    _, _, row, lane = R.lane_of(i)
    for name, (k, (b, e), prem) in pats.items():
        assert k.shape == (n,) and (b, e) == (8 * j, 8 * j + 8), name
        d = R.digit_of(k, j)
        np.testing.assert_array_equal(d, prem["digit"], err_msg=name)
        _assert_position_outside(k, j)
        assert R.passes_ref(k, b, e) == 1, name
    dig = {name: R.digit_of(k, j) for name, (k, _, _) in pats.items()}
    np.testing.assert_array_equal(dig["lane"], lane)
    np.testing.assert_array_equal(dig["255-lane"], 255 - lane)
    np.testing.assert_array_equal(dig["row"], row)
    assert set(dig["two-by-lane"][lane % 2 == 0].tolist()) == {0x55}
    assert set(dig["two-by-lane"][lane % 2 == 1].tolist()) == {0xAA}
    t = dig["descending"][:R.TILE]
    assert t[0] == 255 and t[-1] == 0 and (np.diff(t) <= 0).all()
    assert (np.diff(dig["sorted"]) >= 0).all() and dig["sorted"][0] == 0
    assert len(set(dig["sorted"].tolist())) == 256
    s96, s97 = dig["sawtooth-4096"], dig["sawtooth-4097"]
    assert (np.diff(s96[:R.TILE]) >= 0).all() and s96[R.TILE - 1] == 255 and s96[R.TILE] == 0
    np.testing.assert_array_equal(s96[:R.TILE], s97[:R.TILE])
    assert s97[R.TILE] == 0 and (tail == 1 or s97[R.TILE + 1] == 0)
    # period 4097: key 4096 still belongs to the first tooth (value 4096 >> 4 = 256 -> 0 in 8 bits)
    assert (R.TILE % 4097) // 16 == 256


# ------------------------------------------------------------------ value-summary inputs
@pytest.mark.parametrize("P", range(1, 9))
def test_summary_keys_premises(P):
    k = R.summary_keys(P)
    assert k.shape == (R.N_SUBSET,) and R.passes_ref(k, 0, 64) == P
    assert [j for j in range(8) if R.passes_ref(k, 8 * j, 8 * j + 8)] == list(range(P))
    assert len(set(k.tolist())) == (256 if P == 1 else R.N_SUBSET)
    v = S.key_f64_ref(k)
    assert np.isfinite(v).all() and (v > 0).all()
    np.testing.assert_array_equal(S.f64_key_ref(v), k)
    top = set((k >> np.uint64(56)).tolist())
    assert top == ({0xBF, 0xC0} if P == 8 else {0xBF})
    mixed = R.with_dropped(v)
    assert mixed.shape[0] == R.N_SUBSET + R.N_SUBSET // 4
    with np.errstate(invalid="ignore"):
        kept = mixed[mixed > 0]
    assert np.isnan(mixed).any() and (mixed < 0).any() and (mixed == 0).any()
    assert sorted(kept.tolist()) == sorted(v.tolist())
    assert R.passes_ref(S.f64_key_ref(kept), 0, 64) == P
    assert not np.array_equal(kept, np.sort(kept))                  # shuffled

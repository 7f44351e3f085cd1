"""Reference for the stable LSD radix sort of csrc/radix.hip (a plain helper,
not a conftest): the order the sort must produce, the number of digit passes
it must run, and builders for the inputs that sit on the kernels' borders.

Order.  radix_sort_u64(keys, begin_bit b, end_bit e) orders the keys stably by

  (k >> b) & (2^(e - b) - 1)

Bits below b and at or above e do not affect the order, so keys equal in the
sorted bits keep their input order.  sort_bits_ref is numpy's stable argsort
of that masked value.

Passes.  The sort walks 8-bit steps s = b, b + 8, ... < e, the last one of
width min(8, e - s), and skips a step whose bits are the same in every key
(OR(k) ^ AND(k) has no bit inside the step).  passes_ref counts the rest.

Builders.  Each returns (keys, (b, e), premises): the premises are what the
builder claims about its keys (which wave holds 256 keys of one digit, where
the lone differing key lies, ...).  tests/test_radix_ref_host.py asserts every
one of them, so the GPU tests can rely on the shapes they name."""
import numpy as np

from summary_ref import TILE   # 4096: csrc/radix.hip kTile, keys per scatter / count tile

SCAN_ROWS = 256                # csrc/radix.hip kScanRows: tiles per block of the tile scan
WAVE = 64                      # csrc/radix.hip kWv: lanes per wave, keys per row
ROWS_PER_WAVE = 4              # csrc/radix.hip kRowsPerWave (= kSPer): rows a wave ranks in turn
WAVES = 16                     # csrc/radix.hip kSWaves: waves per scatter tile
ORAND_THREADS = 2048 * 256     # radix_sort_u64: keys_or_and_kernel runs at most 2048 blocks x 256
DIGITS = 8                     # 8-bit digits of a 64-bit key
assert WAVES * ROWS_PER_WAVE * WAVE == TILE

U64 = np.uint64


# ------------------------------------------------------------------ models
def _keys(k) -> np.ndarray:
    return np.ascontiguousarray(k, U64).reshape(-1)


def sorted_bits(k, b, e) -> np.ndarray:
    """(k >> b) & (2^(e - b) - 1): the value the sort orders by."""
    k = _keys(k)
    if e == b:
        return np.zeros_like(k)
    mask = U64((1 << (e - b)) - 1)
    return (k >> U64(b)) & mask


def sort_bits_ref(k, b, e) -> np.ndarray:
    k = _keys(k)
    return k[np.argsort(sorted_bits(k, b, e), kind="stable")]


def passes_ref(k, b, e) -> int:
    k = _keys(k)
    if k.size == 0:
        return 0
    varies = int(np.bitwise_or.reduce(k)) ^ int(np.bitwise_and.reduce(k))
    p = 0
    for s in range(b, e, 8):
        w = min(8, e - s)
        p += (varies >> s) & ((1 << w) - 1) != 0
    return p


def lane_of(i):
    """(tile, wave, row, lane) of input position i: the scatter kernel reads
    position base + w * 256 + k * 64 + lane, base = tile * TILE, as row k of
    wave w."""
    i = np.asarray(i, np.int64)
    r = i % TILE
    per_wave = ROWS_PER_WAVE * WAVE
    return i // TILE, r // per_wave, (r % per_wave) // WAVE, r % WAVE


def position_of(tile, wave, row, lane) -> int:
    return tile * TILE + wave * ROWS_PER_WAVE * WAVE + row * WAVE + lane


def digit_of(k, j) -> np.ndarray:
    return ((_keys(k) >> U64(8 * j)) & U64(0xFF)).astype(np.int64)


def with_position(digit, j) -> np.ndarray:
    """Keys with `digit` in byte j and the input position in the other bits
    (below byte j as far as it fits, the rest above it), so a rank error among
    keys of one digit shows in the output."""
    d = np.asarray(digit, np.int64)
    assert d.min() >= 0 and d.max() <= 0xFF
    pos = np.arange(d.shape[0], dtype=U64)
    low_bits = 8 * j
    low = pos & U64((1 << low_bits) - 1)
    high = pos >> U64(low_bits) if low_bits < 64 else np.zeros_like(pos)
    assert j < 7 or not high.any(), "the position does not fit below byte 7"
    k = low | (d.astype(U64) << U64(low_bits))
    if j < 7:
        k |= high << U64(low_bits + 8)
    return k


# ------------------------------------------------------------------ sizes
SIZES = (1, 2, 63, 64, 65,
         TILE - 1, TILE, TILE + 1, TILE + 64, TILE + 65, 2 * TILE - 1, 2 * TILE + 1,
         SCAN_ROWS * TILE - 1, SCAN_ROWS * TILE, SCAN_ROWS * TILE + 1,   # 256 / 257 tiles
         2 * SCAN_ROWS * TILE + 1)                                       # 513 tiles, 3 scan blocks
N_RANGES = 2 * TILE + 1        # keys of the sweep over every bit range
N_SUBSET = 3 * TILE + 17       # keys of the digit-subset and value-summary cases
N_LONE = ORAND_THREADS + 77_777
LONE_POSITIONS = (N_LONE - 1, ORAND_THREADS, 0)
BIT_RANGES = tuple((b, e) for b in range(65) for e in range(b, 65))
assert len(BIT_RANGES) == 2145


def random_keys(n, seed) -> np.ndarray:
    """Full 64-bit random keys."""
    return np.random.default_rng(seed).integers(0, 2**64, n, dtype=U64)


DUP_RANGE = (24, 43)           # 19 sorted bits: digits of 8, 8 and 3 bits
DUP_VALUES = (0, 1, 0xFF, 0x100, 0x3FFFF, 0x40000, 0x7FFFF)


def duplicate_keys(n, seed):
    """Heavy duplicates: the sorted bits DUP_RANGE take 7 values (which differ
    in each of the range's three digits); the input position is in the 24
    bits below the range and bits above it are set from the position too."""
    assert n <= 1 << DUP_RANGE[0]
    rng = np.random.default_rng(seed)
    pos = np.arange(n, dtype=U64)
    val = np.array(DUP_VALUES, U64)[rng.integers(0, len(DUP_VALUES), n)]
    above = (pos * U64(0x9E3779B1)) & U64((1 << (64 - DUP_RANGE[1])) - 1)
    k = pos | (val << U64(DUP_RANGE[0])) | (above << U64(DUP_RANGE[1]))
    return k, DUP_RANGE, {"distinct": len(DUP_VALUES)}


# ------------------------------------------------------------------ builders
LONE_BASE = 0xA5A5A5A5A5A5A5A5


def lone_variation(n, digit, pos):
    """All keys equal except key `pos`, which differs in bit `digit` of byte
    `digit`.  The base byte 0xA5 has bits 0, 2, 5, 7 set, so the odd key is
    the smallest for those digits and the largest for digits 1, 3, 4, 6."""
    k = np.full(n, LONE_BASE, U64)
    bit = 8 * digit + digit
    k[pos] ^= U64(1 << bit)
    smaller = bool((LONE_BASE >> bit) & 1)
    return k, (0, 64), {"pos": pos, "bit": bit, "lands": 0 if smaller else n - 1,
                        "or_and_blocks": min((n + 255) // 256, 2048)}


def digit_subset(mask8, n=N_SUBSET):
    """Random keys that vary in exactly the digits set in mask8.  A constant
    digit j is 0xA5 ^ j (never 0); the first three keys carry 0x00, 0x80 and
    0xFF in every chosen digit, so each takes at least 3 values."""
    assert 0 <= mask8 < 256 and n >= 3
    k = random_keys(n, 1000 + mask8)
    for j in range(DIGITS):
        byte = U64(0xFF << (8 * j))
        k &= ~byte
        if mask8 >> j & 1:
            d = np.random.default_rng(2000 + 8 * mask8 + j).integers(0, 256, n, dtype=U64)
            d[:3] = (0x00, 0x80, 0xFF)
        else:
            d = np.full(n, 0xA5 ^ j, U64)
        k |= d << U64(8 * j)
    return k, (0, 64), {"digits": [j for j in range(DIGITS) if mask8 >> j & 1]}


SKEW_DIGITS = (0, 255, 0x80)
SKEW_BYTES = (0, 3, 7)
SKEW_CORNERS = ((0, 0, 0), (WAVES - 1, ROWS_PER_WAVE - 1, WAVE - 1))   # (wave, row, lane)


def wave_skew(n_tiles, D, j, tail=0):
    """n_tiles full tiles and `tail` more keys.  Byte j of every key is D,
    except two strays per full tile at SKEW_CORNERS (D ^ 0xFF at the first
    corner, D ^ 0x01 at the last); the input position is in the other bits.
    Waves 1..14 of a full tile hold 256 keys of digit D each."""
    n = n_tiles * TILE + tail
    d = np.full(n, D, np.int64)
    strays = []
    for t in range(n_tiles):
        for (w, r, l), x in zip(SKEW_CORNERS, (D ^ 0xFF, D ^ 0x01)):
            p = position_of(t, w, r, l)
            d[p] = x
            strays.append(p)
    return with_position(d, j), (8 * j, 8 * j + 8), {"D": D, "strays": strays,
                                                     "full_wave_count": ROWS_PER_WAVE * WAVE}


ROW_PATTERNS = ("lane", "255-lane", "row", "two-by-lane", "descending", "sorted",
                "sawtooth-4096", "sawtooth-4097")
ROW_TAILS = (1, 64, 65)


def row_patterns(j=0, tail=65):
    """{name: (keys, (8j, 8j + 8), premises)}: one tile and `tail` more keys;
    byte j follows the named pattern of the input position i, which is also
    carried in the other bits."""
    n = TILE + tail
    i = np.arange(n, dtype=np.int64)
    _, _, row, lane = lane_of(i)
    digit = {
        "lane": lane,                                    # all 64 digits differ in a row
        "255-lane": 255 - lane,                          # the same, descending
        "row": row,                                      # one 64-peer group per row
        "two-by-lane": np.where(lane & 1, 0xAA, 0x55),   # two 32-peer groups
        "descending": 255 - (i // 16) % 256,             # 255 .. 0 over the tile
        "sorted": i * 256 // n,                          # non-decreasing over all keys
        "sawtooth-4096": (i % 4096) // 16,               # restarts with the tile
        "sawtooth-4097": (i % 4097) // 16 % 256,         # restarts one key into the tail
    }
    assert tuple(digit) == ROW_PATTERNS
    return {name: (with_position(d, j), (8 * j, 8 * j + 8), {"digit": np.asarray(d, np.int64)})
            for name, d in digit.items()}


# ------------------------------------------------------------------ value-summary inputs
SUMMARY_TOP = (0xBF, 0xC0)     # top key bytes of positive doubles near 1.0 and 2.0 .. 2^129


def summary_keys(P, c=N_SUBSET, seed=77):
    """c order keys of finite positive doubles (csrc/radix.h f64_key) that vary
    in exactly the low P bytes: byte j >= P is 0xA5 ^ j, the top byte 0xBF; at
    P = 8 the top byte takes both SUMMARY_TOP values.  The keys are distinct
    for P >= 2; one byte has only 256 values, so at P = 1 they repeat."""
    assert 1 <= P <= DIGITS
    rng = np.random.default_rng(seed + P)
    if P == 1:
        low = rng.integers(0, 256, c, dtype=U64)
    elif P == 2:
        low = rng.permutation(1 << 16)[:c].astype(U64)
    else:
        free = 8 * min(P, 7)
        low = np.unique(rng.integers(0, 1 << free, 2 * c, dtype=U64))
        low = rng.permutation(low)[:c]
    assert low.shape == (c,)
    k = low.copy()
    for j in range(P, 7):
        k |= U64((0xA5 ^ j) << (8 * j))
    top = np.full(c, SUMMARY_TOP[0], U64)
    if P == DIGITS:
        top[rng.random(c) < 0.5] = SUMMARY_TOP[1]
    return k | (top << U64(56))


def with_dropped(values, seed=5) -> np.ndarray:
    """The values shuffled, with a quarter as many NaNs, negatives and zeros
    (which the positive filter drops) at random positions between them."""
    rng = np.random.default_rng(seed)
    c = values.shape[0]
    d = c // 4
    hole = np.zeros(c + d, bool)
    hole[rng.choice(c + d, d, replace=False)] = True
    v = np.empty(c + d, np.float64)
    v[~hole] = values[rng.permutation(c)]
    v[hole] = np.array([np.nan, -1.5, -np.inf, 0.0, -0.0])[rng.integers(0, 5, d)]
    return v

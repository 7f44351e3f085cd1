"""Exact model of the trace-grouping paths' DECISIONS (csrc/bucket.hip and
the grouping part of csrc/group.hip), and builders of span sets that sit on
their tile, scan and bucket borders.  Plain numpy, no GPU.

The expected OUTPUT of a grouping never comes from here: it stays
oracle.spec.group_by_trace (a stable argsort of mix64(trace_hash)) and
oracle.native.edge_aggregate on the oracle-grouped spans, which know nothing
of tiles or buckets.  What this file restates is what the kernels do on the
way: the bucket geometry, the two re-split rules, which kernel a bucket of a
given size takes, when a set leaves the bucket path for the LSD path and how
many passes that takes — so a test can say which path a set MUST take
(Context.group_info) and what the ANOMOD_BUCKET_DEBUG line must print, and a
silent fallback fails instead of passing every "same grouping" assertion.

mix64 is a bijection, so unmix64 gives every trace a chosen order key
k = mix64(trace_hash): a plan puts every trace into a chosen bucket.

tests/test_group_ref_host.py checks, without a GPU, that every case of CASES
hits the border it is named after (layout() counts straight from the keys);
tests/test_gpu_group_borders.py runs the cases."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle.spec import mix64

# ---- the constants the borders depend on (test_constants_restate_the_kernel_source)
kBTile = 2048        # records per level-A tile
kPTile = 16384       # pairs per level-B tile
kDMax = 11           # digit bits per scatter level
kScanRows = 256      # tiles per block of the level-A tile scan
kScanB = 16          # loads in flight per serial scan step
kSubBits = 9         # per-bucket split before the key compare
SMALL_CAP = 2048     # kSmallW * kSmallPer: the per-bucket sorting kernel
BIG_CAP = 8192       # kBigW * kBigPer: the large sorting kernel
kHugeKeys = 2048     # distinct keys the huge-bucket walk holds
kDChunk = 4096       # entries per partial sum of the trace-count scan
JOIN_CAP = 2048      # kJoinW * kJoinPer
JOIN_BIG_UNPACKED = 4096   # kJoinBigW * join_big_per(false)
JOIN_BIG_PACKED = 8192     # kJoinBigW * join_big_per(true)
PACK_FROM_T = 12     # the join packs the service into the key word from T >= 12
T_MAX = 22           # 2 * kDMax
DEFAULT_AVG = 1400   # ANOMOD_BUCKET_AVG's default
# LSD path (group.hip)
kSTile = 4096        # records per radix tile
kTTile = 16384       # spans per tile of the bucket-list / trace_ptr scans
kFixCap = 1024       # records of a mixed bucket one wave sorts
kTScanRows = 256     # tiles per block of the tile-count scan
kMaxPasses = 8

# the constexpr lines of the two files these literals restate: (file, name, value)
KERNEL_CONSTANTS = (
    ("bucket.hip", "kBThreads", 1024), ("bucket.hip", "kBPer", 2), ("bucket.hip", "kPPer", 16),
    ("bucket.hip", "kDMax", kDMax), ("bucket.hip", "kScanRows", kScanRows),
    ("bucket.hip", "kScanB", kScanB), ("bucket.hip", "kSubBits", kSubBits),
    ("bucket.hip", "kSmallW", 512), ("bucket.hip", "kSmallPer", 4),
    ("bucket.hip", "kBigW", 1024), ("bucket.hip", "kBigPer", 8),
    ("bucket.hip", "kDChunk", kDChunk), ("bucket.hip", "kHugeKeys", kHugeKeys),
    ("bucket.hip", "kHugeSlots", 4096), ("bucket.hip", "kJoinW", 512),
    ("bucket.hip", "kJoinPer", 4), ("bucket.hip", "kJoinBigW", 1024),
    ("group.hip", "kSThreads", 1024), ("group.hip", "kSPer", 4), ("group.hip", "kTThreads", 1024),
    ("group.hip", "kTPer", 16), ("group.hip", "kFixCap", kFixCap),
    ("group.hip", "kTScanRows", kTScanRows), ("group.hip", "kMaxPasses", kMaxPasses),
)

ONES = (1 << 64) - 1


def unmix64(k) -> np.ndarray:
    """Inverse of oracle.spec.mix64 (hashes with chosen mixed keys)."""
    M = 2**64

    def unxorshift(y, s):
        x = y.copy()
        for _ in range(64 // s + 1):
            x = y ^ (x >> np.uint64(s))
        return x

    z = unxorshift(np.array(k, np.uint64, copy=True).reshape(-1), 31)
    z = z * np.uint64(pow(0x94D049BB133111EB, -1, M))
    z = unxorshift(z, 27)
    z = z * np.uint64(pow(0xBF58476D1CE4E5B9, -1, M))
    return unxorshift(z, 30)


# ---------------------------------------------------------------- geometry
@dataclass(frozen=True)
class Geom:
    T: int
    DA: int
    DB: int
    tilesA: int

    @property
    def levels(self) -> int:
        return 2 if self.DB else 1


def bucket_geom(n: int, avg: int | None = None) -> Geom:
    """bucket_geom() of bucket.hip: the mean bucket size in (avg/2, avg]."""
    avg = min(max(DEFAULT_AVG if avg is None else int(avg), 64), 2048)
    T = 1
    while T < T_MAX and (n >> T) > avg:
        T += 1
    if T <= kDMax:
        DA, DB = T, 0
    else:
        DA = max(T - kDMax, min((T + 1) // 2, 9))
        DB = T - DA
    return Geom(T, DA, DB, (n + kBTile - 1) // kBTile if n else 1)


def resplit(g: Geom) -> Geom:
    """Both re-split rules end in the same geometry: level B takes kDMax bits
    (one level whose largest bucket exceeds BIG_CAP escalates to two; two
    levels split finer, workspace permitting)."""
    return Geom(g.DA + kDMax, g.DA, kDMax, g.tilesA)


# ------------------------------------------------------------------ layout
@dataclass
class Layout:
    T: int
    DA: int
    sizes: np.ndarray        # spans per bucket at T bits
    sizesA: np.ndarray       # spans per level-A bucket (DA bits)
    tilesB: np.ndarray       # level-B tiles per level-A bucket
    keys: np.ndarray         # distinct keys (traces) per bucket at T bits
    max_bucket: int
    n_over_small: int        # buckets over SMALL_CAP spans


def span_keys(flat) -> np.ndarray:
    return mix64(flat.trace_hash)


def layout(flat, T: int, DA: int) -> Layout:
    """Counted directly from mix64(flat.trace_hash)."""
    k = span_keys(flat)
    sizes = np.bincount((k >> np.uint64(64 - T)).astype(np.int64), minlength=1 << T)
    sizesA = np.bincount((k >> np.uint64(64 - DA)).astype(np.int64), minlength=1 << DA)
    uk = np.unique(k)
    keys = np.bincount((uk >> np.uint64(64 - T)).astype(np.int64), minlength=1 << T)
    return Layout(T, DA, sizes, sizesA, (sizesA + kPTile - 1) // kPTile, keys,
                  int(sizes.max()) if k.size else 0, int((sizes > SMALL_CAP).sum()))


def lsd_passes(k: np.ndarray) -> int:
    """Radix passes of the LSD path (group_run of group.hip): the fewest P
    with 2^(8P) >= n, then one more while some bucket of equal top 8P key bits
    holds several keys and more than kFixCap records.  (The other retry, an
    overflow of the key-change list of n/8 + 65536 entries, needs far more
    mixed records than any set here holds.)"""
    n = int(k.shape[0])
    P = 1
    while P < kMaxPasses and (1 << (8 * P)) < n:
        P += 1
    if n == 0:
        return P
    uk, cnt = np.unique(k, return_counts=True)
    while P < kMaxPasses:
        top = uk >> np.uint64(64 - 8 * P)
        _, inv = np.unique(top, return_inverse=True)
        nkeys = np.bincount(inv)
        recs = np.bincount(inv, weights=cnt).astype(np.int64)
        if not ((nkeys >= 2) & (recs > kFixCap)).any():
            break
        P += 1
    return P


def _final_geom(k: np.ndarray, avg):
    """The geometry the bucket path ends with, the largest bucket there, and
    whether the two-level re-split (which also needs workspace for 2^(DA+11)
    buckets, unknown here) was what produced it."""
    g = bucket_geom(int(k.shape[0]), avg)
    mx = int(np.bincount((k >> np.uint64(64 - g.T)).astype(np.int64)).max())
    two_level_resplit = False
    if mx > BIG_CAP and g.DB < kDMax:
        two_level_resplit = g.DB > 0
        g = resplit(g)
    return g, two_level_resplit


def predict_group(flat, avg=None, force_lsd=False) -> dict:
    """What anomod_spans_group does with the set: path / levels / bits of
    Context.group_info, and the numbers of the last ANOMOD_BUCKET_DEBUG line
    ("debug": T, DA, DB, largest bucket, buckets over 2048, buckets too big;
    None where none is printed)."""
    k = span_keys(flat)
    if k.size and not force_lsd:
        g, unsure = _final_geom(k, avg)
        b = (k >> np.uint64(64 - g.T)).astype(np.int64)
        sizes = np.bincount(b, minlength=1 << g.T)
        uk = np.unique(k)
        nkeys = np.bincount((uk >> np.uint64(64 - g.T)).astype(np.int64), minlength=1 << g.T)
        huge = sizes > BIG_CAP
        bad = huge & (nkeys > kHugeKeys)
        if (k == np.uint64(ONES)).any():  # the huge table's empty mark
            bad[-1] |= huge[-1]
        debug = (g.T, g.DA, g.DB, int(sizes.max()), int((sizes > SMALL_CAP).sum()), int(bad.sum()))
        if not bad.any():
            return {"path": "bucket", "levels": g.levels, "bits": g.T, "debug": debug,
                    "resplit": unsure}
    else:
        debug, unsure = None, False
    P = lsd_passes(k)
    return {"path": "lsd", "levels": P, "bits": 8 * P, "debug": debug, "resplit": unsure}


def predict_join(flat, avg=None, pack=True, force_lsd=False, fused=True) -> dict:
    """What anomod_edge_aggregate_ungrouped does with the set: the per-bucket
    hash join while every bucket fits its big kernel (8192 spans with the
    packed key word, from T >= 12; 4096 without), else the unfused path, whose
    grouping is predict_group's."""
    k = span_keys(flat)
    if k.size and fused and not force_lsd:
        g, unsure = _final_geom(k, avg)
        mx = int(np.bincount((k >> np.uint64(64 - g.T)).astype(np.int64)).max())
        cap = JOIN_BIG_PACKED if (g.T >= PACK_FROM_T and pack) else JOIN_BIG_UNPACKED
        if mx <= cap:
            return {"path": "join", "levels": g.levels, "bits": g.T, "max_bucket": mx,
                    "resplit": unsure}
    return predict_group(flat, avg, force_lsd)


# ------------------------------------------------------------------- plans
def _distinct(rng, w: int, m: int) -> np.ndarray:
    """m distinct values of w bits, none of them 0 or all ones (the two
    extreme keys stay free for the policies that name them)."""
    if w <= 24:
        return (rng.choice((1 << w) - 2, m, replace=False) + 1).astype(np.uint64)
    while True:
        v = rng.integers(1, (1 << w) - 1, m, dtype=np.uint64)
        if np.unique(v).shape[0] == m:
            return v


def plan_keys(rng, T: int, bucket: int, m: int, policy) -> np.ndarray:
    """Order keys of m traces of one bucket (bucket index at T bits):
    k = bucket << (64 - T) | r with r distinct, chosen by the policy:
      "random"               r uniform
      "mixsub"               the traces share the next kSubBits bits below T
                             and differ in the 11 bits below those (bits every
                             pair carries): one mixed sub-bucket
      ("share", nb, fill)    the traces share their top nb key bits, the bits
                             between T and nb random / all "ones" / "zeros"
                             (nb = T + 32: equal pair keys, the exact re-rank;
                             nb = 40: one bucket however fine the split)
      "zero" / "ones"        the one trace with k = 0 / k = 2^64 - 1"""
    low = 64 - T
    top = bucket << low
    if policy == "random":
        r = _distinct(rng, low, m).astype(object)
    elif policy == "mixsub":
        assert m <= 2048
        s9 = int(rng.integers(0, 1 << kSubBits))
        w = low - kSubBits - 11
        d11 = rng.choice(2048, m, replace=False).astype(object)
        r = (s9 << (low - kSubBits)) | (d11 << w) | rng.integers(0, 1 << w, m, dtype=np.uint64).astype(object)
    elif policy == "zero":
        assert bucket == 0 and m == 1
        r = np.array([0], object)
    elif policy == "ones":
        assert bucket == (1 << T) - 1 and m == 1
        r = np.array([(1 << low) - 1], object)
    else:
        _, nb, fill = policy
        sw, w = nb - T, 64 - nb
        shared = {"ones": (1 << sw) - 1, "zeros": 0}.get(fill)
        if shared is None:
            shared = int(rng.integers(0, 1 << sw)) if sw else 0
        r = (shared << w) | _distinct(rng, w, m).astype(object)
    return np.array([top | int(x) for x in r], np.uint64)


def _filler_lens(rng, n: int, max_len: int) -> np.ndarray:
    """Trace lengths in [1, max_len] summing to exactly n."""
    if n == 0:
        return np.zeros(0, np.int64)
    lens = rng.integers(1, max_len + 1, n)
    cut = int(np.searchsorted(np.cumsum(lens), n)) + 1
    lens = lens[:cut]
    lens[-1] -= int(lens.sum()) - n
    return lens.astype(np.int64)


def compose(rng, total: int, parts: int) -> list[int]:
    """`parts` positive trace lengths summing to exactly `total`."""
    cuts = np.sort(rng.choice(total - 1, parts - 1, replace=False) + 1) if parts > 1 else []
    return np.diff(np.r_[0, cuts, total]).astype(int).tolist()


def plan_set(rng, S: int, T: int, plan, n: int | None = None, filler=(), mode="random", dup=0.02,
             edit=None):
    """The flat interleaved SpanSet of a plan: a list of (bucket index at T
    bits, [trace lengths], policy), see plan_keys.  Filler groups
    {"buckets": indices at T bits (None: every bucket no plan entry names),
    "n": spans (None: what is missing to `n`), "max_len": L} add short traces
    with random keys to the named buckets only, dealt round the buckets in
    turn, so a planned bucket holds exactly what the plan says.  Spans come
    from _random_spanset (duplicate ids, orphans), arrival order from
    _interleave; edit(sp, lens) may change the grouped spans before they are
    keyed and interleaved."""
    from test_gpu_edge import _random_spanset
    from test_gpu_group import _interleave

    keys, lens = [], []
    for bucket, tl, policy in plan:
        keys.append(plan_keys(rng, T, bucket, len(tl), policy))
        lens.append(np.asarray(tl, np.int64))
    planned = {b for b, _, _ in plan}
    have = int(sum(x.sum() for x in lens))
    for f in filler:
        fn = f["n"]
        if fn is None:
            fn = n - have - sum(x["n"] or 0 for x in filler)
        fl = _filler_lens(rng, fn, f["max_len"])
        buckets = f["buckets"]
        if buckets is None:
            buckets = [b for b in range(1 << T) if b not in planned]
        buckets = rng.permutation(np.asarray(list(buckets), np.int64))
        fb = buckets[np.arange(fl.shape[0]) % buckets.shape[0]].astype(np.uint64)
        low = 64 - T
        keys.append((fb << np.uint64(low)) | _distinct(rng, low, fl.shape[0]))
        lens.append(fl)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    lens = np.concatenate(lens) if lens else np.zeros(0, np.int64)
    if np.unique(keys).shape[0] != keys.shape[0]:
        raise ValueError("two traces of the plan drew one key")
    if n is not None and int(lens.sum()) != n:
        raise ValueError(f"the plan holds {int(lens.sum())} spans, not {n}")
    sp = _random_spanset(rng, S, 0, 0, dup=dup, lens=lens)
    if edit is not None:
        edit(sp, lens)
    sp.trace_hash = np.repeat(unmix64(keys), lens).astype(np.uint64)
    return _interleave(sp, rng, mode)


# ------------------------------------------------------------------- cases
@dataclass
class Case:
    """One span set on a named border.  facts: what layout() must show, as
    (kind, *args) tuples (check_fact); group / join: the literal path, levels
    and bits the test file expects, which the host test holds to the model."""
    name: str
    build: object
    S: int = 12
    avg: int | None = None
    lsd: bool = False
    facts: list = field(default_factory=list)
    group: tuple | None = None       # (path, levels, bits); bits None: re-split, not asserted
    join: tuple | None = None        # with the default ANOMOD_JOIN_PACK

    def env(self) -> dict:
        e = {}
        if self.avg is not None:
            e["ANOMOD_BUCKET_AVG"] = str(self.avg)
        if self.lsd:
            e["ANOMOD_GROUP_PATH"] = "lsd"
        return e


CASES: dict[str, Case] = {}


def _case(name, build, **kw):
    CASES[name] = Case(name, build, **kw)


@functools.lru_cache(maxsize=3)
def built(name: str):
    """(flat set, oracle grouping) of a case, the last few kept."""
    from test_gpu_group import _oracle_grouped

    flat = CASES[name].build()
    return flat, _oracle_grouped(flat)


def check_fact(flat, fact) -> None:
    """Assert one fact of a case from layout() / the keys alone."""
    kind, *a = fact
    k = span_keys(flat)
    if kind == "n":
        assert flat.n_spans == a[0]
    elif kind == "geom":  # (avg, T, DA, DB, tilesA)
        g = bucket_geom(flat.n_spans, a[0])
        assert (g.T, g.DA, g.DB, g.tilesA) == tuple(a[1:]), g
    elif kind == "size":  # (T, bucket, spans, distinct keys or None)
        lay = layout(flat, a[0], min(a[0], kDMax))
        assert lay.sizes[a[1]] == a[2], (fact, int(lay.sizes[a[1]]))
        if a[3] is not None:
            assert lay.keys[a[1]] == a[3], (fact, int(lay.keys[a[1]]))
    elif kind == "sizeA":  # (DA, level-A bucket, spans, level-B tiles)
        lay = layout(flat, a[0], a[0])
        assert lay.sizesA[a[1]] == a[2] and lay.tilesB[a[1]] == a[3], (fact, int(lay.sizesA[a[1]]))
    elif kind == "max":  # (T, largest bucket, buckets over 2048)
        lay = layout(flat, a[0], min(a[0], kDMax))
        assert (lay.max_bucket, lay.n_over_small) == (a[1], a[2]), (fact, lay.max_bucket,
                                                                     lay.n_over_small)
    elif kind == "max_at_most":  # (T, bound)
        assert layout(flat, a[0], min(a[0], kDMax)).max_bucket <= a[1]
    elif kind == "empty_run":  # (T, lo, hi): no span in buckets [lo, hi)
        lay = layout(flat, a[0], min(a[0], kDMax))
        assert a[2] - a[1] >= 300 and not lay.sizes[a[1]:a[2]].any()
    elif kind == "nonempty":  # (T, buckets)
        lay = layout(flat, a[0], min(a[0], kDMax))
        assert all(lay.sizes[b] > 0 for b in a[1])
    elif kind == "has_key":
        assert (k == np.uint64(a[0])).any()
    elif kind == "shared":  # (T, bucket, nbits, traces): that many keys share their top nbits
        uk = np.unique(k[(k >> np.uint64(64 - a[0])) == np.uint64(a[1])])
        _, c = np.unique(uk >> np.uint64(64 - a[2]), return_counts=True)
        assert c.max() == a[3], (fact, int(c.max()))
    elif kind == "differ":  # (T, bucket, nbits): the keys sharing most differ inside nbits
        uk = np.unique(k[(k >> np.uint64(64 - a[0])) == np.uint64(a[1])])
        assert np.unique(uk >> np.uint64(64 - a[2])).shape[0] == uk.shape[0]
    elif kind == "lsd_mixed":  # (P, records): the largest several-key bucket of equal top 8P bits
        uk, cnt = np.unique(k, return_counts=True)
        _, inv = np.unique(uk >> np.uint64(64 - 8 * a[0]), return_inverse=True)
        nkeys, recs = np.bincount(inv), np.bincount(inv, weights=cnt).astype(np.int64)
        assert int(recs[nkeys >= 2].max()) == a[1], (fact, int(recs[nkeys >= 2].max()))
    elif kind == "dups_across_tiles":  # (DA, level-A bucket, at least)
        assert _dups_across_tiles(flat, a[0], a[1]) >= a[2]
    else:
        raise ValueError(kind)


def _dups_across_tiles(flat, DA: int, a: int) -> int:
    """Traces of level-A bucket a whose first two spans with one id lie in
    different level-B tiles (tile = rank in arrival order // kPTile: level A
    is stable)."""
    k = span_keys(flat)
    idx = np.flatnonzero((k >> np.uint64(64 - DA)) == np.uint64(a))
    tile = np.arange(idx.shape[0]) // kPTile
    order = np.lexsort((np.arange(idx.shape[0]), flat.span_id[idx], k[idx]))
    ks, ids, ts = k[idx][order], flat.span_id[idx][order], tile[order]
    same = (ks[1:] == ks[:-1]) & (ids[1:] == ids[:-1])
    return int(np.unique(ks[1:][same & (ts[1:] != ts[:-1])]).shape[0])


# A. level-A tiles and wave rows: one level, every n of the list
A_SIZES = {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 127: 1, 128: 1, 129: 1, 2047: 1, 2048: 1, 2049: 2,
           4097: 3, 7 * 2048 + 1: 8, 8 * 2048: 8, 9 * 2048 - 1: 9, 17 * 2048 + 5: 18}


def _random_case(n, mode, seed, max_len=8, S=12):
    def build():
        rng = np.random.default_rng(seed)
        return plan_set(rng, S, 1, [], n=n, filler=[{"buckets": None, "n": None,
                                                     "max_len": max_len}], mode=mode)
    return build


for _n, _tiles in A_SIZES.items():
    for _avg in (None, 64):
        for _mode in ("time", "reverse"):
            _g = bucket_geom(_n, _avg)
            _case(f"A-{_n}-{_avg}-{_mode}", _random_case(_n, _mode, _n * 3 + (_avg or 0)),
                  avg=_avg, facts=[("n", _n), ("geom", _avg, _g.T, _g.T, 0, _tiles)])

# B. scan blocks: kScanRows tiles per block of the level-A scan
for _n, _tiles in ((524287, 256), (524288, 256), (524289, 257)):
    for _avg, _t in ((None, (9, 9, 0)), (64, (13, 7, 6))):
        def _build(n=_n, T=_t[0]):
            rng = np.random.default_rng(n)
            return plan_set(rng, 12, T, [], n=n, mode="time",
                            filler=[{"buckets": None, "n": None, "max_len": 8}])
        _case(f"B-{_n}-{_avg}", _build, avg=_avg,
              facts=[("n", _n), ("geom", _avg, *_t, _tiles), ("max_at_most", _t[0], SMALL_CAP)],
              group=("bucket", 2 if _t[2] else 1, _t[0]), join=("join", 2 if _t[2] else 1, _t[0]))


def _build_b17():
    rng = np.random.default_rng(17)
    return plan_set(rng, 12, 13, [], n=16 * 524288 + 1, mode="time", dup=0.0,
                    filler=[{"buckets": None, "n": None, "max_len": 6}])


_case("B-17-blocks", _build_b17,
      facts=[("n", 16 * 524288 + 1), ("geom", None, 13, 7, 6, 4097), ("max_at_most", 13, SMALL_CAP)],
      group=("bucket", 2, 13), join=("join", 2, 13))


# C. two digits per thread (nd = 2048): n = 100 000 at avg = 64, T = DA = 11
def _build_c(ends, empty):
    def build():
        rng = np.random.default_rng(len(ends))
        plan = [(b, [5, 7, 3], "random") for b in ends]
        skip = set(ends)
        for lo, hi in empty:
            skip |= set(range(lo, hi))
        return plan_set(rng, 12, 11, plan, n=100000, mode="time",
                        filler=[{"buckets": [b for b in range(2048) if b not in skip], "n": None,
                                 "max_len": 8}])
    return build


_C1 = (0, 1, 1023, 1024, 2046, 2047)
_case("C-ends-and-pairing", _build_c(_C1, ((200, 520), (1300, 1650))), avg=64,
      facts=[("n", 100000), ("geom", 64, 11, 11, 0, 49), ("nonempty", 11, _C1),
             ("empty_run", 11, 200, 520), ("empty_run", 11, 1300, 1650)],
      group=("bucket", 1, 11), join=("join", 1, 11))
_C2 = (0, 1, 2046, 2047)
_case("C-empty-across-pairing", _build_c(_C2, ((850, 1200),)), avg=64,
      facts=[("n", 100000), ("geom", 64, 11, 11, 0, 49), ("nonempty", 11, _C2),
             ("empty_run", 11, 850, 1200)],
      group=("bucket", 1, 11), join=("join", 1, 11))


# D. level-B tiles
def _build_d12(sizes_a):
    """T = 12 (DA = DB = 6): level-A buckets of exactly the given sizes."""
    def build():
        rng = np.random.default_rng(sum(sizes_a))
        fill = [{"buckets": range(a << 6, (a + 1) << 6), "n": m, "max_len": 8}
                for a, m in sizes_a.items() if m]
        rest = [b for a in range(64) if a not in sizes_a for b in range(a << 6, (a + 1) << 6)]
        fill.append({"buckets": rest, "n": None, "max_len": 8})
        return plan_set(rng, 12, 12, [], n=140000, filler=fill, mode="time")
    return build


for _name, _sz in (("first-empty", {0: 0, 1: 1, 2: 16383, 3: 16384, 4: 16385}),
                   ("last-empty", {63: 0, 62: 1, 61: 16385, 60: 16384, 59: 16383})):
    _case(f"D-12-{_name}", _build_d12(_sz), avg=64,
          facts=[("n", 140000), ("geom", 64, 12, 6, 6, 69), ("max_at_most", 12, SMALL_CAP)] +
                [("sizeA", 6, a, m, (m + kPTile - 1) // kPTile) for a, m in _sz.items()],
          group=("bucket", 2, 12), join=("join", 2, 12))

D17_A = 77  # the level-A bucket (DA = 7) of 17 level-B tiles


def _dup_edit(sp, lens):
    """Every 12-span trace: the id of span 1 again at span 6, spans 7.. refer
    to it; the copies carry services 3 and 9 (the first match is service 3)."""
    ptr = sp.trace_ptr[:-1].astype(np.int64)[lens == 12]
    sp.span_id[ptr + 6] = sp.span_id[ptr + 1]
    for j in range(7, 12):
        sp.parent_span_id[ptr + j] = sp.span_id[ptr + 1]
    sp.svc[ptr + 1] = 3
    sp.svc[ptr + 6] = 9


def _build_d17(dups):
    """T = 13 (DA = 7, DB = 6): one level-A bucket of 16 * 16384 + 1 spans,
    dealt over its 64 final buckets (4096 or 4097 spans each)."""
    def build():
        rng = np.random.default_rng(1700 + dups)
        big = 16 * kPTile + 1
        inside = list(range(D17_A << 6, (D17_A + 1) << 6))
        rest = [b for b in range(1 << 13) if b >> 6 != D17_A]
        if not dups:
            fill = [{"buckets": inside, "n": big, "max_len": 8}]
            plan = []
        else:  # 12-span traces with a repeated id, plus one span to make the count
            m = big // 12
            plan = [(b, [12] * len(range(i, m, 64)), "random") for i, b in enumerate(inside)]
            plan.append((inside[0], [big - 12 * m], "random"))
            fill = []
        fill.append({"buckets": rest, "n": None, "max_len": 8})
        return plan_set(rng, 12, 13, plan, n=300000, filler=fill, mode="random",
                        dup=0.0 if dups else 0.02, edit=_dup_edit if dups else None)
    return build


for _name, _d in (("D-13-17-tiles", 0), ("D-13-17-tiles-dups", 1)):
    _case(_name, _build_d17(_d), avg=64,
          facts=[("n", 300000), ("geom", 64, 13, 7, 6, 147), ("sizeA", 7, D17_A, 16 * kPTile + 1, 17),
                 ("max_at_most", 13, BIG_CAP)] + ([("dups_across_tiles", 7, D17_A, 15000)] if _d else []),
          group=("bucket", 2, 13), join=("join", 2, 13))


# E / F at the default mean: n = 65536 spans, T = 6 (64 buckets of ~1000 spans)
def _build_t6(plan_of, S=12, seed=6):
    def build():
        rng = np.random.default_rng(seed)
        return plan_set(rng, S, 6, plan_of(rng), n=65536, mode="random",
                        filler=[{"buckets": None, "n": None, "max_len": 8}])
    return build


_T6 = ("geom", None, 6, 6, 0, 32)
_case("E-caps", _build_t6(lambda rng: [(3, compose(rng, 2047, 5), "random"),
                                       (4, compose(rng, 2048, 5), "random"),
                                       (5, compose(rng, 2049, 5), "random"),
                                       (10, compose(rng, 8191, 7), "random"),
                                       (11, compose(rng, 8192, 7), "random")]),
      facts=[("n", 65536), _T6, ("size", 6, 3, 2047, 5), ("size", 6, 4, 2048, 5),
             ("size", 6, 5, 2049, 5), ("size", 6, 10, 8191, 7), ("size", 6, 11, 8192, 7),
             ("max", 6, 8192, 3)],
      group=("bucket", 1, 6), join=("bucket", 1, 6))
_case("E-huge-3-traces", _build_t6(lambda rng: [(20, [3000, 3000, 2193], ("share", 40, "rand"))]),
      facts=[("n", 65536), _T6, ("size", 6, 20, 8193, 3), ("shared", 6, 20, 40, 3),
             ("max", 6, 8193, 1), ("max", 17, 8193, 1)],
      group=("bucket", 2, 17), join=("bucket", 2, 17))
_case("E-huge-1-trace", _build_t6(lambda rng: [(20, [8193], "random")]),
      facts=[("n", 65536), _T6, ("size", 6, 20, 8193, 1), ("max", 6, 8193, 1),
             ("max", 17, 8193, 1)],
      group=("bucket", 2, 17), join=("bucket", 2, 17))
_case("E-huge-2048-keys", _build_t6(lambda rng: [(20, [4] * 2047 + [5], ("share", 40, "rand"))]),
      facts=[("n", 65536), _T6, ("size", 6, 20, 8193, 2048), ("shared", 6, 20, 40, 2048),
             ("max", 17, 8193, 1)],
      group=("bucket", 2, 17), join=("bucket", 2, 17))
_case("E-huge-2049-keys", _build_t6(lambda rng: [(20, [4] * 2049, ("share", 40, "rand"))]),
      facts=[("n", 65536), _T6, ("size", 6, 20, 8196, 2049), ("shared", 6, 20, 40, 2049),
             ("max", 17, 8196, 1)],
      group=("lsd", 6, 48), join=("lsd", 6, 48))
_case("E-ones-in-huge", _build_t6(lambda rng: [(63, [4100, 4000], ("share", 40, "ones")),
                                               (63, [93], "ones")]),
      facts=[("n", 65536), _T6, ("size", 6, 63, 8193, 3), ("has_key", ONES),
             ("size", 17, (1 << 17) - 1, 8193, 3)],
      group=("lsd", 6, 48), join=("lsd", 6, 48))
_case("E-ones-and-zero-ordinary",
      _build_t6(lambda rng: [(63, [20, 30], "random"), (63, [15], "ones"), (0, [25], "zero"),
                             (0, [10, 12], "random")]),
      facts=[("n", 65536), _T6, ("size", 6, 63, 65, 3), ("size", 6, 0, 47, 3), ("has_key", ONES),
             ("has_key", 0), ("max_at_most", 6, SMALL_CAP)],
      group=("bucket", 1, 6), join=("join", 1, 6))
_case("E-mixed",
      _build_t6(lambda rng: [(7, compose(rng, 2048, 40), "mixsub"),
                             (8, compose(rng, 2048, 40), ("share", 38, "rand")),
                             (30, compose(rng, 6000, 60), "mixsub"),
                             (31, compose(rng, 6000, 60), ("share", 38, "rand"))]),
      facts=[("n", 65536), _T6, ("size", 6, 7, 2048, 40), ("size", 6, 8, 2048, 40),
             ("size", 6, 30, 6000, 60), ("size", 6, 31, 6000, 60),
             ("shared", 6, 7, 6 + kSubBits, 40), ("differ", 6, 7, 6 + kSubBits + 11),
             ("shared", 6, 30, 6 + kSubBits, 60), ("differ", 6, 30, 6 + kSubBits + 11),
             ("shared", 6, 8, 38, 40), ("shared", 6, 31, 38, 60), ("max", 6, 6000, 2)],
      group=("bucket", 1, 6), join=("bucket", 1, 6))

# F. join caps; unpacked (T < 12)
_case("F-unpacked-4096",
      _build_t6(lambda rng: [(3, compose(rng, 2048, 5), "random"), (4, compose(rng, 2049, 5), "random"),
                             (9, compose(rng, 4096, 6), "random")], seed=61),
      facts=[("n", 65536), _T6, ("size", 6, 3, 2048, 5), ("size", 6, 4, 2049, 5),
             ("size", 6, 9, 4096, 6), ("max", 6, 4096, 2)],
      group=("bucket", 1, 6), join=("join", 1, 6))
_case("F-unpacked-4097",
      _build_t6(lambda rng: [(3, compose(rng, 2048, 5), "random"), (4, compose(rng, 2049, 5), "random"),
                             (9, compose(rng, 4097, 6), "random")], seed=62),
      facts=[("n", 65536), _T6, ("size", 6, 9, 4097, 6), ("max", 6, 4097, 2)],
      group=("bucket", 1, 6), join=("bucket", 1, 6))


# packed (T >= 12): n = 140 000 at avg = 64, T = 12
def _build_t12(plan_of, S, seed):
    def build():
        rng = np.random.default_rng(seed)
        return plan_set(rng, S, 12, plan_of(rng), n=140000, mode="random",
                        filler=[{"buckets": None, "n": None, "max_len": 8}])
    return build


_T12 = ("geom", 64, 12, 6, 6, 69)
for _S in (12, 46):
    _case(f"F-packed-8192-S{_S}",
          _build_t12(lambda rng: [(100, compose(rng, 2048, 5), "random"),
                                  (2000, compose(rng, 2049, 5), "random"),
                                  (4095, compose(rng, 8192, 9), "random")], _S, 120 + _S),
          S=_S, avg=64,
          facts=[("n", 140000), _T12, ("size", 12, 100, 2048, 5), ("size", 12, 2000, 2049, 5),
                 ("size", 12, 4095, 8192, 9), ("max", 12, 8192, 2)],
          group=("bucket", 2, 12), join=("join", 2, 12))
# 8193 spans sharing 40 key bits: the two-level re-split (DB = 11) cannot
# split them, the packed join's 8192 cannot hold them -> the unfused path
_case("F-packed-8193",
      _build_t12(lambda rng: [(100, compose(rng, 2048, 5), "random"),
                              (4095, compose(rng, 8193, 9), ("share", 40, "rand"))], 12, 121),
      avg=64,
      facts=[("n", 140000), _T12, ("size", 12, 4095, 8193, 9), ("shared", 12, 4095, 40, 9),
             ("max", 12, 8193, 1), ("max", 17, 8193, 1)],
      group=("bucket", 2, None), join=("bucket", 2, None))

# G. the LSD path (ANOMOD_GROUP_PATH=lsd): its 4096-record radix tiles and
# 16384-span scan tiles, and the kFixCap mixed-bucket border
for _n in (4095, 4096, 4097, 16383, 16384, 16385):
    _case(f"G-{_n}", _random_case(_n, "time", 7000 + _n), lsd=True,
          facts=[("n", _n)], group=("lsd", 2, 16), join=("lsd", 2, 16))


def _build_g_mixed(records):
    def build():
        rng = np.random.default_rng(records)
        return plan_set(rng, 12, 16, [(0x5A5A, compose(rng, records, 6), "random")], n=30000,
                        mode="random", filler=[{"buckets": None, "n": None, "max_len": 8}])
    return build


_case("G-mixed-1024", _build_g_mixed(1024), lsd=True,
      facts=[("n", 30000), ("size", 16, 0x5A5A, 1024, 6), ("lsd_mixed", 2, 1024)],
      group=("lsd", 2, 16), join=("lsd", 2, 16))
_case("G-mixed-1025", _build_g_mixed(1025), lsd=True,
      facts=[("n", 30000), ("size", 16, 0x5A5A, 1025, 6), ("lsd_mixed", 2, 1025),
             ("differ", 16, 0x5A5A, 24)],
      group=("lsd", 3, 24), join=("lsd", 3, 24))

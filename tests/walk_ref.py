"""Model of the shared span walk (a plain helper, not a conftest): the
decisions of csrc/walk.h and csrc/chunk.h restated in plain Python, and the
builders of the span sets that put a border of the walk under every one of the
five passes that resolve parents through it (self time, critical path, trace
shapes, trace spectrum, error origins).  Nothing here computes what a pass
computes: the expected results are the passes' own reference helpers and the C
oracle (refs() below only calls them).

The model
  tail_start / tail_chunks   where a trace runs.  walk_traces gives the first
        nt - nt // DYN traces to its waves in equal static shares (thousands
        of waves: in a small set every such trace is a run, and so a chunk, of
        its own) and hands out the last nt // DYN in segments of DYN_SEG
        consecutive traces; only a run of several traces is packed into chunks
        (make_chunk: the most leading traces, up to CHUNK_TRACES, that hold <=
        STAGE spans together; a longer trace is a chunk of its own, k = 0).
        The packing loop is trace_struct_ref's, started at this driver's tail.
  scan_of       the scan pick_walk_scan picks (forward, bidir, split).
  scan_steps / scan_hit   for span i of the trace [a, b) whose parent sits at
        q: the step, the side and the slot within the block at which
        find_first / find_parent_bidir<6,4> / find_parent_split<12,4> finds
        it, the valid ids of the forward block at that step and the clamped
        backward blocks passed on the way — closed-form arithmetic
        (test_walk_ref_host.py holds it to a literal emulation of the loops).
  big_slot / big_windows / big_blocks   the long-trace lookup big_parents:
        windows of BIG_WIN ids in a table of BIG_SLOTS slots (multiply-shift
        hash, linear probing), blocks of BIG_BLOCK spans.

Placement.  in_tail() puts 3 m one-span root traces in front of a shape of m
traces: the set then has 4 m traces, the shape is exactly the dynamic tail and
is walked as runs of up to DYN_SEG traces from its first trace, so its traces
share chunks as the builder intends (the host test asserts the chunks).
segment_border is about the border between two segments and therefore takes
more than DYN_SEG traces; many_long (about its long traces, each a chunk of
its own) and pack_only_empty (no span at all) get no fillers.

Regimes of a shape ("<shape>-<regime>")
  F   not declared unique: the forward scan
  B   declared unique, S = 9, ANOMOD_UNIQUE_SCAN=1: the scan from both ends
      (only where the set holds no trace longer than a chunk)
  P   declared unique, ANOMOD_UNIQUE_SCAN=1, S = 30 (wider than NARROW_ROWS
      edge rows) or a long trace present (then S = 9): the split-word scan
Shapes with a duplicated id run F only.

Not reachable by a test: big_parents' guard for a trace of 2^32 - 2 spans (the
window loop leaving before its u32 start wraps) — a set of that size fits no
test; it stays untested."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

import anomod
import trace_struct_ref as T
from critical_path_ref import cp_table_ref, critical_path_ref, random_starts
from error_origins_ref import origins_ref
from self_time_ref import NO_PARENT, parents_ref, self_table_ref, self_us_ref
from spectrum_ref import rows_ref, spectrum_ref
from trace_shapes_ref import path_hash_ref, shapes_ref

STAGE = 256          # chunk.h kStage
CHUNK_TRACES = 64    # chunk.h kWave: traces per chunk
DYN = 4              # walk_traces<..., 4, ...>: the last quarter is dynamic
DYN_SEG = 512        # walk.h kDynSeg
FWD = 10             # walk.h kFwdScan
BIDIR = (6, 4)       # chunk.h kFwd, kBwd
SPLIT = (12, 4)      # walk.h kSplitFwd, kSplitBwd
SCAN_SLACK = 16      # chunk.h kScanSlack
NARROW_ROWS = 512    # walk.h kNarrowRows
BIG_WIN = 2048       # walk.h kBigWin
BIG_BLOCK = 4096     # walk.h kBigThreads * kBigPer
BIG_SLOTS = 4096     # walk.h kBigSlots = 2 * kBigWin
MI355X_CUS = T.MI355X_CUS
U32_MAX = 2**32 - 1
ERR = anomod.FLAG_ERROR
SCAN_LOG = {"fwd": "forward", "bidir": "bidir", "split": "split"}   # span_walk.hip scan_name
PASSES = ("self_time", "critical_path", "trace_shapes", "spectrum", "error_origins")
assert (T.STAGE, T.CHUNK_TRACES, T.DYN_SEG) == (STAGE, CHUNK_TRACES, DYN_SEG)


# ------------------------------------------------------------------ the model
def big_slot(ids) -> np.ndarray:
    """walk.h big_slot: bits 32..43 of id * 0x9E3779B97F4A7C15 (mod 2^64)."""
    ids = np.asarray(ids, np.uint64)
    with np.errstate(over="ignore"):
        h = ids * np.uint64(0x9E3779B97F4A7C15)
    return ((h >> np.uint64(32)) & np.uint64(BIG_SLOTS - 1)).astype(np.int64)


def tail_start(nt: int) -> int:
    return nt - nt // DYN


def tail_chunks(lens) -> list:
    """(first trace, k, n) of every chunk over the dynamic tail."""
    return T.tail_chunks(list(lens), tail_start(len(lens)))


def scan_of(declared_unique: bool, S: int, has_long: bool) -> str:
    """pick_walk_scan, for a set whose order hint (or ANOMOD_UNIQUE_SCAN=1)
    lets a declared set scan from both ends."""
    if not declared_unique:
        return "fwd"
    return "split" if (S + 2) * S > NARROW_ROWS or has_long else "bidir"


def big_windows(L: int) -> int:
    return -(-L // BIG_WIN)


def big_blocks(L: int) -> int:
    return -(-L // BIG_BLOCK)


def _widths(kind):
    return {"fwd": (FWD, 0), "bidir": BIDIR, "split": SPLIT}[kind]


@dataclass(frozen=True)
class Step:
    f: int          # forward block [f, f + FW)
    valid: int      # its ids inside the trace: min(b - f, FW)
    gb: int         # backward block [gb, gb + BW), clamped to the trace start
    nb: int         # its ids not seen before: g - gb + 1 (<= 0: none)
    clamped: bool


def scan_steps(a, b, i, kind) -> list:
    """Every step the scan of span i of [a, b) can take, in order."""
    FW, BW = _widths(kind)
    out = []
    for s in range(-(-(b - a) // FW)):
        f, g = a + s * FW, i - 1 - s * BW
        gb = max(a, g - BW + 1)
        out.append(Step(f, min(b - f, FW), gb, g - gb + 1 if BW else 0,
                        bool(BW) and g - BW + 1 < a))
    return out


@dataclass(frozen=True)
class Hit:
    step: int       # the step that returns (the number of steps for q = None)
    side: str       # "f" forward block, "b" backward block, "" not found
    slot: int       # slot within that block
    valid: int      # valid ids of the forward block at that step
    clamped: bool   # the backward block of that step was clamped
    clamps: tuple   # max(nb, 0) of every clamped backward block up to that step


def scan_hit(a, b, i, q, kind) -> Hit:
    """Where the device's scan finds position q (the only carrier of the
    reference in [a, b); None: no carrier) for span i of the trace [a, b)."""
    FW, BW = _widths(kind)
    n_steps = -(-(b - a) // FW)
    if q is None:
        step, side = n_steps - 1, ""
    else:
        sf = (q - a) // FW
        sb = (i - 1 - q) // BW if BW and q <= i - 1 else None
        step, side = (sf, "f") if sb is None or sf <= sb else (sb, "b")   # a tie: forward first
    f, g = a + step * FW, i - 1 - step * BW
    gb = max(a, g - BW + 1)
    slot = -1 if q is None else q - f if side == "f" else q - gb
    clamps = tuple(max(i - 1 - s * BW - a + 1, 0) for s in range(step + 1)
                   if BW and i - 1 - s * BW - BW + 1 < a)
    return Hit(step + (q is None), side, slot, min(b - f, FW), bool(BW) and g - BW + 1 < a, clamps)


def hit_combo(h: Hit, kind) -> tuple:
    """The ladder's coordinates of a hit: side, slot, first / later step, and
    for the forward side whether the block held one valid id, all, or some."""
    FW, _ = _widths(kind)
    when = "first" if h.step == 0 else "later"
    if h.side == "f":
        return ("f", h.slot, when, "one" if h.valid == 1 else "full" if h.valid == FW else "part")
    return ("b", h.slot, when)


def ladder_required(kind) -> set:
    """Every combination a ladder must hold.  Left out because no input
    reaches them: a hit in a clamped backward block (the block then lies
    inside [a, a + BW), which the forward side has covered since its first
    step, BW <= FW, and a tie goes forward) — the clamped blocks are covered as
    blocks passed on the way (ladder_clamps) and by the decoys; a forward block
    of one valid id holds it in slot 0, at the first step only in a one-span
    trace."""
    FW, BW = _widths(kind)
    req = {("f", s, w, "full") for s in range(FW) for w in ("first", "later")}
    req |= {("f", 0, "first", "one"), ("f", 0, "later", "one")}
    req |= {("b", s, w) for s in range(BW) for w in ("first", "later")}
    return req


# ------------------------------------------------------------------ shapes
Shape = T.Shape
_ids = T._ids


def _rand_tree(seed, L, orphan=0.04):
    """L spans, unique ids, every span under a random earlier one (a few
    orphans), then shuffled inside the trace (children before parents)."""
    rng = np.random.default_rng(seed)
    sid = _ids(seed, L) if L else np.zeros(0, np.uint64)
    pos = np.arange(L)
    pid = np.where(pos > 0, sid[(rng.random(L) * np.maximum(pos, 1)).astype(np.int64)],
                   np.uint64(0)) if L else sid.copy()
    orph = (pos > 0) & (rng.random(L) < orphan)
    pid[orph] = rng.integers(1, 1 << 39, int(orph.sum()), dtype=np.uint64)
    order = rng.permutation(L)
    return sid[order], pid[order]


def _trees(seed, lens):
    return [_rand_tree(seed * 10007 + k, L) for k, L in enumerate(lens)]


def _chain_nbr(seed, L):
    sid = _ids(seed, L)
    return sid, T._chain_pid(sid, np.arange(L))


def _ladder_target(kind, L, prev_ids, next_ids, seed, aliases):
    """One trace of L spans between prev and next: self-references at its
    first and last position, orphans naming ids of the neighbours (the decoys:
    distance d past the end = next[d - 1], d before the start = prev[-d]),
    for the split scan the low-word aliases, and every other span under the
    parent that covers a combination of ladder_required not yet covered."""
    FW, BW = _widths(kind)
    BWd = BW or 4                                    # decoys before the start for every kind
    ids = _ids(seed, L)
    par = {0: 0, L - 1: L - 1}                       # position -> parent position (own: a head)
    pid = np.zeros(L, np.uint64)
    decoys, alias = [], {}
    for d in range(1, FW + 1):
        pid[d] = next_ids[d - 1]
        decoys.append((d, "next", d))
    for d in range(1, BWd + 1):
        pid[FW + d] = prev_ids[len(prev_ids) - d]
        decoys.append((FW + d, "prev", d))
    taken = set(range(1, FW + BWd + 1))
    if aliases:
        q, r, i = 3 * FW + 5, FW + BWd + 2, L - 2    # r: an earlier block than the true parent q
        ids[r] = ids[q] ^ np.uint64(1 << 40)
        par[i] = q
        pid[L - 3] = ids[2 * FW + 1] ^ np.uint64(1 << 41)   # a low-word alias, no true parent
        pid[L - 4] = next_ids[0] ^ np.uint64(1 << 42)       # the alias sits in the next trace
        taken |= {L - 3, L - 4}
        alias = {"false_candidate": (i, r, q), "no_parent": (L - 3, 2 * FW + 1),
                 "neighbour": (L - 4, 0)}

    def cycle(i, q):
        seen = 0
        while q in par and par[q] != q and seen <= L:
            if q == i:
                return True
            q, seen = par[q], seen + 1
        return q == i

    missing = ladder_required(kind)
    covered = set()
    for i in range(L):
        if i in par:
            covered.add(hit_combo(scan_hit(0, L, i, par[i], kind), kind))
    for i in range(1, L - 1):
        if i in par or i in taken:
            continue
        for q in list(range(i - 1, -1, -1)) + list(range(i + 1, L)):
            c = hit_combo(scan_hit(0, L, i, q, kind), kind)
            if c in missing and c not in covered and not cycle(i, q):
                par[i] = q
                covered.add(c)
                break
        else:
            par[i] = 0
    for i, q in par.items():
        pid[i] = ids[q]
    return (ids, pid), {"par": par, "decoys": decoys, "alias": alias, "orphans": sorted(taken)}


def _ladder(kind):
    FW, BW = _widths(kind)
    BWd = BW or 4
    seed = {"fwd": 4100, "bidir": 4200, "split": 4300}[kind]
    mult = 8 if kind == "bidir" else 6
    traces, targets = [], {}
    for L in (mult * FW + 1, mult * FW):
        prev, nxt = _chain_nbr(seed + L, BWd + 4), _chain_nbr(seed + L + 500, FW + 4)
        tgt, info = _ladder_target(kind, L, prev[0], nxt[0], seed + L + 900,
                                   aliases=kind == "split" and L % FW == 1)
        traces += [prev, tgt, nxt]
        targets[len(traces) - 2] = info
    # traces shorter than a backward block between 4-span neighbours: both
    # blocks read the next trace.  (length, references: "n<k>" next[k],
    # "p<k>" prev[-k], "self")
    minis = [(1, ["n0"]), (1, ["n1"]), (1, ["self"]), (2, [None, "n0"]), (2, [None, "n1"]),
             (3, [None, "n0", "n0"]), (2, [None, "p1"]), (3, [None, "p2", "n2"])]
    nbrs = [_chain_nbr(seed + 7000 + k, 4) for k in range(len(minis) + 1)]
    for k, (L, refs) in enumerate(minis):
        ids = _ids(seed + 8000 + k, L)
        pid = np.zeros(L, np.uint64)
        decoys, par = [], {}
        for i, r in enumerate(refs):
            if r == "self":
                pid[i], par[i] = ids[i], i
            elif r is not None:
                d = int(r[1:])
                pid[i] = nbrs[k + 1][0][d] if r[0] == "n" else nbrs[k][0][4 - d]
                decoys.append((i, "next", d + 1) if r[0] == "n" else (i, "prev", d))
        traces += [nbrs[k], (ids, pid)]
        targets[len(traces) - 1] = {"par": par, "decoys": decoys, "alias": {},
                                    "orphans": [i for i, r in enumerate(refs)
                                                if r not in (None, "self")]}
    traces.append(nbrs[-1])
    return Shape(traces, target=1, facts={"ladder": kind, "targets": targets})


def _word_border_starts():
    """Three chunks of exactly 256 spans.  Trace starts on 63, 64, 127, 128,
    191, 192 and 255 (the lane == 63 / b == 63 selects of trace_bounds and
    rank_at), a one-span trace at 255, a 140-span trace covering mask words 1
    and 2 without a start in them, empty traces at a chunk's front, between
    traces and at its end."""
    X = [63, 1, 63, 1, 63, 1, 63, 1]
    Y = [60, 0, 140, 55, 1]
    Z = [64, 64, 64, 63, 1]
    lens = [0] + X + [0] + Y + [0, 0] + Z
    return Shape(_trees(51, lens), target=1,
                 facts={"chunks": [(10, 256), (7, 256), (5, 256)],
                        "starts": {63, 64, 127, 128, 191, 192, 255},
                        "bare_words": [(1, 1), (1, 2)]})


def _pack_span_limit():
    lens = [253, 3] + [254] + [3, 253] + [3, 5] * 32 + [2] * 63 + [257]
    return Shape(_trees(52, lens), target=len(lens) - 1,
                 facts={"chunks": [(2, 256), (1, 254), (2, 256), (64, 256), (63, 126), (0, 257)]})


def _segment_border():
    """More than DYN_SEG traces on purpose: the tail's segments are [0, 512),
    [512, 1024) and [1024, 1084).  A long trace is the last of segment 0, one
    the first of segment 1, and short traces lie on both sides of 1024, where
    a chunk must end although the next traces would fit."""
    lens = [1 + j % 3 for j in range(1084)]
    lens[511], lens[512] = 300, 260
    return Shape(_trees(53, lens), target=511,
                 facts={"segments": [512, 1024], "long_at": {511: 300, 512: 260}})


def _big_cluster_4095():
    """A 600-span trace (one table window) in which 48 ids are at home in slot
    4095, so their probes wrap to slot 0 and displace the 40 ids at home in
    slots 0..39; the chain runs through the cluster, and a span with id 0 (the
    table's empty key: never inserted, never a parent) sits in the middle."""
    draw = np.unique(np.random.default_rng(54).integers(1, 2**64, 1 << 20, dtype=np.uint64))
    slot = big_slot(draw)
    cluster = draw[slot == BIG_SLOTS - 1][:48]
    assert len(cluster) >= 40, "the fixed draw no longer fills one table slot"
    front = draw[slot < 40][:40]
    rest = draw[(slot >= 40) & (slot < BIG_SLOTS - 1)][:600 - len(cluster) - len(front)]
    sid = np.concatenate([rest[:100], cluster, front, rest[100:]])
    L, zero = len(sid), 300
    order = T._order("shuf", L, seed=54)
    order = order[order != zero]
    pid = T._chain_pid(sid, order)
    sid[zero] = 0
    pid[zero] = sid[order[7]]
    return Shape([(sid, pid)], facts={"cluster": (BIG_SLOTS - 1, int(len(cluster))),
                                      "zero_at": zero, "chain": order})


def _big_window_borders():
    """Long traces of 2048..6145 spans, random trees with planted parents: the
    last position of every table window and the first of the next, a parent in
    a last window of one span, a child in span block 1 under window 0 and
    children in block 0 under parents in block 1, and (from 4096 spans on) an
    id at 30 and again at 2078, a window later, with children right behind the
    later copy: the first copy is the parent."""
    traces, planted, dups = [], {}, {}
    for t, L in enumerate((2048, 2049, 4096, 4097, 6145)):
        rng = np.random.default_rng(5500 + L)
        sid = _ids(5500 + L, L)
        pos = np.arange(L)
        pid = sid[(rng.random(L) * np.maximum(pos, 1)).astype(np.int64)]
        pid[0] = 0
        want = {}
        for w in range(big_windows(L) - 1):
            e = BIG_WIN * (w + 1)
            want[10 + 2 * w], want[11 + 2 * w] = e - 1, e
            pid[e - 1] = pid[e] = sid[0]
        if L > BIG_BLOCK:
            want[L - 1] = 5                                   # block 1 under window 0
        if L >= BIG_BLOCK:
            sid[2078] = sid[30]
            want[2079], want[2080] = 30, 30
            dups[t] = (30, 2078)
        for c, p in want.items():
            pid[c] = sid[p]
        traces.append((sid, pid))
        planted[t] = want
    return Shape(traces, target=4, dup=True, facts={"planted": planted, "dups": dups})


CHAIN_LENS = (255, 256, 257, 4095, 4096, 4097, 8193)
REUSED = tuple(f"chain_{k}_{L}" for k in ("fwd", "rev", "shuf") for L in CHAIN_LENS) + (
    "pack_64x4", "pack_65x4", "pack_chain256_then_1", "pack_empty_w1", "pack_empty_w2",
    "pack_only_empty", "cycle_self_parent", "cycle_two", "cycle_whole_fwd_6",
    "cycle_whole_rev_256", "cycle_whole_shuf_256", "cycle_whole_shuf_300", "cycle_beside_tree",
    "lookup_low_word_twins_10", "lookup_low_word_twins_300", "many_long")
NEW = {"scan_ladder_fwd": functools.partial(_ladder, "fwd"),
       "scan_ladder_bidir": functools.partial(_ladder, "bidir"),
       "scan_ladder_split": functools.partial(_ladder, "split"),
       "word_border_starts": _word_border_starts, "pack_span_limit": _pack_span_limit,
       "segment_border": _segment_border, "big_cluster_4095": _big_cluster_4095,
       "big_window_borders": _big_window_borders}
SHAPES = REUSED + tuple(NEW)
NO_FILLERS = ("many_long", "pack_only_empty")


@functools.lru_cache(maxsize=None)
def shape(name, n_cus=MI355X_CUS) -> Shape:
    if name in NEW:
        return NEW[name]()
    return T._shape(name, n_cus)


def _lens(sh) -> list:
    return [len(t[0]) for t in sh.traces]


def has_long(sh) -> bool:
    return max(_lens(sh), default=0) > STAGE


def regimes(name) -> tuple:
    sh = shape(name)
    if sh.dup:
        return ("F",)
    return ("F", "P") if has_long(sh) else ("F", "B", "P")


def case_names() -> list:
    return [f"{s}-{r}" for s in SHAPES for r in regimes(s)]


# ------------------------------------------------------------------ placement, decoration
def in_tail(traces, seed=556):
    """(3 m one-span root traces + the m traces, 3 m): the shape becomes the
    dynamic tail of the set."""
    m = len(traces)
    fill = [(x, np.zeros(1, np.uint64)) for x in _ids(seed, 3 * m).reshape(3 * m, 1)]
    return fill + list(traces), 3 * m


def decorate(traces, S, unique, seed) -> anomod.SpanSet:
    """The span set of the traces (ids, parent references) with everything the
    passes read beyond them, from a fixed seed: services by position, shifted
    from one trace to the next (never more than 9, whatever S); error flags
    on a quarter of the spans; durations with 0 and 2^32 - 1 among them; start
    times laid around the parents' intervals along the tree (not sorted by
    position)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray([len(t[0]) for t in traces], np.int64)
    ptr = np.zeros(len(traces) + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    n = int(ptr[-1])
    cat = lambda k: (np.concatenate([np.asarray(t[k], np.uint64) for t in traces])  # noqa: E731
                     if traces else np.zeros(0, np.uint64))
    t_of = np.repeat(np.arange(len(traces), dtype=np.int64), lens)
    pos = np.arange(n) - ptr[:-1].astype(np.int64)[t_of]
    svc = (2 * pos + 5 * t_of + pos // 7) % 9
    flags = (rng.random(n) < 0.25) * ERR
    dur = rng.integers(1, 20000, n)
    u = rng.random(n)
    dur[u < 0.04] = 0
    dur[u > 0.98] = U32_MAX
    if n >= 2:
        dur[0], dur[n - 1] = 0, U32_MAX
    th = np.repeat(_ids(77, len(traces)) if traces else np.zeros(0, np.uint64), lens)
    sp = anomod.SpanSet([f"s{i:02d}" for i in range(S)], ptr, th, cat(0), cat(1),
                        svc.astype(np.uint16), flags.astype(np.uint16), dur.astype(np.uint32),
                        unique_ids=unique, start_us=np.zeros(n, np.uint64))
    return random_starts(sp, seed + 1) if n else sp


@dataclass
class Case:
    name: str
    shape_name: str
    regime: str
    sp: anomod.SpanSet
    S: int
    scan: str            # the scan the model expects: "fwd", "bidir", "split"
    n_long: int
    first: int           # the shape's first trace (after the fillers)
    facts: dict
    env: dict            # what the regime sets for the calls

    @property
    def lens(self):
        return np.diff(self.sp.trace_ptr.astype(np.int64))

    def bounds(self, t):
        """[a, b) of trace t of the shape."""
        p = self.sp.trace_ptr
        return int(p[self.first + t]), int(p[self.first + t + 1])

    @functools.cached_property
    def par(self):
        return parents_ref(self.sp)

    @functools.cached_property
    def thr(self):
        """Spectrum thresholds: the upper half of the ordinary durations."""
        E = (self.S + 2) * self.S
        return np.random.default_rng(9).integers(10000, 20000, E).astype(np.uint32)

    @functools.cached_property
    def refs(self) -> dict:
        """What each pass's own reference says about the set."""
        sp, par = self.sp, self.par
        if sp.n_spans == 0:
            return {}
        su = self_us_ref(sp, par)
        cp, on, nsel = critical_path_ref(sp, par)
        P, on_tree = path_hash_ref(sp, par)
        rows = rows_ref(sp)
        return {"self_time": (su, self_table_ref(sp, su)),
                "critical_path": (cp, on, nsel, cp_table_ref(sp, cp, on)),
                "trace_shapes": (P, on_tree, shapes_ref(sp, P, on_tree)),
                "spectrum": (rows, spectrum_ref(sp, self.thr, True, rows)),
                "error_origins": origins_ref(sp, par)}


@functools.lru_cache(maxsize=4)
def case(name, n_cus=MI355X_CUS) -> Case:
    shape_name, regime = name.rsplit("-", 1)
    sh = shape(shape_name, n_cus)
    assert regime in regimes(shape_name)
    traces, first = list(sh.traces), 0
    if shape_name not in NO_FILLERS:
        traces, first = in_tail([t[:2] for t in traces])
    long_ = has_long(sh)
    S = 30 if regime == "P" and not long_ else 9
    sp = decorate([t[:2] for t in traces], S, regime != "F", zlib.crc32(shape_name.encode()))
    n_long = sum(1 for L in _lens(sh) if L > STAGE)
    env = {"ANOMOD_LOG_KERNEL": "1"}
    if regime != "F":
        env["ANOMOD_UNIQUE_SCAN"] = "1"
    return Case(name, shape_name, regime, sp, S, scan_of(regime != "F", S, long_), n_long, first,
                dict(sh.facts), env)

"""Model of the shared edge stream (a plain helper, not a conftest): the
decisions of csrc/edge_stream.h and csrc/edge_stream.hip restated in plain
Python, and the builders of the span sets that put a border of the driver under
each of the four passes that run on it (the windowed edge table, the per-window
quantiles, the edge load, the edge exemplars).  Nothing here computes what a
pass computes: the expected results are the passes' own reference helpers
(refs() below only calls them).

The model
  grid_of          stream_grid: the workgroups of a launch and the spans each
                   owns, for a workgroup cap of at most 4 that does not exceed
                   the batch count (then no device property enters).
  lane_positions   Lanes<THREADS, RUN>::pos: the four spans of a lane.
  tile_of / exemplars_place   the host side's LDS decisions.
  ring_events      WindowRing for one workgroup, step by step: the three-deep
                   batch minima, advance, slot_of and finish.  It returns which
                   spans hit the LDS tile, the events of the walk, and the table
                   that the flushed slots plus the global adds make — which must
                   be the plain per-span table (test_stream_ref_host.py).
  simulate         a whole launch of a ring pass: every workgroup's ring.
  sorted_cells / cell_borders   what window_cell_bounds_kernel streams.

Events of a ring walk, as (workgroup, name, batch, ...):
  anchor (base)         the first batch with a window
  advance (adv)         the batch minimum rose by adv
  wrap                  slot0 + adv reached or passed Wt (adv < Wt)
  jump                  adv >= Wt: the whole tile flushed, slot0 back to 0
  backward              the batch minimum is below base
  no_window_batch       no live span of the batch has a window
  straddle              one batch with windows inside and outside the tile
  finish_cut            finish() stopped at T before it had walked Wt slots
  never_anchored        the workgroup saw no window at all

Cases are named "<id>@<batch>": a case that depends on the batch size is built
for the 2048-span batch of edge_windows_kernel, edge_load_kernel and
edge_exemplars_kernel and for the 1024-span batch of the two quantile stream
kernels.  Sets are laid out by position: traces of one to three spans (roots,
children of a span of the same trace, a few orphans), S = 2 or 3, so that E is
small and the tile is set by the *_TILE cap.  The d cases, whose cell
populations must be exact, use one-span root traces (cell = window, service).

Not reachable by a test: the kStreamMaxRange clamp of 2^31 spans a workgroup
(no test can hold such a set) and the occupancy-derived default grid (it
depends on the device; the per-pass tests run it)."""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import anomod
from anomod.spans import edge_rows
from edge_exemplars_ref import exemplars_ref
from edge_load_ref import edge_load_brute, edge_load_ref
from edge_window_quantiles_ref import edge_window_quantiles_ref
from edge_windows_ref import edge_windows_ref
from oracle import native

WAVE = 64
B_WIDE = 2048            # kWinThreads / kLoadThreads / kExThreads (512) * 4
B_CELL = 1024            # edge_window_quantiles.hip kCellThreads (256) * 4
THREADS = {B_WIDE: 512, B_CELL: 256}
WIN_LDS = 64 * 1024 - 64     # edge_windows.hip kWinLdsBudget
WIN_CELL = 20                # edge_windows.hip kCellBytes
LOAD_LDS = 40 * 1024 - 64    # edge_load.hip kLoadLdsBudget
LOAD_CELL = 8                # edge_load.hip: one u64 a cell
EX_LDS = 40 * 1024 - 64      # edge_exemplars.hip kExLdsBudget
CELL_PER_CU = 8              # edge_window_quantiles.hip cell_grid
NO_CAP = 0xFFFFFFFF          # edge_stream.hip env_cap: unset
ERR = anomod.FLAG_ERROR
RING_PASSES = ("windows", "load")
PASSES = ("windows", "load", "quantiles", "exemplars")
KERNEL = {"windows": "edge_windows_kernel", "load": "edge_load_kernel",
          "exemplars": "edge_exemplars_kernel"}
ENV = {"windows": ("ANOMOD_EDGE_WINDOWS_WGS", "ANOMOD_EDGE_WINDOWS_TILE"),
       "load": ("ANOMOD_EDGE_LOAD_WGS", "ANOMOD_EDGE_LOAD_TILE"),
       "quantiles": ("ANOMOD_EDGE_WINDOW_QUANTILES_WGS", None),
       "exemplars": ("ANOMOD_EXEMPLARS_WGS", None)}
T0 = 10**9
STEP = 1000


# ------------------------------------------------------------------ the model
def grid_of(n: int, B: int, cap: int):
    """stream_grid: (grid, per_wg) of n > 0 positions in batches of B under a
    workgroup cap.  Only for caps that bind on every device: at most 4 (fewer
    than any device's resident workgroups) and at most the batch count."""
    batches = -(-n // B)
    assert 1 <= cap <= 4 and cap <= batches, (n, B, cap)
    per_wg = -(-batches // cap) * B
    return -(-n // per_wg), per_wg


def wg_ranges(n: int, B: int, cap: int):
    grid, per_wg = grid_of(n, B, cap)
    return [(g * per_wg, min(g * per_wg + per_wg, n)) for g in range(grid)]


def lane_positions(b: int, tid: int, threads: int, run: int):
    """Lanes<threads, run>::pos(j), j = 0..3."""
    return [b + tid * run + (j // run) * threads * run + j % run for j in range(4)]


def tile_of(pass_name: str, E: int, T: int, cap: int = NO_CAP, busy: bool = True) -> int:
    """Wt of edge_windows_kernel / edge_load_kernel."""
    if pass_name == "windows":
        return min(WIN_LDS // (E * WIN_CELL), T, cap)
    return min(LOAD_LDS // (E * LOAD_CELL), T, cap) if busy else 0


def exemplars_place(E: int, K: int, lds_cap: int = NO_CAP) -> str:
    budget = min(EX_LDS, lds_cap)
    return "lds" if E * K * 8 <= budget else "cached" if E * 8 <= budget else "global"


def window_of(start, t0, step, T):
    """stream::window_of per span, -1 for none (int64; starts below 2^62)."""
    s = np.asarray(start, np.uint64).astype(np.int64)
    w = np.where(s >= t0, (s - t0) // step, T)
    return np.where(w < T, w, -1)


def load_head(start, dur, t0, step, T):
    """edge_load_kernel: (window of the head partial or -1, the head partial)."""
    s = np.asarray(start, np.uint64).astype(np.int64)
    d = np.asarray(dur, np.int64)
    e = s + d
    before = s < t0
    aw = np.where(before, 0, (s - t0) // step)
    none = (e == s) | (e <= t0) | (aw >= T)
    oa = np.where(before, 0, (s - t0) - aw * step)
    ln = np.where(before, e - t0, d)
    head = np.minimum(ln, step - oa)
    return np.where(none, -1, aw), np.where(none, 0, head)


@dataclass
class RingTrace:
    hit: np.ndarray       # bool per position of [lo, hi): went to the LDS tile
    events: list          # (name, batch, ...)
    table: np.ndarray     # u64 [T, E] from the flushed slots and the global adds


def ring_events(windows, live, lo, hi, B, Wt, T, rows=None, values=None, E=1) -> RingTrace:
    """WindowRing over the batches of one workgroup's range [lo, hi).  windows:
    the pass's window per position (-1: none); live: the span lies in a trace;
    rows / values: the cell row and the addend of each position."""
    n = len(windows)
    rows = np.zeros(n, np.int64) if rows is None else np.asarray(rows, np.int64)
    values = np.ones(n, np.uint64) if values is None else np.asarray(values, np.uint64)
    table = np.zeros((T, E), np.uint64)
    lds = np.zeros((max(Wt, 1), E), np.uint64)
    hit = np.zeros(hi - lo, bool)
    events = []
    NONE = 1 << 32
    s_min = [NONE] * 3                       # WindowRing::s_min, init()
    anchored, base, slot0 = False, 0, 0

    def flush(slot, w):
        table[w] += lds[slot]
        lds[slot] = 0

    for it, b in enumerate(range(lo, hi, B)):
        pos = np.arange(b, min(b + B, hi))
        pos = pos[live[pos] & (windows[pos] >= 0)]
        ws = windows[pos]
        if Wt:
            # advance(): the batch minimum through slot it % 3, the slot of
            # batch it - 1 cleared for batch it + 2
            if len(ws):
                s_min[it % 3] = min(s_min[it % 3], int(ws.min()))
            bmin = s_min[it % 3]
            s_min[(it + 2) % 3] = NONE
            assert bmin == (int(ws.min()) if len(ws) else NONE), "a stale batch minimum"
            if bmin == NONE:
                events.append(("no_window_batch", it))
            elif not anchored:
                anchored, base = True, bmin
                events.append(("anchor", it, bmin))
            elif bmin > base:
                adv = bmin - base
                for k in range(min(adv, Wt)):
                    flush((slot0 + k) % Wt, base + k)
                events.append(("advance", it, adv))
                if adv >= Wt:
                    events.append(("jump", it))
                    slot0 = 0
                else:
                    if slot0 + adv >= Wt:
                        events.append(("wrap", it))
                    slot0 = (slot0 + adv) % Wt
                base = bmin
            elif bmin < base:
                events.append(("backward", it))
        inside = (ws >= base) & (ws - base < Wt) if (Wt and anchored) else np.zeros(len(ws), bool)
        if inside.any() and not inside.all():
            events.append(("straddle", it))
        slot = (slot0 + ws[inside] - base) % max(Wt, 1)
        np.add.at(lds, (slot, rows[pos[inside]]), values[pos[inside]])
        np.add.at(table, (ws[~inside], rows[pos[~inside]]), values[pos[~inside]])
        hit[pos[inside] - lo] = True
    if Wt:                                   # finish()
        if anchored:
            k = 0
            while k < Wt and base + k < T:
                flush((slot0 + k) % Wt, base + k)
                k += 1
            if k < Wt:
                events.append(("finish_cut", k))
        else:
            events.append(("never_anchored",))
    assert not lds.any()
    return RingTrace(hit, events, table)


def stream_grid_literal(num_cus, n, batch, per_cu, cap, max_range):
    """stream_grid of csrc/edge_stream.hip, line by line."""
    batches = (n + batch - 1) // batch
    grid = min(num_cus * per_cu, batches)
    grid = min(grid, cap)
    per_wg = (batches + grid - 1) // grid * batch
    if per_wg > max_range:
        per_wg = max_range
    return (n + per_wg - 1) // per_wg, per_wg


# ------------------------------------------------------------------ the cases
@dataclass
class Case:
    name: str
    sp: object
    B: int
    T: int
    cap: int
    tile: object                  # the *_TILE cap, None: no cap
    passes: tuple
    t0: int = T0
    step: int = STEP
    expect: dict = field(default_factory=dict)
    ks: tuple = (3,)              # exemplars: the K values
    places: tuple = ("lds",)      # exemplars: the list placements
    errors_only: bool = False
    ring_extra: bool = False      # ring cases: tile 0, busy only, carried only as well

    @property
    def begin(self):
        return int(self.sp.trace_ptr[0])

    @property
    def end(self):
        return int(self.sp.trace_ptr[-1])

    @property
    def E(self):
        return edge_rows(len(self.sp.services))

    def env(self, tile="case", lds=None) -> dict:
        """The caps of every pass, as environment strings."""
        tile = self.tile if tile == "case" else tile
        out = {}
        for p in PASSES:
            wgs, tl = ENV[p]
            out[wgs] = str(self.cap)
            if tl is not None and tile is not None:
                out[tl] = str(tile)
        if lds is not None:
            out["ANOMOD_EXEMPLARS_LDS"] = str(lds)
        return out

    def live(self):
        pos = np.arange(self.sp.n_spans)
        return (pos >= self.begin) & (pos < self.end)

    def rows(self):
        """The edge row of every position (oracle.native.span_edges)."""
        return _rows(self.name)

    def refs(self) -> dict:
        """The reference of every pass of the case, by the passes' own helpers."""
        return _refs(self.name)


@functools.lru_cache(maxsize=None)
def _rows(name):
    c = case(name)
    return native.span_edges(c.sp, len(c.sp.services)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = case(name)
    sp, r = c.sp, {}
    if "windows" in c.passes:
        r["windows"] = edge_windows_ref(sp, c.t0, c.step, c.T)
    if "load" in c.passes:
        r["load"] = edge_load_ref(sp, c.t0, c.step, c.T)
    if "quantiles" in c.passes:
        r["quantiles"] = edge_window_quantiles_ref(sp, c.t0, c.step, c.T)
    if "exemplars" in c.passes:
        r["exemplars"] = {k: exemplars_ref(sp, k, 1 if c.errors_only else 0) for k in c.ks}
    return r


def load_brute(c):
    """edge_load_brute of a case small enough for it, else None."""
    if c.sp.n_spans > 2 * B_WIDE + 16 or c.T > 64:
        return None
    return edge_load_brute(c.sp, c.t0, c.step, c.T)


def pass_windows(c: Case, pass_name: str):
    """(window, addend) per position as the ring of `pass_name` sees them."""
    sp = c.sp
    if pass_name == "windows":
        return window_of(sp.start_us, c.t0, c.step, c.T), sp.dur_us.astype(np.uint64)
    w, head = load_head(sp.start_us, sp.dur_us, c.t0, c.step, c.T)
    return w, head.astype(np.uint64)


def geometry(c: Case, pass_name: str):
    """[(kernel, positions, grid, per_wg)] of the stream launches of a pass."""
    if pass_name == "quantiles":
        return [("window_cell_keys_kernel", c.end) + grid_of(c.end, B_CELL, c.cap),
                ("window_cell_bounds_kernel", c.end - c.begin)
                + grid_of(c.end - c.begin, B_CELL, c.cap)]
    return [(KERNEL[pass_name], c.end) + grid_of(c.end, B_WIDE, c.cap)]


def simulate(c: Case, pass_name: str, tile="case", busy=True, ones=False):
    """Every workgroup's ring of a launch of a ring pass: (Wt, events with the
    workgroup in front, table, hits).  ones: count spans instead of adding the
    pass's addend."""
    assert pass_name in RING_PASSES
    tile = c.tile if tile == "case" else tile
    Wt = tile_of(pass_name, c.E, c.T, NO_CAP if tile is None else tile, busy)
    w, val = pass_windows(c, pass_name)
    val = np.ones(len(w), np.uint64) if ones else val
    live, rows = c.live(), c.rows()
    table = np.zeros((c.T, c.E), np.uint64)
    events, hits = [], 0
    for g, (lo, hi) in enumerate(wg_ranges(c.end, B_WIDE, c.cap)):
        tr = ring_events(w, live, lo, hi, B_WIDE, Wt, c.T, rows, val, c.E)
        table += tr.table
        events += [(g,) + e for e in tr.events]
        hits += int(tr.hit.sum())
    return Wt, events, table, hits


def plain_table(c: Case, pass_name: str):
    """The per-span table of the ring's addends: no ring, no batches."""
    w, val = pass_windows(c, pass_name)
    ok = c.live() & (w >= 0)
    table = np.zeros((c.T, c.E), np.uint64)
    np.add.at(table, (w[ok], c.rows()[ok]), val[ok])
    return table


def sorted_cells(c: Case):
    """The cells of the sorted keys window_cell_bounds_kernel streams
    (T * E: the sentinel cell)."""
    w = window_of(c.sp.start_us, c.t0, c.step, c.T)
    cell = np.where(w >= 0, w * c.E + c.rows(), c.T * c.E)
    return np.sort(cell[c.begin:c.end], kind="stable")


def cell_borders(c: Case):
    """The positions i > 0 of the sorted keys at which a cell begins."""
    sc = sorted_cells(c)
    return (np.nonzero(np.diff(sc))[0] + 1).tolist()


def sentinel_start(c: Case):
    """Where the sentinel run begins in the sorted keys, None when absent."""
    sc = sorted_cells(c)
    i = int(np.searchsorted(sc, c.T * c.E))
    return i if i < len(sc) else None


# ------------------------------------------------------------------ set builder
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _build(name, win, begin=0, end=None, S=2, T=16, long_spans=False, singles=False,
           svc=None, dur=None, flags=None, zero_dur=False, dead_win=0):
    """A set of len(win) column positions whose spans [begin, end) lie in
    traces.  win[p]: the window position p starts in, -1: outside the range
    (before t0 at odd positions, after the last window at even ones).  The
    positions outside the traces hold spans that start in window dead_win, last
    4000 us and carry the error flag: counted anywhere, they show."""
    rng = _rng(name)
    win = np.asarray(win, np.int64)
    n = len(win)
    end = n if end is None else end
    assert 0 <= begin < end <= n
    pos = np.arange(n)
    dead = (pos < begin) | (pos >= end)
    win = np.where(dead, dead_win, win)
    if dur is None:
        dur = rng.integers(1, int(3.5 * STEP) if long_spans else 60, n)
        if zero_dur:
            dur[pos % 16 == 5] = 0
    dur = np.where(dead, 4000, dur).astype(np.uint32)
    off = rng.integers(0, STEP - 60, n)
    start = np.where(win >= 0, T0 + win * STEP + off,
                     np.where(pos % 2 == 0, T0 + T * STEP + off, T0 - 100 - off))
    if flags is None:
        flags = np.where(rng.random(n) < 0.25, ERR, 0)
    flags = np.where(dead, ERR, flags).astype(np.uint16)
    if svc is None:
        svc = rng.integers(0, S, n)
    # traces of 1, 2, 3, 2, 1, 3, ... spans over [begin, end)
    ptr, t = [begin], 0
    while ptr[-1] < end:
        ptr.append(min(ptr[-1] + (1 if singles else (1, 2, 3, 2, 1, 3)[t % 6]), end))
        t += 1
    ptr = np.asarray(ptr, np.uint64)
    ids = (pos + 1).astype(np.uint64)
    parent = np.zeros(n, np.uint64)
    thash = np.zeros(n, np.uint64)
    for t in range(len(ptr) - 1):
        a, b = int(ptr[t]), int(ptr[t + 1])
        thash[a:b] = t + 1
        if b - a >= 2:
            parent[a + 1] = ids[a]
        if b - a == 3:   # a grandchild, or an orphan: its parent is in no trace
            parent[a + 2] = ids[a + 1] if t % 2 else np.uint64(2**63 + a)
    return anomod.SpanSet([f"s{i}" for i in range(S)], ptr, thash, ids, parent,
                          svc.astype(np.uint16), flags, dur, unique_ids=True,
                          start_us=start.astype(np.uint64))


def _ordered(n, T):
    """Time-ordered windows over n positions with every 37th span outside."""
    p = np.arange(n)
    return np.where(p % 37 == 11, -1, p * T // n)


def _by_batch(pattern, B):
    """Windows of len(pattern) full batches: an int (every span), None (every
    span outside the range) or a function of the index inside the batch."""
    j = np.arange(B)
    out = []
    for x in pattern:
        if x is None:
            out.append(np.full(B, -1))
        elif callable(x):
            out.append(np.asarray(x(j), np.int64))
        else:
            out.append(np.full(B, x))
    return np.concatenate(out)


def _geom(n, B, cap):
    grid, per_wg = grid_of(n, B, cap)
    return {"grid": grid, "per_wg": per_wg}


def _passes(B):
    return ("windows", "load", "exemplars") if B == B_WIDE else ("quantiles",)


def _sizes(B):
    return {"1": 1, "B-1": B - 1, "B": B, "B+1": B + 1, "2B": 2 * B, "2B+1": 2 * B + 1}


CASES = {}


def _register():
    for B in (B_WIDE, B_CELL):
        tag = f"@{B}"
        # ---- a: range and batch
        for label, n in _sizes(B).items():
            CASES[f"a1-n={label}{tag}"] = functools.partial(_range_case, B=B, n=n, cap=1,
                                                            grid=1, per_wg=-(-n // B) * B)
        CASES[f"a2{tag}"] = functools.partial(_range_case, B=B, n=3 * B, cap=3, grid=3, per_wg=B)
        CASES[f"a3{tag}"] = functools.partial(_range_case, B=B, n=3 * B + 1, cap=3, grid=2,
                                              per_wg=2 * B)
        CASES[f"a4{tag}"] = functools.partial(_range_case, B=B, n=4 * B + 1, cap=3, grid=3,
                                              per_wg=2 * B)
        CASES[f"a5{tag}"] = functools.partial(_range_case, B=B, n=5 * B, cap=4, grid=3,
                                              per_wg=2 * B)
        # ---- b: spans outside the traces
        for label, begin in (("1", 1), ("2", 2), ("3", 3), ("B-1", B - 1), ("B", B),
                             ("B+1", B + 1)):
            CASES[f"b1-begin={label}{tag}"] = functools.partial(
                _range_case, B=B, n=2 * B + 7, cap=1, grid=1, per_wg=3 * B, begin=begin,
                late_anchor=begin >= B)
        CASES[f"b2{tag}"] = functools.partial(_range_case, B=B, n=6 * B, cap=3, grid=3,
                                              per_wg=2 * B, begin=2 * B + 5, idle_wg=0)
        CASES[f"b3{tag}"] = functools.partial(_range_case, B=B, n=B + 77, cap=1, grid=1,
                                              per_wg=2 * B, cols=B + 77 + B // 2 + 3)
        CASES[f"b4{tag}"] = functools.partial(_b4, B=B)
    CASES[f"b5@{B_CELL}"] = functools.partial(_range_case, B=B_CELL, n=4 * B_CELL + 1, cap=2,
                                              grid=2, per_wg=3 * B_CELL, begin=B_CELL + 1)


def _range_case(name, B, n, cap, grid, per_wg, begin=0, cols=None, late_anchor=False,
                idle_wg=None):
    """Groups a and b: n = trace_ptr[-1] positions under `cap` workgroups, time
    ordered over T = 16 windows with a tile of 2."""
    T = 16
    cols = n if cols is None else cols
    sp = _build(name, _ordered(cols, T), begin, n, T=T, zero_dur=True)
    exp = {p: {"grid": grid, "per_wg": per_wg} for p in _passes(B)}
    if B == B_WIDE:
        for p in RING_PASSES:
            exp[p]["Wt"] = 2
            if late_anchor:      # batch 0 gives no minimum
                exp[p]["first"] = [("no_window_batch", 0), ("anchor", 1)]
            if idle_wg is not None:
                exp[p]["events"] = {(idle_wg, "never_anchored")}
    return Case(name, sp, B, T, cap, 2, _passes(B), expect=exp)


def _b4(name, B):
    """The dead head and tail of the range and the spans before t0 would all
    carry the smallest window of their batch: the live spans start in windows
    3.., the anchor must be 3."""
    T = 16
    j = np.arange(2 * B)
    win = np.where(j % 2 == 1, np.where(j % 8 == 1, -1, 3 + j // B), 4 + j // B)
    sp = _build(name, win, 5, 2 * B - 3, T=T, dead_win=0)
    exp = {p: _geom(2 * B - 3, B, 1) for p in _passes(B)}
    if B == B_WIDE:
        for p in RING_PASSES:
            exp[p].update(Wt=2, first=[("anchor", 0, 3), ("advance", 1, 1)])
    return Case(name, sp, B, T, 1, 2, _passes(B), expect=exp)


# ---- c: the ring (the 2048-span batch; the windows pass and the load pass)
def _ring_case(name, pattern, Wt, T=16, events=(), first=None, long_spans=False, n_cut=0):
    win = _by_batch(pattern, B_WIDE)
    if n_cut:
        win = win[:len(win) - n_cut]
    sp = _build(name, win, T=T, long_spans=long_spans)
    wt = min(Wt, T)
    exp = {p: dict(_geom(len(win), B_WIDE, 1), Wt=wt, names=set(events)) for p in RING_PASSES}
    if first:
        for p in RING_PASSES:
            exp[p]["first"] = first
    return Case(name, sp, B_WIDE, T, 1, Wt, RING_PASSES, expect=exp, ring_extra=True)


def _register_ring():
    W = f"@{B_WIDE}"
    for Wt in (1, 2, 3):
        # the minimum rises by exactly 1 a batch over 2 Wt + 2 batches: slot0
        # wraps exactly at Wt; windows k .. k + Wt in batch k
        pat = [(lambda j, k=k, Wt=Wt: k + j % (Wt + 1)) for k in range(2 * Wt + 2)]
        CASES[f"c1-Wt={Wt}{W}"] = functools.partial(
            _ring_case, pattern=pat, Wt=Wt, events=("anchor", "advance", "wrap") if Wt > 1
            else ("anchor", "advance", "jump"))
        if Wt == 2:
            CASES[f"c9-c1{W}"] = functools.partial(_ring_case, pattern=pat, Wt=Wt, long_spans=True,
                                                   events=("anchor", "advance", "wrap"))
    # advances of Wt - 1, Wt, Wt + 1, then 1 and 2 (a wrap after the jumps)
    pat = [(lambda j, k=k: k + j % 3) for k in (0, 2, 5, 9, 10, 12)]
    adv = [("anchor", 0, 0), ("advance", 1, 2), ("advance", 2, 3), ("jump", 2),
           ("advance", 3, 4), ("jump", 3), ("advance", 4, 1), ("advance", 5, 2), ("wrap", 5)]
    CASES[f"c2{W}"] = functools.partial(_ring_case, pattern=pat, Wt=3, first=adv,
                                        events=("advance", "jump", "wrap"))
    CASES[f"c9-c2{W}"] = functools.partial(_ring_case, pattern=pat, Wt=3, first=adv,
                                           long_spans=True, events=("advance", "jump", "wrap"))
    # batches without a window between anchored batches, and before the anchor
    CASES[f"c3-mid{W}"] = functools.partial(
        _ring_case, pattern=[2, None, None, None, lambda j: 5 + j % 2, 6], Wt=2,
        first=[("anchor", 0, 2), ("no_window_batch", 1), ("no_window_batch", 2),
               ("no_window_batch", 3), ("advance", 4, 3), ("jump", 4), ("advance", 5, 1)],
        events=("no_window_batch",))
    CASES[f"c3-head{W}"] = functools.partial(
        _ring_case, pattern=[None, None, 3, lambda j: 4 + j % 2], Wt=2,
        first=[("no_window_batch", 0), ("no_window_batch", 1), ("anchor", 2, 3),
               ("advance", 3, 1)], events=("no_window_batch",))
    # a batch whose minimum is below base: spans below base and inside the tile
    CASES[f"c4{W}"] = functools.partial(
        _ring_case, pattern=[lambda j: 4 + j % 3,
                             lambda j: np.where(j % 5 == 0, 2, np.where(j % 5 == 1, 3, 4 + j % 3)),
                             lambda j: 6 + j % 2], Wt=3,
        first=[("anchor", 0, 4), ("backward", 1), ("straddle", 1), ("advance", 2, 2)],
        events=("backward", "straddle"))
    # one batch over windows base .. base + Wt + 1
    CASES[f"c5{W}"] = functools.partial(
        _ring_case, pattern=[2, lambda j: 2 + j % 5], Wt=3,
        first=[("anchor", 0, 2), ("straddle", 1)], events=("straddle",))
    # the tile at the end of the range
    CASES[f"c6-cut{W}"] = functools.partial(
        _ring_case, pattern=[lambda j: 3 + j % 2, 7], Wt=3, T=8,
        first=[("anchor", 0, 3), ("advance", 1, 4), ("jump", 1), ("finish_cut", 1)],
        events=("finish_cut",))
    CASES[f"c6-T=1{W}"] = functools.partial(_ring_case, pattern=[0, 0], Wt=3, T=1,
                                            first=[("anchor", 0, 0)])
    CASES[f"c6-T=2{W}"] = functools.partial(_ring_case, pattern=[lambda j: j % 2, 1], Wt=3, T=2,
                                            first=[("anchor", 0, 0), ("advance", 1, 1),
                                                   ("finish_cut", 1)], events=("finish_cut",))
    # the batch minimum held by one span only
    for label, x in (("lane0", 0), ("last", B_WIDE - 1), ("fourth-keys", 1024 + 11),
                     ("fourth-rows", 23)):
        CASES[f"c7-{label}{W}"] = functools.partial(
            _ring_case, pattern=[1, lambda j, x=x: np.where(j == x, 3, 4), 4], Wt=2,
            first=[("anchor", 0, 1), ("advance", 1, 2), ("jump", 1), ("advance", 2, 1)])


MIN_HOLDER = {"c7-lane0": (0, 0, 0), "c7-last": (511, 3, 3), "c7-fourth-keys": (5, 3, None),
              "c7-fourth-rows": (None, None, 3)}   # (tid, j in the keys form, j in the rows form)


# ---- d: cell borders of the sorted keys (the 1024-span batch, quantiles only)
D_M = 5 * B_CELL + 300
D_BORDERS = (1, 128, 512, 640, 1024, 1280, 2048, 3072, 4096, 5120, D_M - 1)


def _cells_case(name, cum, cap, m=D_M, T=8, sentinel_at=None, begin=0):
    """One-span root traces whose cells (window, service), in sorted order, end
    at the cumulative counts `cum`; from sentinel_at on, spans outside the
    window range."""
    rng = _rng(name)
    cum = [x for x in cum if sentinel_at is None or x < sentinel_at]
    edges = [0] + list(cum) + [m if sentinel_at is None else sentinel_at]
    cell = np.repeat(np.arange(len(edges) - 1), np.diff(edges))
    assert len(edges) - 1 <= 2 * T
    win = np.concatenate([cell // 2, np.full(m - len(cell), -1)])
    svc = np.concatenate([cell % 2, rng.integers(0, 2, m - len(cell))])
    perm = rng.permutation(m)
    win, svc = win[perm], svc[perm]
    if begin:      # a dead head in front: the sort reads keys + begin
        win, svc = np.r_[np.zeros(begin, np.int64), win], np.r_[np.zeros(begin, np.int64), svc]
    sp = _build(name, win, begin, T=T, singles=True, svc=svc)
    exp = {"quantiles": dict(bounds=_geom(m, B_CELL, cap), borders=list(cum),
                             sentinel=sentinel_at)}
    return Case(name, sp, B_CELL, T, cap, None, ("quantiles",), expect=exp)


def _register_cells():
    Q = f"@{B_CELL}"
    for cap in (2, 3):
        CASES[f"d1-cap={cap}{Q}"] = functools.partial(_cells_case, cum=D_BORDERS, cap=cap)
    CASES[f"d1-begin=3{Q}"] = functools.partial(_cells_case, cum=D_BORDERS, cap=3, begin=3)
    CASES[f"d2{Q}"] = functools.partial(_cells_case, cum=(), cap=2, m=2 * B_CELL + 7)
    m3 = 2 * B_CELL + 7
    CASES[f"d3{Q}"] = functools.partial(_cells_case, cum=tuple(range(1, m3)), cap=2, m=m3,
                                        T=(m3 + 1) // 2)
    for x in D_BORDERS:
        CASES[f"d4-at={x}{Q}"] = functools.partial(_cells_case, cum=D_BORDERS,
                                                   cap=2 if x == 3072 else 3, sentinel_at=x)


# ---- e: exemplars across workgroups (the 2048-span batch, cap 3)
E_N = 4 * B_WIDE + B_WIDE // 2        # ranges [0, 2B), [2B, 4B), [4B, 4.5B)
E_KS = (1, 3, 64)
E_PLACES = ("lds", "global", "cached")


def _ex_case(name, shape):
    rng = _rng(name)
    begin = 5 if shape == "begin" else 0
    B, n, S = B_WIDE, E_N + begin, 2
    dur = rng.integers(1, 40, n)
    flags = svc = None
    errors_only = False
    marks = None
    if shape == "equal":                     # position decides
        dur = np.full(n, 25)
    elif shape == "range_borders":           # error winners at the range borders
        marks = [2 * B - 1, 2 * B, 4 * B]
        flags = np.where(rng.random(n) < 0.01, ERR, 0)
        flags[marks] = ERR
        dur[marks] = (1000, 999, 998)
        errors_only = True
    elif shape == "few":                     # K above an edge's span count
        S = 3
        svc = rng.integers(0, 2, n)
        svc[rng.choice(n, 12, replace=False)] = 2
    sp = _build(name, _ordered(n, 16), begin, T=16, S=S, dur=dur, flags=flags, svc=svc)
    if shape == "split":                     # one edge's slowest over all three ranges
        rows = native.span_edges(sp, S).astype(np.int64)
        r = int(np.bincount(rows).argmax())
        where = np.nonzero(rows == r)[0]
        marks = [int(where[np.searchsorted(where, x)]) for x in
                 (7, B, 2 * B - 40, 2 * B + 3, 3 * B + 1, 4 * B - 9, 4 * B + 2, 4 * B + 700)]
        sp.dur_us[marks] = 5000 + np.arange(len(marks), dtype=np.uint32) * 7 % 5
    exp = {"exemplars": dict(_geom(n, B, 3), marks=marks)}
    return Case(name, sp, B, 16, 3, None, ("exemplars",), expect=exp, ks=E_KS, places=E_PLACES,
                errors_only=errors_only)


def _register_exemplars():
    W = f"@{B_WIDE}"
    for label, shape in (("e1", "equal"), ("e2", "range_borders"), ("e3", "split"),
                         ("e4", "few"), ("e5", "begin")):
        CASES[f"{label}{W}"] = functools.partial(_ex_case, shape=shape)


_register()
_register_ring()
_register_cells()
_register_exemplars()


def case_names():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return CASES[name](name)

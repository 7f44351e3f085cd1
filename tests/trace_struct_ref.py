"""Reference for the trace-structure kernels (a plain helper, not a conftest):
an independent model of anomod_trace_structure in plain Python / numpy and
the input builders the host and GPU tests share.

Model (trace_structure_ref), per trace, from the header text of
csrc/trace_struct.hip and include/anomod.h:

  first / last   dicts id -> first / last position of the id in the trace
  pf[i]          first[parent reference of span i], none when the reference is
                 0 or names no span of the trace
  node parent    of span i: pf[last[id_i]] (the LAST span's reference)
  n_children     of a node: the spans whose pf names it, copied to every span
                 carrying the id
  flags          ROOT when the node parent is none, FIRST when first[id_i] == i
  n_roots        nodes with ROOT
  depth          graph definition, no iteration to a fixpoint: edges
                 pf[i] -> first[id_i]; the nodes reachable from the roots;
                 Kahn's topological order on that subgraph; a node the order
                 finishes gets its longest path from a root, a node it never
                 finishes sits on or after a reached cycle and gets 0, as does
                 every unreachable node
  svc_mask       [n_traces, ceil(S / 64)] u64 bit set of the service indices

O(L) per trace: two dict passes, one stack walk, one queue walk.  Nothing
here scans a trace per span, relaxes edges until nothing changes or jumps
pointers, which is what the C oracle and the kernels do.

Builders.  case_names() lists "<shape>-<regime>" names and case(name) builds
(and caches) the span set with the facts the builder claims about it; the
host test asserts those facts against the model, so a case cannot silently
stop reaching the path it was written for.  Regimes:

  U     ids unique within every trace, declared (unique_ids=True): the
        declared-unique kernel
  G     the same spans undeclared: the general scan, then pointer jumping
  Din   the same spans plus a twin of one span (same id, same parent
        reference, appended to the trace under test): a duplicated id, so the
        chunk (or the long trace) takes the longest-path relaxation; the twin
        changes no depth
  Dout  the same spans plus a two-span trace holding one id twice right before
        the trace under test, in the same chunk (only where the shape + 2
        spans still fit one chunk)
  D     shapes that need a duplicated id by construction

Where the traces run.  trace_struct_kernel gives the first nt - nt // 2
traces to its waves in equal static shares (thousands of waves: in a small
set every such trace is a run, and so a chunk, of its own) and hands out the
last nt // 2 in segments of DYN_SEG = 512 consecutive traces; only a run of
several traces is packed into chunks (tail_chunks restates that packing).  So
case() puts as many one-span filler traces in front of a shape's traces as
the shape has: the shape is then exactly the dynamic tail, walked as one run
from its first trace, and its traces share chunks as the builder intends
(the host test asserts the chunks).  many_long (about its long traces, each a
chunk of its own) and pack_only_empty (no span at all) get no fillers.

Kernel constants restated here (csrc/chunk.h, csrc/trace_struct.hip): a chunk
stages STAGE = 256 spans of at most 64 traces; a longer trace goes to the
workgroup-per-trace kernel, which looks ids up BIG_BLOCK = 4096 spans at a
time against table windows of BIG_WIN = 4096 ids in BIG_SLOTS = 8192 slots
(multiply-shift hash, linear probing)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import anomod

NO_PARENT = 0xFFFFFFFF
SPAN_ROOT, SPAN_FIRST = 1, 2
FIELDS = ("parent_pos", "depth", "n_children", "span_flags", "n_roots", "svc_mask")

STAGE = 256         # chunk.h kStage
CHUNK_TRACES = 64   # chunk.h kWave: traces per chunk
BIG_WIN = 4096      # trace_struct.hip kBigWin
BIG_BLOCK = 4096    # trace_struct.hip kBigThreads * kBigPer
BIG_SLOTS = 8192    # trace_struct.hip kBigSlots
DYN_SEG = 512       # trace_struct.hip kDynSeg: traces per segment of the dynamic tail
MI355X_CUS = 256


# ------------------------------------------------------------------ the model
def _trace_nodes(sid, pid):
    """first-position of every span's node, pf, node parent (lists; -1 = none)."""
    first, last = {}, {}
    for i, x in enumerate(sid):
        if x not in first:
            first[x] = i
        last[x] = i
    pf = [first.get(p, -1) if p else -1 for p in pid]
    node = [first[x] for x in sid]
    npar = [pf[last[x]] for x in sid]
    return node, pf, npar


def _reach(L, node, pf, npar):
    """(out-edge lists per node, reachable flags) from the root nodes."""
    out = [[] for _ in range(L)]
    for i in range(L):
        if pf[i] >= 0:
            out[pf[i]].append(node[i])
    seen = [False] * L
    stack = [i for i in range(L) if node[i] == i and npar[i] < 0]
    for r in stack:
        seen[r] = True
    while stack:
        u = stack.pop()
        for v in out[u]:
            if not seen[v]:
                seen[v] = True
                stack.append(v)
    return out, seen


def reachable_positions(sid, pid):
    """Positions of the spans whose node a root reaches (for builder premises)."""
    sid, pid = [int(x) for x in sid], [int(x) for x in pid]
    node, pf, npar = _trace_nodes(sid, pid)
    _, seen = _reach(len(sid), node, pf, npar)
    return [i for i in range(len(sid)) if seen[node[i]]]


def _trace_ref(sid, pid):
    L = len(sid)
    node, pf, npar = _trace_nodes(sid, pid)
    cnt = [0] * L
    for p in pf:
        if p >= 0:
            cnt[p] += 1
    out, seen = _reach(L, node, pf, npar)
    indeg = [0] * L
    for u in range(L):
        if seen[u]:
            for v in out[u]:
                indeg[v] += 1
    # Kahn: a reachable node without a reachable in-edge is a root
    dist = [0 if (seen[v] and node[v] == v and npar[v] < 0) else -1 for v in range(L)]
    queue = [v for v in range(L) if seen[v] and indeg[v] == 0]
    done = [False] * L
    while queue:
        u = queue.pop()
        done[u] = True
        for v in out[u]:
            if dist[u] + 1 > dist[v]:
                dist[v] = dist[u] + 1
            indeg[v] -= 1
            if indeg[v] == 0:
                queue.append(v)
    depth = [dist[node[i]] if done[node[i]] else 0 for i in range(L)]
    ppos = [p if p >= 0 else NO_PARENT for p in npar]
    flags = [(SPAN_ROOT if npar[i] < 0 else 0) | (SPAN_FIRST if node[i] == i else 0)
             for i in range(L)]
    nch = [cnt[node[i]] for i in range(L)]
    return ppos, depth, nch, flags, sum(1 for f in flags if f == (SPAN_ROOT | SPAN_FIRST))


def trace_structure_ref(sp, S=None) -> dict:
    """The six outputs of anomod_trace_structure for a SpanSet-like object."""
    S = len(sp.services) if S is None else S
    words = (S + 63) // 64
    n, nt = sp.n_spans, sp.n_traces
    ptr = sp.trace_ptr.astype(np.int64).tolist()
    sid, pid = sp.span_id.tolist(), sp.parent_span_id.tolist()
    ppos, depth, nch, flags, roots = [], [], [], [], []
    for t in range(nt):
        a, b = ptr[t], ptr[t + 1]
        r = _trace_ref(sid[a:b], pid[a:b])
        ppos += r[0]
        depth += r[1]
        nch += r[2]
        flags += r[3]
        roots.append(r[4])
    mask = np.zeros((nt, words), np.uint64)
    svc = sp.svc.astype(np.int64)
    t_of = np.repeat(np.arange(nt, dtype=np.int64), np.diff(sp.trace_ptr).astype(np.int64))
    np.bitwise_or.at(mask, (t_of, svc >> 6), np.uint64(1) << (svc & 63).astype(np.uint64))
    assert len(ppos) == n
    return {"parent_pos": np.array(ppos, np.uint32).reshape(n),
            "depth": np.array(depth, np.uint32).reshape(n),
            "n_children": np.array(nch, np.uint32).reshape(n),
            "span_flags": np.array(flags, np.uint8).reshape(n),
            "n_roots": np.array(roots, np.uint32).reshape(nt), "svc_mask": mask}


def big_slot(ids) -> np.ndarray:
    """trace_struct.hip big_slot: the top 13 bits of id * 0x9E3779B97F4A7C15
    (mod 2^64)."""
    ids = np.asarray(ids, np.uint64)
    with np.errstate(over="ignore"):
        h = ids * np.uint64(0x9E3779B97F4A7C15)
    return ((h >> np.uint64(64 - 13)) & np.uint64(BIG_SLOTS - 1)).astype(np.int64)


def tail_chunks(lens, start=None) -> list:
    """(first trace, k, n) of every chunk the device forms over the dynamic
    tail of a set with these trace lengths: the last nt // 2 traces (or, for
    another driver of the same chunk walk, the traces from `start` on) in
    segments of DYN_SEG, each walked from its start in chunks of the most
    leading traces (up to CHUNK_TRACES) that hold <= STAGE spans together
    (chunk.h make_chunk); k = 0 is a trace longer than STAGE on its own."""
    nt = len(lens)
    out = []
    for s in range(nt - nt // 2 if start is None else start, nt, DYN_SEG):
        e, t = min(s + DYN_SEG, nt), s
        while t < e:
            k = n = 0
            while t + k < e and k < CHUNK_TRACES and n + lens[t + k] <= STAGE:
                n += lens[t + k]
                k += 1
            out.append((t, k, n if k else lens[t]))
            t += max(k, 1)
    return out


# ------------------------------------------------------------------ shapes
@dataclass
class Shape:
    """Traces as (ids, parent references[, services]) with unique ids unless
    dup is set; `target` is the trace under test and the facts are about it
    (positions are trace-local and survive the regimes: the twin is appended)."""

    traces: list
    target: int = 0
    S: int = 3
    dup: bool = False          # holds a duplicated id by construction (regime D only)
    facts: dict = field(default_factory=dict)


@dataclass
class Case:
    name: str
    sp: anomod.SpanSet
    target: int
    regime: str
    facts: dict
    first: int = 0             # the shape's first trace (after the fillers)

    @functools.cached_property
    def model(self) -> dict:
        return trace_structure_ref(self.sp)

    def target_slice(self) -> slice:
        return slice(int(self.sp.trace_ptr[self.target]), int(self.sp.trace_ptr[self.target + 1]))


def _ids(seed, n) -> np.ndarray:
    """n distinct random non-zero u64 ids."""
    rng = np.random.default_rng(seed)
    while True:
        x = rng.integers(1, 2**64, n, dtype=np.uint64)
        if np.unique(x).shape[0] == n:
            return x


def _chain_pid(sid, order) -> np.ndarray:
    """Parent references of a chain visiting the positions in `order`."""
    pid = np.zeros(len(sid), np.uint64)
    pid[order[1:]] = sid[order[:-1]]
    return pid


def _order(kind, L, seed=0) -> np.ndarray:
    if kind == "fwd":
        return np.arange(L)
    if kind == "rev":
        return np.arange(L)[::-1].copy()
    return np.random.default_rng(1000 + seed + L).permutation(L)


def make_set(traces, S, unique_ids) -> anomod.SpanSet:
    lens = [len(t[0]) for t in traces]
    ptr = np.zeros(len(traces) + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    n = int(ptr[-1])
    cat = lambda k, dt: (np.concatenate([np.asarray(t[k], dt) for t in traces])  # noqa: E731
                         if traces else np.zeros(0, dt))
    sid, pid = cat(0, np.uint64), cat(1, np.uint64)
    svcs = [np.asarray(t[2], np.uint16) if len(t) > 2 else
            ((np.arange(len(t[0])) + k) % S).astype(np.uint16) for k, t in enumerate(traces)]
    svc = np.concatenate(svcs) if svcs else np.zeros(0, np.uint16)
    # one hash per trace (the ungrouped upload knows a span's trace by it alone)
    th = np.repeat(_ids(77, len(traces)) if traces else np.zeros(0, np.uint64), lens)
    assert not (sid == 0).any(), "span id 0 is reserved by the ABI"
    return anomod.SpanSet([f"s{i:04d}" for i in range(S)], ptr, th, sid, pid, svc,
                          np.zeros(n, np.uint16), np.ones(n, np.uint32), unique_ids=unique_ids)


# -- chains
CHUNK_LENS = (1, 2, 127, 128, 129, 255, 256)
LONG_LENS = (257, 4095, 4096, 4097, 8193)


def _chain(kind, L):
    sid = _ids(L, L)
    order = _order(kind, L)
    depth = np.empty(L, np.int64)
    depth[order] = np.arange(L)
    return Shape([(sid, _chain_pid(sid, order))],
                 facts={"max_depth": L - 1, "n_roots": 1, "depth": depth})


# -- chunk packing
def _small_chains(seed, lens):
    traces = []
    for k, L in enumerate(lens):
        sid = _ids(seed * 1000 + k, L)
        traces.append((sid, _chain_pid(sid, _order("fwd" if k % 2 else "rev", L))))
    return traces


def _pack(n_traces):
    """n_traces chains of 4 spans.  Every trace carries the same four ids
    (unique within a trace is all the ABI asks), rotated and in alternating
    chain order, so a lookup that left its trace would find a wrong span."""
    ids = _ids(3, 4)
    traces = []
    for k in range(n_traces):
        sid = np.roll(ids, k)
        traces.append((sid, _chain_pid(sid, _order("fwd" if k % 2 else "rev", 4))))
    chunks = [(CHUNK_TRACES, STAGE)] + ([(n_traces - CHUNK_TRACES, 4 * (n_traces - CHUNK_TRACES))]
                                        if n_traces > CHUNK_TRACES else [])
    return Shape(traces, target=n_traces - 1,
                 facts={"max_depth": 3, "n_roots": 1, "chunks": chunks})


def _pack_chain_then_one():
    sid = _ids(5, STAGE)
    one = _ids(6, 1)
    return Shape([(sid, _chain_pid(sid, _order("fwd", STAGE))), (one, np.zeros(1, np.uint64))],
                 target=1, facts={"max_depth": 0, "n_roots": 1, "chunks": [(1, STAGE), (1, 1)]})


def _pack_empty(S):
    # empty traces at the start, in the middle (two in a row) and at the end
    lens = [0, 5, 0, 0, 7, 3, 0]
    return Shape(_small_chains(7, lens), target=4, S=S,
                 facts={"max_depth": 6, "n_roots": 1, "empty_traces": 4, "chunks": [(7, 15)]})


def _only_empty():
    return Shape(_small_chains(8, [0] * 5), target=4, facts={"set_spans": 0})


# -- cycles no root reaches
def _self_parent():
    sid = _ids(11, 6)
    pid = _chain_pid(sid, np.arange(3))  # 0 -> 1 -> 2, then 3 its own parent, 4 under 3
    pid[3], pid[4], pid[5] = sid[3], sid[3], sid[2]
    return Shape([(sid, pid)], facts={"n_roots": 1, "max_depth": 3, "zero": [3, 4],
                                      "depth": np.array([0, 1, 2, 0, 0, 3])})


def _two_cycle():
    sid = _ids(12, 7)
    pid = np.zeros(7, np.uint64)
    pid[1], pid[2] = sid[0], sid[1]      # a tree 0 -> 1 -> 2
    pid[3], pid[4] = sid[4], sid[3]      # 3 <-> 4
    pid[5], pid[6] = sid[4], sid[0]      # 5 hangs off the cycle, 6 off the root
    return Shape([(sid, pid)], facts={"n_roots": 1, "max_depth": 2, "zero": [3, 4, 5],
                                      "depth": np.array([0, 1, 2, 0, 0, 0, 1])})


def _whole_cycle(L, kind):
    sid = _ids(13 + L, L)
    order = _order(kind, L)
    pid = _chain_pid(sid, order)
    pid[order[0]] = sid[order[-1]]
    return Shape([(sid, pid)], facts={"n_roots": 0, "max_depth": 0, "zero": list(range(L))})


def _cycle_beside_tree():
    sid = _ids(14, 18)
    pid = np.zeros(18, np.uint64)
    for i in range(1, 10):               # a tree on 0..9: two branches off the root
        pid[i] = sid[0] if i in (1, 2) else sid[i - 2]
    for i in range(10, 15):              # a cycle on 10..14, referenced forward
        pid[i] = sid[10 + (i - 10 + 1) % 5]
    pid[15], pid[16], pid[17] = sid[12], sid[15], sid[16]  # a tail off the cycle
    return Shape([(sid, pid)], facts={"n_roots": 1, "max_depth": 5,
                                      "zero": list(range(10, 18))})


# -- cycles a root reaches (need a duplicated id: the entry node's two spans)
def _reached_cycle(a, c, b, chain_first):
    """A root chain of a spans, a cycle of c nodes, a tail of b spans off the
    cycle.  The entry node carries two spans, one under the chain's end and
    one under the cycle's last node, at positions a and a + c; chain_first
    says which of the two comes first (the later one names the node parent)."""
    L = a + c + b + 1
    ids = _ids(15 + L + a, a + c + b)
    chain, cyc, tail = ids[:a], ids[a:a + c], ids[a + c:]
    sid, pid = np.zeros(L, np.uint64), np.zeros(L, np.uint64)
    sid[:a] = chain
    pid[1:a] = chain[:-1]
    e_chain, e_cyc = (a, a + c) if chain_first else (a + c, a)
    sid[a] = sid[a + c] = cyc[0]
    pid[e_chain], pid[e_cyc] = chain[-1], cyc[-1]
    sid[a + 1:a + c] = cyc[1:]
    pid[a + 1:a + c] = cyc[:-1]
    sid[a + c + 1:] = tail
    pid[a + c + 1:] = np.r_[cyc[-1:], tail[:-1]]
    depth = np.zeros(L, np.int64)
    depth[:a] = np.arange(a)
    return Shape([(sid, pid)], dup=True,
                 facts={"n_roots": 1, "max_depth": a - 1, "depth": depth, "len": L,
                        "zero": list(range(a, L)), "reached": list(range(L)),
                        "entry_parent": a - 1 if not chain_first else (a + c - 1 if c > 1 else a)})


def _reached_sizes(L):
    third = (L - 1) // 3
    return ((third, third, L - 1 - 2 * third), (L - 6, 2, 3), (2, 2, L - 5))


def _root_on_cycle(root_last):
    """Node R carries a span without a parent and a span under X, and X sits
    under R.  With the parentless span last R is a root on the cycle R -> X ->
    R that it reaches itself (every depth on it 0); with the other span last R
    is no root and nothing reaches the cycle.  A chain 0 -> 1 -> 2 beside it."""
    ids = _ids(16, 5)
    r, x = ids[3], ids[4]
    sid = np.r_[ids[:3], r, x, r]
    pid = np.r_[np.uint64(0), ids[:2], np.uint64(0), r, x]
    if root_last:
        pid[3], pid[5] = x, np.uint64(0)
    return Shape([(sid, pid)], dup=True,
                 facts={"n_roots": 2 if root_last else 1, "max_depth": 2, "zero": [3, 4, 5],
                        "depth": np.array([0, 1, 2, 0, 0, 0])})


# -- deepest visit
def _diamond(k, fill, shallow_first):
    """Root 0, a deep path 1..k under it, node N with a span under the root and
    a span under the path's end, M under N, then `fill` spans under M's chain."""
    ids = _ids(17 + k, k + 3 + fill)
    root, path, nid, mid, rest = ids[0], ids[1:k + 1], ids[k + 1], ids[k + 2], ids[k + 3:]
    sh, dp = (root, path[-1]) if shallow_first else (path[-1], root)
    sid = np.r_[root, nid, path, nid, mid, rest]
    pid = np.r_[np.uint64(0), sh, root, path[:-1], dp, nid, np.r_[mid, rest][:fill]]
    L = len(sid)
    depth = np.r_[0, k + 1, np.arange(1, k + 1), k + 1, k + 2, k + 3 + np.arange(fill)]
    return Shape([(sid, pid)], dup=True,
                 facts={"n_roots": 1, "max_depth": int(depth.max()), "depth": depth, "len": L})


# -- long-trace lookups
def _tree_8193(seed):
    L = 8193
    sid = _ids(seed, L)
    rng = np.random.default_rng(seed)
    par = (rng.random(L) * np.maximum(np.arange(L), 1)).astype(np.int64)
    pid = sid[par].copy()
    pid[0] = 0
    return sid, pid, par


def _dup_across_windows(p, q):
    """One id at positions p < q of an 8193-span tree, in different table
    windows, each span under another parent, and two spans under the id."""
    sid, pid, par = _tree_8193(18 + p)
    sid[q] = sid[p]
    far = 7000 if q != 7000 else 7001
    for i in (p + 5, far):  # references to the duplicated id from both sides of it
        pid[i] = sid[p]
    assert par[p] != par[q] and par[q] != p and p // BIG_WIN != q // BIG_WIN
    # the node's parent is the LAST span's: position q's reference
    return Shape([(sid, pid)], dup=True,
                 facts={"windows": [(int(sid[p]), [p, q])],
                        "parent_at": {p: int(par[q]), q: int(par[q])}})


def _cross_window_parents():
    """8193 spans: position 6000 (window 1) is the only span under position
    100 (window 0); position 50 (window 0) sits under position 8192 (window
    2), a second root."""
    sid, pid, par = _tree_8193(19)
    pid[par == 100] = sid[99]
    pid[100] = sid[99]
    pid[6000] = sid[100]
    pid[8192] = 0
    pid[50] = sid[8192]
    return Shape([(sid, pid)], facts={"n_roots": 2, "parent_at": {6000: 100, 50: 8192},
                                      "children_at": {100: 1}})


def _collision_cluster():
    """A 600-span trace in which a cluster of ids hashes to table slot 8191,
    so their probes wrap to slot 0 and displace the ids that hash there; the
    chain runs through the cluster (every lookup of it is a parent lookup)."""
    draw = np.random.default_rng(20).integers(1, 2**64, 1 << 20, dtype=np.uint64)
    draw = np.unique(draw)
    slot = big_slot(draw)
    cluster = draw[slot == BIG_SLOTS - 1][:48]
    # should the hash constant change, the case only loses sharpness: say so
    assert len(cluster) >= 40, "the fixed draw no longer fills one table slot"
    front = draw[slot < 40][:40]        # ids at home where the cluster spills
    rest = draw[(slot >= 40) & (slot < BIG_SLOTS - 1)][:600 - len(cluster) - len(front)]
    sid = np.concatenate([rest[:100], cluster, front, rest[100:]])
    order = _order("shuf", len(sid), seed=20)
    depth = np.empty(len(sid), np.int64)
    depth[order] = np.arange(len(sid))
    return Shape([(sid, _chain_pid(sid, order))],
                 facts={"cluster": (BIG_SLOTS - 1, int(len(cluster))), "n_roots": 1,
                        "max_depth": len(sid) - 1, "depth": depth})


def _low_word_twins(L):
    sid = _ids(21 + L, L)
    sid[7] = sid[3] ^ np.uint64(1 << 40)
    order = _order("shuf", L, seed=21)
    return Shape([(sid, _chain_pid(sid, order))],
                 facts={"n_roots": 1, "max_depth": L - 1, "low_twins": (3, 7)})


# -- many long traces
def _many_long(n_cus):
    """More long traces than twice the workgroups of one launch (one per CU),
    so every workgroup takes several tickets and reuses its table.  Lengths
    run through 257..300, every trace differing from its neighbours (the range
    holds 44 lengths, fewer than the traces); a 3-span trace after every
    seventh; a long trace last (the dynamic tail of the chunk walk).  Every
    long trace names two of five services, another pair than its neighbours,
    so a service word kept from a workgroup's previous trace would show."""
    n_long = 2 * n_cus + 88
    traces = []
    for j in range(n_long):
        L = 257 + (j * 13) % 44
        sid = _ids(30000 + j, L)
        svc = np.where(np.arange(L) % 9 == 0, (j * 3 + 1) % 5, j % 5).astype(np.uint16)
        traces.append((sid, _chain_pid(sid, _order(("fwd", "rev", "shuf")[j % 3], L, seed=j)),
                       svc))
        if j % 7 == 6 and j != n_long - 1:
            s3 = _ids(60000 + j, 3)
            traces.append((s3, _chain_pid(s3, np.arange(3))))
    return Shape(traces, target=len(traces) - 1, S=5,
                 facts={"long_traces": n_long, "n_roots": 1,
                        "max_depth": len(traces[-1][0]) - 1})


# -- services
def _svc_indices(S):
    return sorted({i for i in (0, 63, 64, S - 1) if i < S})


def _services(S, layout):
    idx = _svc_indices(S)
    lens = {"chunk": [6, 9, 5, 8], "empty": [6, 0, 9, 0, 5], "long": [300, 7]}[layout]
    chunks = {"chunk": [(4, 28)], "empty": [(5, 20)], "long": [(0, 300), (1, 7)]}[layout]
    traces = []
    for sid, pid in _small_chains(40 + S, lens):
        L = len(sid)
        # every trace with spans leaves another of the indices out (where there
        # are several), so the masks of neighbouring traces differ
        k = sum(1 for t in traces if len(t[0]))
        use = [v for j, v in enumerate(idx) if len(idx) == 1 or j != k % len(idx)]
        traces.append((sid, pid, np.array([use[i % len(use)] for i in range(L)], np.uint16)))
    return Shape(traces, target=0, S=S, facts={"svc_present": idx, "chunks": chunks})


# -- unknown max_trace_len (ungrouped upload, grouped on the device)
def _ungrouped():
    lens = [5, 4097, 0, 9, 256, 3]
    traces = _small_chains(50, lens)
    return Shape(traces, target=1, facts={"max_depth": 4096, "n_roots": 1})


def _shapes() -> dict:
    s = {}
    for kind in ("fwd", "rev", "shuf"):
        for L in CHUNK_LENS + LONG_LENS:
            s[f"chain_{kind}_{L}"] = functools.partial(_chain, kind, L)
    s["pack_64x4"] = functools.partial(_pack, 64)
    s["pack_65x4"] = functools.partial(_pack, 65)
    s["pack_chain256_then_1"] = _pack_chain_then_one
    s["pack_empty_w1"] = functools.partial(_pack_empty, 3)
    s["pack_empty_w2"] = functools.partial(_pack_empty, 70)
    s["pack_only_empty"] = _only_empty
    s["cycle_self_parent"] = _self_parent
    s["cycle_two"] = _two_cycle
    for L, kind in ((6, "fwd"), (256, "rev"), (256, "shuf"), (300, "shuf")):
        s[f"cycle_whole_{kind}_{L}"] = functools.partial(_whole_cycle, L, kind)
    s["cycle_beside_tree"] = _cycle_beside_tree
    for L in (256, 257, 4097, 8193):
        for a, c, b in (_reached_sizes(L) if L != 8193 else _reached_sizes(L)[:1]):
            for first in ("chain", "cycle"):
                s[f"reached_{L}_a{a}_c{c}_b{b}_{first}first"] = functools.partial(
                    _reached_cycle, a, c, b, first == "chain")
    s["root_on_cycle_rootlast"] = functools.partial(_root_on_cycle, True)
    s["root_on_cycle_rootfirst"] = functools.partial(_root_on_cycle, False)
    for where, k, fill in (("chunk", 5, 3), ("300", 290, 6)):
        for first in ("shallow", "deep"):
            s[f"diamond_{where}_{first}first"] = functools.partial(_diamond, k, fill,
                                                                   first == "shallow")
    s["lookup_dup_5_4100"] = functools.partial(_dup_across_windows, 5, 4100)
    s["lookup_dup_4100_8192"] = functools.partial(_dup_across_windows, 4100, 8192)
    s["lookup_cross_window_parents"] = _cross_window_parents
    s["lookup_collision_cluster"] = _collision_cluster
    s["lookup_low_word_twins_10"] = functools.partial(_low_word_twins, 10)
    s["lookup_low_word_twins_300"] = functools.partial(_low_word_twins, 300)
    s["many_long"] = None  # built per CU count, see case()
    for S in (1, 64, 65, 128, 4096):
        for layout in ("chunk", "empty", "long"):
            s[f"services_S{S}_{layout}"] = functools.partial(_services, S, layout)
    s["ungrouped_4097"] = _ungrouped
    return s


SHAPES = _shapes()
# shapes whose ids repeat by construction: regime D only
_DUP_PREFIXES = ("reached_", "root_on_cycle_", "diamond_", "lookup_dup_")


def _regimes(shape_name) -> tuple:
    if shape_name.startswith(_DUP_PREFIXES):
        return ("D",)
    if shape_name == "pack_only_empty":
        return ("U", "G")
    return ("U", "G", "Din", "Dout")


def _fits_dout(shape: Shape) -> bool:
    n = sum(len(t[0]) for t in shape.traces)
    return n + 2 <= STAGE and len(shape.traces) + 1 <= CHUNK_TRACES


@functools.lru_cache(maxsize=None)
def _shape(shape_name, n_cus) -> Shape:
    if shape_name == "many_long":
        return _many_long(n_cus)
    return SHAPES[shape_name]()


@functools.lru_cache(maxsize=None)
def case(name, n_cus=MI355X_CUS):
    """The case "<shape>-<regime>", or None where the regime does not apply to
    the shape (Dout on a shape that fills its chunk)."""
    shape_name, regime = name.rsplit("-", 1)
    sh = _shape(shape_name, n_cus)
    traces, target = list(sh.traces), sh.target
    if regime == "D":
        assert sh.dup
    else:
        assert not sh.dup
    if regime == "Din":
        every = 2 if shape_name == "many_long" else len(traces) + 1  # many_long: every other trace
        for t in range(target % every, len(traces), every):
            tr = traces[t]
            m = len(tr[0]) // 2
            traces[t] = tuple(np.r_[col, col[m:m + 1]] for col in tr)
    elif regime == "Dout":
        if not _fits_dout(sh):
            return None
        x = _ids(99, 1)
        extra = (np.r_[x, x], np.zeros(2, np.uint64))
        if len(traces[target]) > 2:  # explicit services: add no new one
            extra += (traces[target][2][:1].repeat(2),)
        traces.insert(target, extra)
        target += 1
    first = 0
    if shape_name not in ("many_long", "pack_only_empty"):
        # as many one-span traces in front as the shape has: the shape becomes
        # the dynamic tail, one run (see the module text)
        first = len(traces)
        assert first <= DYN_SEG
        fill = [(x, np.zeros(1, np.uint64)) for x in _ids(555, first).reshape(first, 1)]
        explicit = [t[2] for t in traces if len(t) > 2 and len(t[0])]
        if explicit:  # explicit services: the fillers add no new one
            fill = [f + (explicit[0][:1],) for f in fill]
        traces = fill + traces
        target += first
    sp = make_set(traces, sh.S, unique_ids=regime == "U")
    return Case(name, sp, target, regime, dict(sh.facts), first)


def case_names() -> list:
    """Every applicable "<shape>-<regime>" (Dout decided from the shape's
    size, which does not depend on the CU count)."""
    names = []
    for shape_name in SHAPES:
        for regime in _regimes(shape_name):
            if regime == "Dout" and (shape_name == "many_long"
                                     or not _fits_dout(_shape(shape_name, MI355X_CUS))):
                continue
            names.append(f"{shape_name}-{regime}")
    return names

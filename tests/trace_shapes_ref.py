"""Exact host model of the trace shape census (a plain helper, not a conftest).

The definition of include/anomod.h (anomod_trace_shapes_spans) restated in
Python integers mod 2^64: parents from self_time_ref.parents_ref (first match
in position order), the call-path hash P by the sequential recurrence with an
explicit walk up the parent chain (a chain that never reaches a head — a
reference cycle, or a span hanging off one — is off the tree), the trace shape
as the wrapping sum of mix64(P), and the census with its order (count
descending, then value ascending).  jump_ref is the pointer-jumping form the
kernels run, in numpy u64, with the number of rounds it needed.  GPU results
are compared to this model bit for bit."""
from dataclasses import dataclass

import numpy as np

import anomod
from anomod.decode import hash64

from self_time_ref import NO_PARENT, parents_ref

M64 = (1 << 64) - 1
B = 0x9E3779B97F4A7C15
SEED_ROOT = 0x243F6A8885A308D3
SEED_ORPHAN = 0x13198A2E03707344
SEED_SELF = 0xA4093822299F31D0
ERR_KEY = 0xD1B54A32D192ED03


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def service_keys(sp, svc_key="names") -> list:
    """The label keys Context.trace_shapes passes: the hash of the names, or
    mix64(s + 1) for None, or the caller's."""
    if isinstance(svc_key, str):
        assert svc_key == "names"
        return [hash64(s) for s in sp.services]
    if svc_key is None:
        return [mix64(s + 1) for s in range(sp.n_services)]
    return [int(k) for k in svc_key]


def label_keys(sp, use_errors=False, svc_key="names") -> list:
    keys = service_keys(sp, svc_key)
    err = ((sp.flags & anomod.FLAG_ERROR) != 0).tolist()
    return [keys[s] ^ (ERR_KEY if use_errors and e else 0) for s, e in zip(sp.svc.tolist(), err)]


def head_seeds(sp, par) -> list:
    """Per span: the seed of its head kind, None for a span with a parent."""
    sid, pid = sp.span_id.tolist(), sp.parent_span_id.tolist()
    ptr = sp.trace_ptr.tolist()
    out = [None] * sp.n_spans
    plist = par.tolist()
    for t in range(sp.n_traces):
        ids = set(sid[ptr[t]:ptr[t + 1]])
        for i in range(ptr[t], ptr[t + 1]):
            if plist[i] != NO_PARENT:
                continue
            out[i] = SEED_ROOT if pid[i] == 0 else SEED_SELF if pid[i] in ids else SEED_ORPHAN
    return out


def path_hash_ref(sp, par=None, use_errors=False, svc_key="names"):
    """(P u64 [n_spans], on_tree bool [n_spans]) by the sequential definition;
    spans outside every trace read 0 / False."""
    par = parents_ref(sp) if par is None else par
    K = label_keys(sp, use_errors, svc_key)
    seed = head_seeds(sp, par)
    plist = par.tolist()
    n = sp.n_spans
    P = [0] * n
    state = [0] * n          # 0 unknown, 1 on the walk, 2 on the tree, 3 off the tree
    lo, hi = int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])
    for i0 in range(lo, hi):
        if state[i0]:
            continue
        walk, i = [], i0
        while state[i] == 0 and plist[i] != NO_PARENT:
            state[i] = 1
            walk.append(i)
            i = plist[i]
        if state[i] == 0:            # a head
            P[i] = (seed[i] * B + K[i]) & M64
            state[i] = 2
        on = state[i] == 2           # state 1: the walk met itself (a cycle); 3: off
        for j in reversed(walk):
            if on:
                P[j] = (P[plist[j]] * B + K[j]) & M64
            state[j] = 2 if on else 3
    return np.asarray(P, np.uint64), np.asarray([s == 2 for s in state], bool)


def jump_ref(sp, par=None, use_errors=False, svc_key="names", max_rounds=None):
    """The jumping form: (P, on_tree, rounds until no span was open any more or
    max_rounds).  max_rounds=None: ceil(log2(longest trace))."""
    par = parents_ref(sp) if par is None else par
    n = sp.n_spans
    K = np.asarray(label_keys(sp, use_errors, svc_key), np.uint64)
    seed = head_seeds(sp, par)
    lo, hi = int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])
    inside = np.zeros(n, bool)
    inside[lo:hi] = True
    head = np.asarray([s is not None for s in seed], bool)
    done = head | ~inside
    sd = np.asarray([s or 0 for s in seed], np.uint64)
    with np.errstate(over="ignore"):
        H = np.where(head, sd * np.uint64(B) + K, K)
        Mul = np.full(n, B, np.uint64)
        anc = np.where(done, np.arange(n), par)
        if max_rounds is None:
            L = int(np.diff(sp.trace_ptr).max()) if sp.n_traces else 1
            max_rounds = max(0, (max(L, 1) - 1).bit_length())
        rounds = 0
        for _ in range(max_rounds):
            open_ = ~done
            if not open_.any():
                break
            rounds += 1
            a = anc[open_]
            Ha, Ma, da, aa = H[a], Mul[a], done[a], anc[a]      # the state before the round
            H[open_] = Ha * Mul[open_] + H[open_]
            Mul[open_] = np.where(da, Mul[open_], Ma * Mul[open_])
            anc[open_] = aa
            done[open_] = da
    on = done & inside
    return np.where(on, H, np.uint64(0)), on, rounds


def shapes_ref(sp, P=None, on=None, **kw) -> np.ndarray:
    """shape[t]: the wrapping sum of mix64(P) over the on-tree spans."""
    if P is None:
        P, on = path_hash_ref(sp, **kw)
    ptr = sp.trace_ptr.tolist()
    Pl, ol = P.tolist(), on.tolist()
    out = []
    for t in range(sp.n_traces):
        s = 0
        for i in range(ptr[t], ptr[t + 1]):
            if ol[i]:
                s += mix64(Pl[i])
        out.append(s & M64)
    return np.asarray(out, np.uint64)


@dataclass
class CensusRef:
    shape: np.ndarray
    count: np.ndarray
    abnormal: np.ndarray
    first_trace: np.ndarray


def census_ref(shape, trace_class=None) -> CensusRef:
    rows = {}
    cls = [0] * len(shape) if trace_class is None else np.asarray(trace_class).tolist()
    for t, v in enumerate(np.asarray(shape, np.uint64).tolist()):
        r = rows.setdefault(v, [0, 0, t])
        r[0] += 1
        r[1] += 1 if cls[t] != 0 else 0
    order = sorted(rows.items(), key=lambda kv: (-kv[1][0], kv[0]))
    col = lambda k: np.asarray([r[k] for _, r in order], np.uint64)  # noqa: E731
    return CensusRef(np.asarray([v for v, _ in order], np.uint64), col(0), col(1), col(2))


def novelty_ref(sp, shape, base_shapes) -> np.ndarray:
    """Per service: traces of shapes absent from base_shapes whose exemplar
    (first trace of the shape) holds the service, over the traces of all
    shapes whose exemplar holds it; Python integers, one division."""
    cen = census_ref(shape)
    have = set(np.asarray(base_shapes, np.uint64).tolist())
    S = sp.n_services
    num, den = [0] * S, [0] * S
    ptr = sp.trace_ptr.tolist()
    for v, c, t in zip(cen.shape.tolist(), cen.count.tolist(), cen.first_trace.tolist()):
        for s in set(sp.svc[ptr[t]:ptr[t + 1]].tolist()):
            den[s] += c
            if v not in have:
                num[s] += c
    return np.asarray([a / b if b else 0.0 for a, b in zip(num, den)], np.float64)


# ---------------------------------------------------------------- set builders
def spanset(S, lens, sid, pid, svc=None, flags=None, unique=False):
    lens = np.asarray(lens, np.int64)
    ptr = np.zeros(lens.shape[0] + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    n = int(ptr[-1])
    sid = np.asarray(sid, np.uint64)
    svc = np.arange(n) % S if svc is None else svc
    flags = np.zeros(n) if flags is None else flags
    return anomod.SpanSet([f"svc{i:02d}" for i in range(S)], ptr, sid.copy(), sid,
                          np.asarray(pid, np.uint64), np.asarray(svc, np.uint16),
                          np.asarray(flags, np.uint16), np.full(n, 5, np.uint32),
                          unique_ids=unique)


def from_trees(trees, S=None, unique=True):
    """trees: per trace a list of (id, parent id, service index[, flags])."""
    rows = [r for tr in trees for r in tr]
    S = S or max(r[2] for r in rows) + 1
    return spanset(S, [len(tr) for tr in trees], [r[0] for r in rows], [r[1] for r in rows],
                   [r[2] for r in rows], [r[3] if len(r) > 3 else 0 for r in rows], unique)


def random_tree(rng, lens, orphan=0.03, S=9, self_ref=0.0, shuffle=True):
    """Traces of the given lengths: unique ids, random-ancestor parents, a
    share of orphans and of spans naming their own id, 10 % error flags, then
    (shuffle) every trace shuffled inside itself."""
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    starts = np.r_[0, np.cumsum(lens)[:-1]]
    t_of = np.repeat(np.arange(lens.shape[0]), lens)
    pos = np.arange(n) - starts[t_of]
    sid = rng.permutation(np.arange(1, n + 1, dtype=np.uint64)) + np.uint64(1 << 40)
    pick = starts[t_of] + (rng.random(n) * np.maximum(pos, 1)).astype(np.int64)
    pid = np.where(pos > 0, sid[pick], np.uint64(0))
    orph = (pos > 0) & (rng.random(n) < orphan)
    pid[orph] = rng.integers(1, 1 << 39, int(orph.sum()), dtype=np.uint64)
    own = rng.random(n) < self_ref
    pid[own] = sid[own]
    order = np.arange(n)
    if shuffle:
        order = np.concatenate([s + rng.permutation(k) for s, k in zip(starts, lens)])
    order = order.astype(np.int64)
    return spanset(S, lens, sid[order], pid[order], rng.integers(0, S, n)[order],
                   (rng.random(n) < 0.1)[order])


def chain(N, first_id=1, S=5):
    """(id, parent, service) rows of a chain N deep, the head first."""
    return [(first_id + k, first_id + k - 1 if k else 0, k % S) for k in range(N)]


def shuffled(sp, seed):
    """sp with every trace shuffled inside itself (unique ids stay unique)."""
    rng = np.random.default_rng(seed)
    ptr = sp.trace_ptr.astype(np.int64)
    order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(ptr[:-1], ptr[1:])])
    out = sp.take(order.astype(np.int64), sp.trace_ptr)
    out.unique_ids = sp.unique_ids
    return out


def without_subtrees(sp, service: str, every=10, par=None):
    """(set, altered trace mask): sp with, in every `every`-th trace that
    holds `service`, the spans of that service and everything below them
    removed."""
    par = parents_ref(sp) if par is None else par
    c = sp.services.index(service)
    t_of = sp.trace_of_span()
    holds = np.zeros(sp.n_traces, bool)
    holds[t_of[sp.svc == c]] = True
    pick = np.zeros(sp.n_traces, bool)
    pick[np.nonzero(holds)[0][::every]] = True
    drop = (sp.svc == c) & pick[t_of]
    has = par != NO_PARENT
    while True:                       # down the parent chains to a fixed point
        more = drop | (has & drop[np.where(has, par, 0)])
        if np.array_equal(more, drop):
            break
        drop = more
    keep = ~drop
    lens = np.bincount(t_of[keep], minlength=sp.n_traces)
    ptr = np.zeros(sp.n_traces + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    out = anomod.SpanSet(list(sp.services), ptr, sp.trace_hash[keep], sp.span_id[keep],
                         sp.parent_span_id[keep], sp.svc[keep], sp.flags[keep], sp.dur_us[keep],
                         sp.trace_ids, sp.unique_ids)
    return out, pick

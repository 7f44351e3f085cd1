"""Exact host model of the call repeats (a plain helper, not a conftest).

The definition of include/anomod.h (anomod_call_repeats_spans) restated in
Python integers: parents from self_time_ref.parents_ref (first match in
position order; a root, an orphan and a self-reference are heads), edge rows
from the C oracle (native.span_edges), and the groups from a dict keyed
(parent position, svc) that lists every group's members in position order.
after_error compares Python integers, so start + max(dur, 1) never wraps.
GPU results are compared to this model bit for bit.  The file also holds the
input helpers of the tests."""
from dataclasses import dataclass

import numpy as np

import anomod
from oracle import native

from self_time_ref import NO_PARENT, parents_ref

BINS = 8
TABLES = ("groups", "repeats", "repeated", "retried", "recovered", "exhausted", "after_error",
          "size_hist", "size_max")


@dataclass
class RepeatsRef:
    groups: np.ndarray        # u64 [E] ...
    repeats: np.ndarray
    repeated: np.ndarray
    retried: np.ndarray
    recovered: np.ndarray
    exhausted: np.ndarray
    after_error: np.ndarray
    size_hist: np.ndarray     # u64 [E, 8]
    size_max: np.ndarray      # u32 [E]
    grouped_spans: int
    max_size: int
    timed: bool
    span_group_size: np.ndarray    # u32 [n_spans]
    span_after_error: np.ndarray   # u8 [n_spans]
    members: dict                  # (parent position, svc) -> member positions


def group_members(sp, par=None) -> dict:
    """(parent position, svc) -> the group's member positions, ascending.
    Positions are global, so equal ids in two traces stay apart."""
    par = parents_ref(sp) if par is None else par
    svc = sp.svc.tolist()
    out = {}
    for i, j in enumerate(par.tolist()):
        if j != NO_PARENT:
            out.setdefault((j, svc[i]), []).append(i)
    return out


def bucket(n: int) -> int:
    return min(n.bit_length() - 1, BINS - 1)


def repeats_ref(sp, par=None) -> RepeatsRef:
    S = sp.n_services
    E = (S + 2) * S
    n_spans = sp.n_spans
    members = group_members(sp, par)
    rows = native.span_edges(sp, S).astype(np.int64).tolist() if n_spans else []
    err = ((sp.flags & anomod.FLAG_ERROR) != 0).tolist()
    svc = sp.svc.tolist()
    timed = sp.start_us is not None
    start = sp.start_us.tolist() if timed else None
    dur = sp.dur_us.tolist()
    tab = {k: [0] * E for k in TABLES if k != "size_hist"}
    hist = [[0] * BINS for _ in range(E)]
    gsize, after = [0] * n_spans, [0] * n_spans
    for (j, c), mem in members.items():
        r = svc[j] * S + c
        assert r < S * S and all(rows[i] == r for i in mem)   # the edge table's row
        n, e = len(mem), sum(err[i] for i in mem)
        tab["groups"][r] += 1
        tab["repeats"][r] += n - 1
        tab["repeated"][r] += n >= 2
        tab["retried"][r] += n >= 2 and e >= 1
        tab["recovered"][r] += n >= 2 and 1 <= e < n
        tab["exhausted"][r] += n >= 2 and e == n
        tab["size_max"][r] = max(tab["size_max"][r], n)
        hist[r][bucket(n)] += 1
        for i in mem:
            gsize[i] = n
        if not timed:
            continue
        ends = [start[m] + max(dur[m], 1) for m in mem if err[m] and start[m] != 0]
        if not ends:
            continue
        first_end = min(ends)
        for i in mem:
            if start[i] != 0 and start[i] >= first_end:
                after[i] = 1
                tab["after_error"][r] += 1
    u = {k: np.asarray(v, np.uint32 if k == "size_max" else np.uint64) for k, v in tab.items()}
    return RepeatsRef(size_hist=np.asarray(hist, np.uint64).reshape(E, BINS),
                      grouped_spans=sum(len(m) for m in members.values()),
                      max_size=max((len(m) for m in members.values()), default=0), timed=timed,
                      span_group_size=np.asarray(gsize, np.uint32),
                      span_after_error=np.asarray(after, np.uint8), members=members, **u)


def assert_repeats_equal(got, ref: RepeatsRef, per_span=True):
    """got: anomod.CallRepeats."""
    for k in TABLES:
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    assert (got.grouped_spans, got.max_size, got.timed) == \
        (ref.grouped_spans, ref.max_size, ref.timed)
    if per_span:
        np.testing.assert_array_equal(got.span_group_size, ref.span_group_size,
                                      err_msg="span_group_size")
        np.testing.assert_array_equal(got.span_after_error, ref.span_after_error,
                                      err_msg="span_after_error")


def assert_invariants(r, sp, par=None):
    """The invariants of the definition, on a model or a GPU result."""
    S = sp.n_services
    par = parents_ref(sp) if par is None else par
    rows = native.span_edges(sp, S).astype(np.int64)
    has = par != NO_PARENT
    np.testing.assert_array_equal(r.groups + r.repeats,
                                  np.bincount(rows[has], minlength=(S + 2) * S))
    assert not (r.groups + r.repeats)[S * S:].any()          # ROOT and ORPHAN rows
    np.testing.assert_array_equal(r.retried, r.recovered + r.exhausted)
    np.testing.assert_array_equal(r.size_hist.sum(axis=1), r.groups)
    np.testing.assert_array_equal(r.size_hist[:, 0], r.groups - r.repeated)
    assert r.grouped_spans == int(has.sum()) == int((r.groups + r.repeats).sum())
    assert r.max_size == int(r.size_max.max(initial=0))
    assert ((r.size_max > 0) == (r.groups > 0)).all()


# ---------------------------------------------------------------- input helpers
def build(S, traces, dur=5, start=None, unique_ids=False):
    """A span set from (ids, parent ids, flags, services) tuples, one per
    trace; dur / start: a scalar or one value per span (start None: no
    start-time column)."""
    lens = [len(t[0]) for t in traces]
    ptr = np.zeros(len(traces) + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    cat = lambda k, dt: (np.concatenate([np.asarray(t[k], dt) for t in traces])  # noqa: E731
                         if traces else np.zeros(0, dt))
    ids = cat(0, np.uint64)
    n = ids.shape[0]
    col = lambda v, dt: np.broadcast_to(np.asarray(v, dt), (n,)).copy()  # noqa: E731
    return anomod.SpanSet([f"svc{i:02d}" for i in range(S)], ptr, ids.copy(), ids,
                          cat(1, np.uint64), cat(3, np.uint16), cat(2, np.uint16),
                          col(dur, np.uint32), None, unique_ids,
                          start_us=None if start is None else col(start, np.uint64))


def star(L, n_callees, first_id=1000, flagged=False):
    """(ids, parent ids, flags, services) of a root (service 0) with L - 1
    children on the services 1 .. n_callees in turn: n_callees groups under
    one parent.  flagged: every child carries the error flag."""
    ids = np.arange(first_id, first_id + L, dtype=np.uint64)
    pid = np.r_[np.uint64(0), np.full(L - 1, first_id, np.uint64)]
    flags = np.r_[np.uint16(0), np.full(L - 1, anomod.FLAG_ERROR if flagged else 0, np.uint16)]
    svc = np.r_[0, 1 + np.arange(L - 1) % n_callees]
    return ids, pid, flags, svc


def add_repeats(sp, service, share, k, rng, fail_first=True):
    """A new SpanSet in which a `share` of the groups of `service` (drawn by
    rng) went out k times instead of once: right before the first member of
    each drawn group stand k - 1 more siblings with fresh ids, the same parent
    reference and service, duration and trace.  With fail_first the k - 1
    earlier attempts carry the error flag, the last one — it keeps the
    original id, so the original's children stay with it — does not, and the
    attempts are laid end to end in start_us (a set without the column gets
    one: 0, no time recorded, for every other span).  Without it the siblings
    copy the original's flags and start time.  Returns (set, positions of the
    drawn members in the new set: one per group made)."""
    members = group_members(sp)
    c = sp.services.index(service)
    firsts = np.asarray(sorted(m[0] for (_, s), m in members.items() if s == c), np.int64)
    picked = firsts[rng.random(firsts.shape[0]) < share]
    n = sp.n_spans
    reps = np.ones(n, np.int64)
    reps[picked] = k
    src = np.repeat(np.arange(n), reps)                  # original position of every new span
    run0 = np.cumsum(reps) - reps                        # new position of each original's first copy
    attempt = np.arange(src.shape[0]) - run0[src]        # 0 .. k - 1 inside a drawn run
    last = attempt == reps[src] - 1
    extra = ~last                                        # the added siblings: the earlier attempts
    sid = sp.span_id[src].copy()
    taken = set(sp.span_id.tolist())
    fresh = []
    while len(fresh) < int(extra.sum()):
        v = int(rng.integers(1, 1 << 62))
        if v not in taken:
            taken.add(v)
            fresh.append(v)
    sid[extra] = np.asarray(fresh, np.uint64)
    flags = sp.flags[src].copy()
    start = None if sp.start_us is None else sp.start_us[src].copy()
    if fail_first:
        in_run = reps[src] > 1
        flags[extra] |= anomod.FLAG_ERROR
        flags[in_run & last] &= np.uint16(~anomod.FLAG_ERROR & 0xFFFF)
        if start is None:
            start = np.zeros(src.shape[0], np.uint64)
        base = np.where(start != 0, start, np.uint64(1_000_000) + src.astype(np.uint64) * 1000)
        step = np.maximum(sp.dur_us[src], 1).astype(np.uint64)
        start = np.where(in_run, base + attempt.astype(np.uint64) * step, start)
    assert int(sp.trace_ptr[0]) == 0 and int(sp.trace_ptr[-1]) == n   # every span in a trace
    lens = np.bincount(sp.trace_of_span(), weights=reps, minlength=sp.n_traces).astype(np.int64)
    ptr = np.zeros(sp.n_traces + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    out = anomod.SpanSet(list(sp.services), ptr, sp.trace_hash[src], sid, sp.parent_span_id[src],
                         sp.svc[src], flags, sp.dur_us[src], sp.trace_ids, sp.unique_ids,
                         start_us=start)
    return out, run0[picked]


def hand_made():
    """One trace of 12 spans, not declared unique, and what the definition
    gives for it, written out by hand (services a = 0, b = 1, c = 2).

    pos id  parent  svc flag  what
     0  10   0      a   -     ROOT: a head; the parent at position 0
     1  20  10      b   E     group (0, b) ...
     2  21  10      b   -     ... two children to the same callee: n 2, e 1, recovered
     3  22  10      c   -     group (0, c): a child of the same parent to another callee
     4  30  20      c   -     group (1, c): the same callee under another parent
     5  40  999     a   -     ORPHAN: a head
     6  50  50      b   -     SELF: a head
     7  60  22      a   -     duplicated id, first carrier; group (3, a) ...
     8  60  22      a   E     ... second carrier: n 2, e 1, recovered
     9  61  60      b   -     the children of id 60 all join the first carrier (7):
    10  62  60      b   -     group (7, b): n 2, e 0
    11  63  60      c   E     group (7, c): n 1 (a failure that was not repeated)
    """
    ids = [10, 20, 21, 22, 30, 40, 50, 60, 60, 61, 62, 63]
    pids = [0, 10, 10, 10, 20, 999, 50, 22, 22, 60, 60, 60]
    svc = [0, 1, 1, 2, 2, 0, 1, 0, 0, 1, 1, 2]
    flags = [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1]
    sp = build(3, [(ids, pids, flags, svc)])
    size = [0, 2, 2, 1, 1, 0, 0, 2, 2, 2, 2, 1]
    # rows p * 3 + c: a->b 1, a->c 2, b->c 5, c->a 6
    want = {"groups": {1: 2, 2: 2, 5: 1, 6: 1}, "repeats": {1: 2, 6: 1}, "repeated": {1: 2, 6: 1},
            "retried": {1: 1, 6: 1}, "recovered": {1: 1, 6: 1}, "exhausted": {},
            "size_max": {1: 2, 2: 1, 5: 1, 6: 2}}
    return sp, size, want

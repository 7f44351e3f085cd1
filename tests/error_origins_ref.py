"""Exact host model of the error origins (a plain helper, not a conftest).

The definition of include/anomod.h (anomod_error_origins_spans) restated in
Python integers: parents from self_time_ref.parents_ref (first match in
position order; a root, an orphan and a self-reference are heads), edge rows
from the C oracle (native.span_edges), the class of a span from its own error
flag and the number of its error-flagged children, and fate and hops by
literally following up(i) — the parent while it exists and carries the flag —
with a step cap of the trace length: a chain that has not ended by then runs
in a reference cycle (LOOP, hops 0).  GPU results are compared to this model
bit for bit.  The file also holds the input helpers of the tests."""
from dataclasses import dataclass

import numpy as np

import anomod
from oracle import native

from self_time_ref import NO_PARENT, parents_ref

CLEAN, ORIGIN, PROPAGATED, ABSORBER = 0, 1, 2, 3
SURFACED, CONTAINED, LOOP = 1, 2, 3
TABLES = ("origin", "propagated", "stopped", "surfaced", "absorbers", "hops_sum", "hops_max")


@dataclass
class OriginsRef:
    cls: np.ndarray          # u8 [n_spans]
    fate: np.ndarray         # u8 [n_spans]
    hops: np.ndarray         # u32 [n_spans]
    origin: np.ndarray       # u64 [E] ...
    propagated: np.ndarray
    stopped: np.ndarray
    surfaced: np.ndarray
    absorbers: np.ndarray
    hops_sum: np.ndarray
    hops_max: np.ndarray     # u32 [E]
    error_spans: int
    loop_spans: int

    @property
    def span_state(self) -> np.ndarray:
        return (self.cls | (self.fate << 2)).astype(np.uint8)


def span_classes_ref(sp, par=None):
    """(class, fate, hops) lists by span position; spans outside every trace
    read 0 / 0 / 0."""
    par = parents_ref(sp) if par is None else par
    plist = par.tolist()
    err = ((sp.flags & anomod.FLAG_ERROR) != 0).tolist()
    ptr = sp.trace_ptr.tolist()
    n = sp.n_spans
    cls, fate, hops = [CLEAN] * n, [0] * n, [0] * n
    kid_err = [0] * n
    for t in range(sp.n_traces):
        for i in range(ptr[t], ptr[t + 1]):
            if err[i] and plist[i] != NO_PARENT:
                kid_err[plist[i]] += 1
    for t in range(sp.n_traces):
        cap = ptr[t + 1] - ptr[t]
        for i in range(ptr[t], ptr[t + 1]):
            if not err[i]:
                cls[i] = ABSORBER if kid_err[i] else CLEAN
                continue
            cls[i] = PROPAGATED if kid_err[i] else ORIGIN
            j, steps = i, 0
            while steps <= cap:
                p = plist[j]
                if p == NO_PARENT or not err[p]:
                    break
                j = p
                steps += 1
            if steps > cap:                     # the chain never ends
                fate[i] = LOOP
            else:
                fate[i] = SURFACED if plist[j] == NO_PARENT else CONTAINED
                hops[i] = steps
    return cls, fate, hops


def origins_ref(sp, par=None) -> OriginsRef:
    S = sp.n_services
    E = (S + 2) * S
    cls, fate, hops = span_classes_ref(sp, par)
    rows = native.span_edges(sp, S).astype(np.int64).tolist() if sp.n_spans else []
    tab = {k: [0] * E for k in TABLES}
    err = ((sp.flags & anomod.FLAG_ERROR) != 0).tolist()
    n_err = n_loop = 0
    for i in range(int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])):
        c, f, h, r = cls[i], fate[i], hops[i], rows[i]
        if c == ABSORBER:
            tab["absorbers"][r] += 1
        if not err[i]:
            continue
        n_err += 1
        n_loop += f == LOOP
        tab["origin" if c == ORIGIN else "propagated"][r] += 1
        if h == 0 and f == CONTAINED:
            tab["stopped"][r] += 1
        if c == ORIGIN:
            tab["surfaced"][r] += f == SURFACED
            tab["hops_sum"][r] += h
            tab["hops_max"][r] = max(tab["hops_max"][r], h)
    u = {k: np.asarray(v, np.uint32 if k == "hops_max" else np.uint64) for k, v in tab.items()}
    return OriginsRef(np.asarray(cls, np.uint8), np.asarray(fate, np.uint8),
                      np.asarray(hops, np.uint32), error_spans=n_err, loop_spans=n_loop, **u)


def assert_origins_equal(got, ref: OriginsRef, per_span=True):
    """got: anomod.ErrorOrigins."""
    for k in TABLES:
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    assert (got.error_spans, got.loop_spans) == (ref.error_spans, ref.loop_spans)
    if per_span:
        np.testing.assert_array_equal(got.span_state, ref.span_state, err_msg="span_state")
        np.testing.assert_array_equal(got.span_hops, ref.hops, err_msg="span_hops")


# ---------------------------------------------------------------- input helpers
def with_flags(sp, flags):
    """sp with another flags column."""
    return anomod.SpanSet(list(sp.services), sp.trace_ptr, sp.trace_hash, sp.span_id,
                          sp.parent_span_id, sp.svc, np.ascontiguousarray(flags, np.uint16),
                          sp.dur_us, sp.trace_ids, sp.unique_ids, start_us=sp.start_us)


def propagate_errors(sp, service: str, share: float, p_up: float, rng, par=None):
    """sp with every flag cleared, then a `share` of the spans of `service`
    flagged and, from each of them, the parent flagged with probability p_up,
    and so on upward: some chains reach the head of their trace, some are
    contained.  Every flagged span of another service has a flagged child, so
    no failure starts outside `service`."""
    par = parents_ref(sp) if par is None else par
    plist = par.tolist()
    c = sp.services.index(service)
    flag = np.zeros(sp.n_spans, bool)
    seeds = np.flatnonzero((sp.svc == c) & (rng.random(sp.n_spans) < share))
    flag[seeds] = True
    coin = rng.random((seeds.shape[0], 16)) < p_up      # (chains deeper than 16 stop there)
    for k, i in enumerate(seeds.tolist()):
        j = i
        for up in coin[k].tolist():
            if not up or plist[j] == NO_PARENT:
                break
            j = plist[j]
            flag[j] = True
    return with_flags(sp, flag.astype(np.uint16) * anomod.FLAG_ERROR)


def inclusive_error_rate(sp) -> np.ndarray:
    """Per service: error-flagged spans over spans (the default error term)."""
    S = sp.n_services
    cnt = np.bincount(sp.svc, minlength=S).astype(np.float64)
    err = np.bincount(sp.svc[(sp.flags & anomod.FLAG_ERROR) != 0], minlength=S).astype(np.float64)
    return np.divide(err, cnt, out=np.zeros(S), where=cnt > 0)


def hand_made():
    """One trace of 12 spans, not declared unique, and what the definition
    gives for it, written out by hand (services a = 0, b = 1, c = 2).

    pos id  parent  flag  what
     0  30  20      E     child before its parent (span 1); ORIGIN, 1 hop, SURFACED
     1  20   0      E     root with two failing children (0, 2): PROPAGATED, SURFACED, 0 hops
     2  31  20      E     second ORIGIN under the same propagated parent
     3  40  20      -     clean child of span 1, parent of span 4: ABSORBER
     4  41  40      E     PROPAGATED, top of a contained chain (0 hops, CONTAINED): stopped here
     5  42  41      E     PROPAGATED, 1 hop, CONTAINED
     6  43  42      E     ORIGIN, 2 hops, CONTAINED (the two-step chain that is contained)
     7  50  50      E     SELF reference: a head; ORIGIN, SURFACED, 0 hops
     8  60  999     E     ORPHAN: a head; ORIGIN, SURFACED, 0 hops
     9  70  20      -     duplicated id, first carrier: gets span 11's error (ABSORBER)
    10  70  20      -     second carrier of id 70: no child resolves to it, CLEAN
    11  71  70      E     ORIGIN under the first carrier (span 9), 0 hops, CONTAINED
    """
    ids = [30, 20, 31, 40, 41, 42, 43, 50, 60, 70, 70, 71]
    pids = [20, 0, 20, 20, 40, 41, 42, 50, 999, 20, 20, 70]
    flags = [1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1]
    svc = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2]
    sp = anomod.SpanSet(["a", "b", "c"], [0, 12], [7] * 12, ids, pids, svc, flags, [5] * 12)
    cls = [ORIGIN, PROPAGATED, ORIGIN, ABSORBER, PROPAGATED, PROPAGATED, ORIGIN, ORIGIN, ORIGIN,
           ABSORBER, CLEAN, ORIGIN]
    fate = [SURFACED, SURFACED, SURFACED, 0, CONTAINED, CONTAINED, CONTAINED, SURFACED, SURFACED,
            0, 0, CONTAINED]
    hops = [1, 0, 1, 0, 0, 1, 2, 0, 0, 0, 0, 0]
    return sp, cls, fate, hops


def chain_trace(L, first_id, flagged_root=True, reverse=False, S=4):
    """(ids, parent ids, flags, services) of a chain L deep, every span
    flagged (the root only with flagged_root); reverse: children before
    parents."""
    ids = np.arange(first_id, first_id + L, dtype=np.uint64)
    pid = np.r_[np.uint64(0), ids[:-1]]
    flags = np.ones(L, np.uint16)
    flags[0] = 1 if flagged_root else 0
    svc = np.arange(L) % S
    if reverse:
        ids, pid, flags, svc = ids[::-1], pid[::-1], flags[::-1], svc[::-1]
    return ids, pid, flags, svc


def build(S, traces):
    """A span set from (ids, parent ids, flags, services) tuples, one per trace."""
    lens = [len(t[0]) for t in traces]
    ptr = np.zeros(len(traces) + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    cat = lambda k, dt: (np.concatenate([np.asarray(t[k], dt) for t in traces])  # noqa: E731
                         if traces else np.zeros(0, dt))
    ids = cat(0, np.uint64)
    return anomod.SpanSet([f"svc{i:02d}" for i in range(S)], ptr, ids.copy(), ids,
                          cat(1, np.uint64), cat(3, np.uint16), cat(2, np.uint16),
                          np.full(ids.shape[0], 5, np.uint32))

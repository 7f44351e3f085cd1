"""Exact host model of the call transit (a plain helper, not a conftest).

The definition of include/anomod.h (anomod_call_transit_spans) restated in
Python integers: parents from self_time_ref.parents_ref (first match in
position order; a root, an orphan and a self-reference are heads), kids counted
per parent position, every span classified, and the two tables accumulated into
the C oracle's empty tables (native.new_tables) with its histogram bin
(native.hist_bin) and finalize.  Ends are min(start + dur, 2^64 - 1) and gaps
min(gap, 2^32 - 1) in Python integers, so nothing wraps.  GPU results are
compared to this model bit for bit.  The file also holds the input helpers of
the tests."""
from dataclasses import dataclass

import numpy as np

import anomod
from oracle import native

from self_time_ref import NO_PARENT, parents_ref

U64_MAX = 2**64 - 1
U32_MAX = 2**32 - 1
CALL, PAIRED, TIMED, EARLY, LATE = 1, 2, 4, 8, 16
COUNTS = ("untimed", "early", "late", "early_us", "late_us")
FIELDS = ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us")


@dataclass
class TransitRef:
    request: dict             # the C oracle's table dict, finalized
    response: dict
    untimed: np.ndarray       # u64 [E] ...
    early: np.ndarray
    late: np.ndarray
    early_us: np.ndarray
    late_us: np.ndarray
    calls: int
    paired: int
    span_req_us: np.ndarray   # u32 [n_spans]
    span_resp_us: np.ndarray  # u32 [n_spans]
    span_state: np.ndarray    # u8 [n_spans]


def _record(tab, r, err, v):
    tab["count"][r] += np.uint64(1)
    tab["errors"][r] += np.uint64(err)
    tab["sum_us"][r] += np.uint64(v)
    tab["min_us"][r] = min(int(tab["min_us"][r]), v)
    tab["max_us"][r] = max(int(tab["max_us"][r]), v)
    tab["hist"][r, native.hist_bin(v)] += np.uint64(1)


def transit_ref(sp, par=None) -> TransitRef:
    S = sp.n_services
    E = (S + 2) * S
    n = sp.n_spans
    par = (parents_ref(sp) if par is None else par).tolist()
    kids = [0] * n
    for j in par:
        if j != NO_PARENT:
            kids[j] += 1
    s = sp.start_us.tolist()
    d = sp.dur_us.tolist()
    e = [min(si + di, U64_MAX) for si, di in zip(s, d)]
    svc = sp.svc.tolist()
    err = ((sp.flags & anomod.FLAG_ERROR) != 0).tolist()
    req, resp = native.new_tables(S), native.new_tables(S)
    cnt = {k: [0] * E for k in COUNTS}
    req_us, resp_us, state = [0] * n, [0] * n, [0] * n
    calls = paired = 0
    for c, p in enumerate(par):
        if p == NO_PARENT:
            continue
        state[c] = CALL
        calls += 1
        if kids[p] != 1:
            continue
        state[c] |= PAIRED
        paired += 1
        r = svc[p] * S + svc[c]
        if s[c] == 0 or s[p] == 0:
            cnt["untimed"][r] += 1
            continue
        state[c] |= TIMED
        if s[c] >= s[p]:
            req_us[c] = min(s[c] - s[p], U32_MAX)
            _record(req, r, err[c], req_us[c])
        else:
            state[c] |= EARLY
            cnt["early"][r] += 1
            cnt["early_us"][r] += min(s[p] - s[c], U32_MAX)
        if e[c] <= e[p]:
            resp_us[c] = min(e[p] - e[c], U32_MAX)
            _record(resp, r, err[c], resp_us[c])
        else:
            state[c] |= LATE
            cnt["late"][r] += 1
            cnt["late_us"][r] += min(e[c] - e[p], U32_MAX)
    return TransitRef(native.finalize(req), native.finalize(resp),
                      **{k: np.asarray(v, np.uint64) for k, v in cnt.items()},
                      calls=calls, paired=paired, span_req_us=np.asarray(req_us, np.uint32),
                      span_resp_us=np.asarray(resp_us, np.uint32),
                      span_state=np.asarray(state, np.uint8))


def as_call_transit(ref: TransitRef, services, with_hist=True) -> "anomod.CallTransit":
    """The model's result as the object Context.call_transit returns."""
    def table(t):
        return anomod.EdgeTable(list(services), t["count"], t["errors"], t["sum_us"], t["min_us"],
                                t["max_us"], t["p50_us"], t["p99_us"],
                                t["hist"] if with_hist else None)
    return anomod.CallTransit(list(services), table(ref.request), table(ref.response),
                              *(getattr(ref, k) for k in COUNTS), ref.calls, ref.paired)


def assert_transit_equal(got, ref: TransitRef, per_span=True):
    """got: anomod.CallTransit — every table field, array, scalar and column."""
    for name in ("request", "response"):
        tg, tr = getattr(got, name), getattr(ref, name)
        for k in FIELDS:
            if k == "hist" and tg.hist is None:
                continue
            assert np.array_equal(getattr(tg, k), tr[k], equal_nan=True), f"{name}.{k}"
    for k in COUNTS:
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    assert (got.calls, got.paired) == (ref.calls, ref.paired)
    if per_span:
        for k in ("span_req_us", "span_resp_us", "span_state"):
            np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)


def _count(t):
    return t["count"] if isinstance(t, dict) else t.count


def assert_invariants(r, sp, par=None):
    """The three invariants of the definition, on a model or a GPU result."""
    S = sp.n_services
    E = (S + 2) * S
    par = parents_ref(sp) if par is None else par
    has = par != NO_PARENT
    kids = np.bincount(par[has], minlength=sp.n_spans)
    pair = has & (kids[np.where(has, par, 0)] == 1)
    rows = sp.svc[np.where(has, par, 0)].astype(np.int64) * S + sp.svc.astype(np.int64)
    rq, rs = _count(r.request), _count(r.response)
    np.testing.assert_array_equal(rq + r.early + r.untimed, np.bincount(rows[pair], minlength=E))
    np.testing.assert_array_equal(rs + r.late, rq + r.early)
    assert not (rq + rs + r.early + r.late + r.untimed + r.early_us + r.late_us)[S * S:].any()
    edge = native.edge_aggregate(sp)["count"][:S * S]
    selfs = (~has) & (sp.parent_span_id == sp.span_id) & (sp.parent_span_id != 0)
    assert r.calls == int(has.sum()) == int(edge.sum()) - int(selfs.sum())
    assert r.paired == int(pair.sum())


# ---------------------------------------------------------------- input helpers
def build(S, rows, services=None, unique_ids=False):
    """A span set from one list of (id, parent, svc, start, dur[, flags]) rows
    per trace."""
    flat = [r for t in rows for r in t]
    ptr = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(t) for t in rows], out=ptr[1:])
    col = lambda k, dt: np.asarray([r[k] for r in flat], dt)  # noqa: E731
    ids = col(0, np.uint64)
    names = [f"svc{i:02d}" for i in range(S)] if services is None else list(services)
    return anomod.SpanSet(names, ptr, ids.copy(), ids, col(1, np.uint64), col(2, np.uint16),
                          np.asarray([r[5] if len(r) > 5 else 0 for r in flat], np.uint16),
                          col(4, np.uint32), None, unique_ids, start_us=col(3, np.uint64))


HAND_ROWS = [(1, 0, 0, 1000, 100),     # head, two kids
             (2, 1, 0, 1010, 50),      # call, unpaired
             (3, 1, 0, 1060, 30),      # call, unpaired
             (4, 2, 1, 1015, 40),      # paired, row 1: request 5, response 5
             (5, 3, 2, 1055, 40),      # paired, row 2: early by 5 and late by 5, no record
             (6, 4, 2, 0, 10),         # paired, row 5: untimed
             (7, 99, 1, 1000, 1),      # orphan: head
             (8, 8, 1, 1000, 1)]       # self-reference: head
HAND_STATE = [0, CALL, CALL, CALL | PAIRED | TIMED, CALL | PAIRED | TIMED | EARLY | LATE,
              CALL | PAIRED, 0, 0]


def hand_made():
    """The issue's worked trace (S = 3) and what the definition gives for it:
    calls 5, paired 3; request and response one record of 5 on row 1; early,
    late 1 and early_us, late_us 5 on row 2; untimed 1 on row 5."""
    return build(3, [HAND_ROWS])


def check_hand_made(r, k=1):
    """r (a model or a GPU result) is k times the hand-made trace's result."""
    assert (r.calls, r.paired) == (5 * k, 3 * k)
    sparse = lambda a: {i: int(v) for i, v in enumerate(a) if v}  # noqa: E731
    for t in (r.request, r.response):
        get = (lambda f: t[f]) if isinstance(t, dict) else (lambda f: getattr(t, f))
        assert sparse(get("count")) == {1: k} and sparse(get("sum_us")) == {1: 5 * k}
        assert not get("errors").any()
        assert int(get("min_us")[1]) == 5 and int(get("max_us")[1]) == 5
        assert int(get("hist").sum()) == k
    assert sparse(r.early) == sparse(r.late) == {2: k}
    assert sparse(r.early_us) == sparse(r.late_us) == {2: 5 * k}
    assert sparse(r.untimed) == {5: k}
    if r.span_state is not None:
        assert r.span_state.tolist() == HAND_STATE * k
        assert r.span_req_us.tolist() == [0, 0, 0, 5, 0, 0, 0, 0] * k
        assert r.span_resp_us.tolist() == [0, 0, 0, 5, 0, 0, 0, 0] * k


TRANSIT_SERVICES = ["a", "b", "c", "front"]
T0_US = 1_700_000_000_000_000


def transit_set(n_traces, seed, slow=None, d_req=0, d_resp=0, abandon=0.0):
    """Every trace: front server span -> front client span -> a's server span
    -> two client spans of a laid end to end -> the server spans of b and c.
    Base request / response gaps are drawn from 150-250 and 100-200 us.
    slow="b" (or "c") adds d_req / d_resp to the gaps of the pair into that
    service: its client span and every ancestor grow by d_req + d_resp, what
    follows the client span inside a (for b: a's later client span and its
    child) moves by as much, the slow service's own span keeps its duration —
    no other pair's gaps change.  For a share `abandon` of those calls the
    client span ends 1 us before the callee's span does."""
    rng = np.random.default_rng(seed)
    n = n_traces
    A, B, C_, F = 0, 1, 2, 3
    gap = lambda lo, hi: rng.integers(lo, hi + 1, n)  # noqa: E731
    rq = {k: gap(150, 250) for k in ("a", "b", "c")}
    rs = {k: gap(100, 200) for k in ("a", "b", "c")}
    own = {"b": gap(2000, 3000), "c": gap(1000, 2000)}
    drop = rng.random(n) < abandon
    if slow is not None:
        assert slow in ("b", "c")
        rq[slow] = rq[slow] + d_req
        rs[slow] = rs[slow] + d_resp
    t0 = T0_US + np.arange(n) * 1_000_000
    f_srv_s = t0
    f_cli_s = f_srv_s + 50
    a_srv_s = f_cli_s + rq["a"]
    cb_s = a_srv_s + 40                                   # a's client span into b
    b_s = cb_s + rq["b"]
    cb_d = rq["b"] + own["b"] + rs["b"]
    cc_s = cb_s + cb_d + 10                               # a's client span into c, end to end
    c_s = cc_s + rq["c"]
    cc_d = rq["c"] + own["c"] + rs["c"]
    a_srv_d = (cc_s + cc_d + 30) - a_srv_s
    f_cli_d = rq["a"] + a_srv_d + rs["a"]
    f_srv_d = 50 + f_cli_d + 50
    if slow is not None and abandon > 0:
        # the client span into `slow` ends 1 us before the callee does; nothing else moves
        end = (b_s + own["b"] if slow == "b" else c_s + own["c"]) - 1
        if slow == "b":
            cb_d = np.where(drop, end - cb_s, cb_d)
        else:
            cc_d = np.where(drop, end - cc_s, cc_d)
    ids = np.arange(1, 7 * n + 1, dtype=np.uint64).reshape(n, 7)
    pid = np.stack([np.zeros(n, np.uint64), ids[:, 0], ids[:, 1], ids[:, 2], ids[:, 3], ids[:, 2],
                    ids[:, 5]], 1)
    start = np.stack([f_srv_s, f_cli_s, a_srv_s, cb_s, b_s, cc_s, c_s], 1)
    dur = np.stack([f_srv_d, f_cli_d, a_srv_d, cb_d, own["b"], cc_d, own["c"]], 1)
    svc = np.tile(np.array([F, F, A, A, B, A, C_], np.uint16), n)
    ptr = np.arange(n + 1, dtype=np.uint64) * 7
    return anomod.SpanSet(list(TRANSIT_SERVICES), ptr, np.repeat(ids[:, 0], 7), ids.ravel(),
                          pid.ravel(), svc, np.zeros(7 * n, np.uint16),
                          dur.ravel().astype(np.uint32), unique_ids=True,
                          start_us=start.ravel().astype(np.uint64))

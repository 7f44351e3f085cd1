"""Reference for the critical path and its edge table (a plain helper, not a
conftest), and the input helpers of its tests.

The definition (include/anomod.h) is restated in Python
integers on top of self_time_ref.parents_ref:

    s(i) = start_us[i];  e(i) = min(s(i) + dur_us[i], 2^64 - 1)
    head: a span of a trace without a parent (root, orphan, self-reference)
    child c of p: a = max(s(c), s(p)), b = min(e(c), e(p)), eligible if a < b
    selection at p: cur = e(p); among the eligible children with b <= cur take
        the largest b (smallest position among equal b), select it, cur = a
    on_path: heads, and selected spans whose parent is on the path (the least
        such set: a breadth-first walk down from the heads)
    cp_us[i] = dur_us[i] - sum of (b - a) over the selected children of i,
        for i on the path, else 0

The table is the C oracle's edge table of the on-path sub-set with dur_us
replaced by cp_us: an on-path span's parent is on the path and is the first
carrier of its id, so every kept span keeps its edge row.  Every result is an
integer: GPU results are compared to it bit for bit."""
import numpy as np

import anomod
from oracle import native

from self_time_ref import NO_PARENT, parents_ref

U64_MAX = 2**64 - 1
T0_US = 1_700_000_000_000_000


def with_cols(sp, dur_us=None, start_us=None):
    """sp with other duration / start columns."""
    return anomod.SpanSet(list(sp.services), sp.trace_ptr, sp.trace_hash, sp.span_id,
                          sp.parent_span_id, sp.svc, sp.flags,
                          np.ascontiguousarray(sp.dur_us if dur_us is None else dur_us, np.uint32),
                          sp.trace_ids, sp.unique_ids,
                          start_us=sp.start_us if start_us is None else
                          np.ascontiguousarray(start_us, np.uint64))


def _children(par):
    kids = {}
    for i, j in enumerate(par.tolist()):
        if j != NO_PARENT:
            kids.setdefault(j, []).append(i)       # position order
    return kids


def select_literal(cur, cands):
    """The definition's loop, word for word; cands = [(a, b, position)]."""
    out = []
    while True:
        fit = [c for c in cands if c[1] <= cur and c[2] not in out]
        if not fit:
            return out
        best = max(c[1] for c in fit)
        a, _, pos = min((c for c in fit if c[1] == best), key=lambda c: c[2])
        out.append(pos)
        cur = a


def select_sorted(cur, cands):
    """The same selection in one pass over the candidates by (b descending,
    position ascending): the cursor only moves down, so a candidate passed
    over once (b > cur) never fits later, and the first that fits is the
    definition's choice."""
    out = []
    for a, b, pos in sorted(cands, key=lambda c: (-c[1], c[2])):
        if b <= cur:
            out.append(pos)
            cur = a
    return out


def critical_path_ref(sp, par=None, select=select_sorted):
    """(cp_us u32 [n], on_path u8 [n], selected-children count per span)."""
    par = parents_ref(sp) if par is None else par
    n = sp.n_spans
    s = sp.start_us.tolist()
    d = sp.dur_us.tolist()
    e = [min(si + di, U64_MAX) for si, di in zip(s, d)]
    kids = _children(par)
    selected = {}                                   # parent -> [(child, b - a)]
    for p, cs in kids.items():
        cands = []
        for c in cs:
            a, b = max(s[c], s[p]), min(e[c], e[p])
            if a < b:
                cands.append((a, b, c))
        length = {c: b - a for a, b, c in cands}
        selected[p] = [(c, length[c]) for c in select(e[p], cands)]
    lo, hi = int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])
    plist = par.tolist()
    on = np.zeros(n, np.uint8)
    front = [i for i in range(lo, hi) if plist[i] == NO_PARENT]
    while front:
        nxt = []
        for i in front:
            on[i] = 1
            nxt.extend(c for c, _ in selected.get(i, ()))
        front = nxt
    cp = np.zeros(n, np.uint32)
    nsel = np.zeros(n, np.int64)
    for i in range(n):
        sel = selected.get(i, ())
        nsel[i] = len(sel)
        if on[i]:
            cp[i] = d[i] - sum(w for _, w in sel)
    return cp, on, nsel


def cp_table_ref(sp, cp_us, on_path) -> dict:
    keep = np.nonzero(on_path)[0]
    before = np.r_[0, np.cumsum(on_path.astype(np.int64))]   # on-path spans before a position
    tp = sp.trace_ptr.astype(np.int64)
    lens = before[tp[1:]] - before[tp[:-1]]
    ptr = np.zeros(sp.n_traces + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    in_tr = (keep >= int(sp.trace_ptr[0])) & (keep < int(sp.trace_ptr[-1]))
    assert in_tr.all() and int(ptr[-1]) == keep.shape[0]
    sub = anomod.SpanSet(list(sp.services), ptr, sp.trace_hash[keep], sp.span_id[keep],
                         sp.parent_span_id[keep], sp.svc[keep], sp.flags[keep], cp_us[keep])
    return native.finalize(native.edge_aggregate(sub))


# ------------------------------------------------------------------ inputs
def _levels(par):
    """Positions by depth along the parent chain (heads first); a span whose
    chain never reaches a head is left out."""
    kids = _children(par)
    level = [i for i, j in enumerate(par.tolist()) if j == NO_PARENT]
    out = []
    while level:
        out.append(level)
        level = [c for p in level for c in kids.get(p, ())]
    return out, kids


def nested_set(sp, par, p_seq, seed):
    """sp with durations rewritten bottom-up and starts top-down so that
    children lie inside their parents: own = old dur % 1000 + 1; a parent lays
    its children back to back with probability p_seq (dur = own + sum), else
    all starting together (dur = own + max); the children begin own // 2 after
    the parent."""
    rng = np.random.default_rng(seed)
    levels, kids = _levels(par)
    n = sp.n_spans
    own = (sp.dur_us.astype(np.int64) % 1000 + 1).tolist()
    seq = (rng.random(n) < p_seq).tolist()
    dur = list(own)
    for level in reversed(levels):
        for p in level:
            cs = kids.get(p)
            if cs:
                dur[p] = own[p] + (sum(dur[c] for c in cs) if seq[p] else max(dur[c] for c in cs))
    t_of = sp.trace_of_span()
    start = (T0_US + t_of * 1000).tolist()
    for level in levels:
        for p in level:
            t = start[p] + own[p] // 2
            for c in kids.get(p, ()):
                start[c] = t
                if seq[p]:
                    t += dur[c]
    assert max(dur) < 2**32
    return with_cols(sp, dur, np.asarray(start, np.uint64))


def random_starts(sp, seed, par=None):
    """sp with its durations kept and every child started at an arbitrary
    offset around its parent's interval (clipping, ineligible children)."""
    par = parents_ref(sp) if par is None else par
    rng = np.random.default_rng(seed)
    levels, kids = _levels(par)
    d = sp.dur_us.astype(np.int64)
    u = rng.random(sp.n_spans)
    start = (T0_US + sp.trace_of_span() * 1000).tolist()
    for level in levels:
        for p in level:
            for c in kids.get(p, ()):
                span = int(d[p]) + int(d[c]) + 20
                start[c] = start[p] - int(d[c]) - 10 + int(u[c] * span)
    return with_cols(sp, start_us=np.asarray(start, np.uint64))


FANOUT_SERVICES = ["a", "b", "c", "gateway", "root"]


def fanout_set(n_traces, seed, gateway_extra_us=0, b_extra_us=0):
    """root -> gateway (100 ms +- 10 ms) -> a, b, c in parallel (0.9, 0.5, 0.3
    of the gateway), every trace the same five spans.  gateway_extra_us is
    added to the gateway's own work (children unchanged, the root lengthened
    by as much), b_extra_us to sibling b."""
    rng = np.random.default_rng(seed)
    G = 100_000 + rng.integers(-10_000, 10_001, n_traces)
    root_own = 5_000 + rng.integers(0, 1_000, n_traces)
    t0 = T0_US + np.arange(n_traces) * 1_000_000
    ids = np.arange(1, 5 * n_traces + 1, dtype=np.uint64).reshape(n_traces, 5)
    pid = np.stack([np.zeros(n_traces, np.uint64), ids[:, 0], ids[:, 1], ids[:, 1], ids[:, 1]], 1)
    dur = np.stack([G + root_own + gateway_extra_us, G + gateway_extra_us, G * 9 // 10,
                    G // 2 + b_extra_us, G * 3 // 10], 1)
    gs = t0 + root_own // 2
    start = np.stack([t0, gs, gs + 1_000, gs + 1_000, gs + 1_000], 1)
    svc = np.tile(np.array([4, 3, 0, 1, 2], np.uint16), n_traces)
    ptr = np.arange(n_traces + 1, dtype=np.uint64) * 5
    return anomod.SpanSet(list(FANOUT_SERVICES), ptr, np.repeat(ids[:, 0], 5), ids.ravel(),
                          pid.ravel(), svc, np.zeros(5 * n_traces, np.uint16), dur.ravel(),
                          unique_ids=True, start_us=start.ravel())


# Hand-made traces: (name, span ids, parent ids, starts, durations, expected
# on_path, expected cp_us); starts are relative to T0_US unless absolute=True.
B64 = 2**64
HAND_CASES = [
    ("sequential children", [1, 2, 3], [0, 1, 1], [0, 10, 40], [100, 30, 50],
     [1, 1, 1], [20, 30, 50]),
    ("parallel fan-out", [1, 2, 3, 4], [0, 1, 1, 1], [0, 10, 10, 10], [100, 80, 50, 20],
     [1, 1, 0, 0], [20, 80, 0, 0]),
    ("partial overlap: the overlapped earlier child is skipped", [1, 2, 3], [0, 1, 1],
     [0, 10, 40], [100, 40, 50], [1, 0, 1], [50, 0, 50]),
    ("equal b: the lower position wins, the other is skipped", [1, 2, 3], [0, 1, 1],
     [0, 20, 50], [100, 60, 30], [1, 1, 0], [40, 60, 0]),
    ("child outlasting its parent", [1, 2], [0, 1], [0, 50], [100, 100], [1, 1], [50, 100]),
    ("child starting before its parent", [1, 2], [0, 1], [100, 50], [100, 100],
     [1, 1], [50, 100]),
    ("child entirely outside its parent", [1, 2], [0, 1], [0, 200], [100, 50], [1, 0], [100, 0]),
    ("zero-duration child", [1, 2], [0, 1], [0, 50], [100, 0], [1, 0], [100, 0]),
    ("2-cycle beside a real root", [1, 2, 3], [0, 3, 2], [0, 10, 15], [100, 20, 10],
     [1, 0, 0], [100, 0, 0]),
    ("self-reference with a child", [5, 6], [5, 5], [0, 10], [40, 20], [1, 1], [20, 20]),
    ("orphan head with a child", [7, 8], [999, 7], [0, 20], [60, 30], [1, 1], [30, 30]),
    ("duplicated id: the first carrier is the parent", [10, 10, 11], [0, 0, 10], [0, 0, 60],
     [100, 50, 30], [1, 1, 1], [70, 50, 30]),
    ("two roots", [1, 2, 3], [0, 0, 2], [0, 60, 70], [50, 40, 10], [1, 1, 1], [50, 30, 10]),
    ("s + dur past 2^64", [1, 2], [0, 1], [B64 - 10, B64 - 6], [100, 50], [1, 1], [95, 50],
     True),
]


def hand_set(S=3):
    """All HAND_CASES as one span set, one trace each -> (set, on_path, cp_us)."""
    lens, sid, pid, st, du, on, cp = [], [], [], [], [], [], []
    for case in HAND_CASES:
        _, ids, pids, starts, durs, e_on, e_cp = case[:7]
        base = 0 if len(case) > 7 else T0_US
        lens.append(len(ids))
        sid += ids
        pid += pids
        st += [base + x for x in starts]
        du += durs
        on += e_on
        cp += e_cp
    n = len(sid)
    ptr = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    sp = anomod.SpanSet([f"svc{i}" for i in range(S)], ptr,
                        np.repeat(np.arange(1, len(lens) + 1, dtype=np.uint64), lens),
                        np.asarray(sid, np.uint64), np.asarray(pid, np.uint64),
                        (np.arange(n) % S).astype(np.uint16),
                        (np.arange(n) % 5 == 0).astype(np.uint16), np.asarray(du, np.uint32),
                        start_us=np.asarray(st, np.uint64))
    return sp, np.asarray(on, np.uint8), np.asarray(cp, np.uint32)

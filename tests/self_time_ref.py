"""Reference for the self-time edge table (a plain helper, not a conftest).

The definition is restated in Python integers: the parent of a span is the
first span of its trace, in position order, whose span_id equals the span's
parent_span_id (a dict of first positions per trace); a root, an orphan and a
span whose first match is itself have none; self_us = dur_us - min(dur_us,
sum of the children's dur_us).  The table is the C oracle's edge table of the
same set with dur_us replaced by self_us (its edge rows depend only on ids).
Every result is an integer: GPU results are compared to it bit for bit."""
import numpy as np

import anomod
from anomod.spans import EdgeTable
from oracle import native

INT_FIELDS = ("count", "errors", "sum_us", "min_us", "max_us", "hist")
NO_PARENT = -1


def parents_ref(sp) -> np.ndarray:
    """par[i]: global position of span i's parent, NO_PARENT for a root, an
    orphan and a self-reference."""
    sid = sp.span_id.tolist()
    pid = sp.parent_span_id.tolist()
    ptr = sp.trace_ptr.tolist()
    par = np.full(sp.n_spans, NO_PARENT, np.int64)
    for t in range(sp.n_traces):
        first = {}
        for i in range(ptr[t], ptr[t + 1]):
            first.setdefault(sid[i], i)
        for i in range(ptr[t], ptr[t + 1]):
            if pid[i] == 0:          # ROOT
                continue
            j = first.get(pid[i])
            if j is None:            # ORPHAN
                continue
            if j == i:               # a span is not its own child
                continue
            par[i] = j
    return par


def self_us_ref(sp, par=None) -> np.ndarray:
    par = parents_ref(sp) if par is None else par
    dur = sp.dur_us.tolist()
    child_sum = [0] * sp.n_spans     # Python integers: no wrap
    for i, j in enumerate(par.tolist()):
        if j != NO_PARENT:
            child_sum[j] += dur[i]
    return np.asarray([d - min(d, c) for d, c in zip(dur, child_sum)], np.uint32)


def with_dur(sp, dur_us):
    """sp with another duration column."""
    return anomod.SpanSet(list(sp.services), sp.trace_ptr, sp.trace_hash, sp.span_id,
                          sp.parent_span_id, sp.svc, sp.flags,
                          np.ascontiguousarray(dur_us, np.uint32), sp.trace_ids, sp.unique_ids)


def self_table_ref(sp, self_us=None) -> dict:
    self_us = self_us_ref(sp) if self_us is None else self_us
    return native.finalize(native.edge_aggregate(with_dur(sp, self_us)))


def as_edge_table(tab: dict, services) -> EdgeTable:
    return EdgeTable(list(services), tab["count"], tab["errors"], tab["sum_us"], tab["min_us"],
                     tab["max_us"], tab["p50_us"], tab["p99_us"], tab["hist"])


def assert_table_equal(got: EdgeTable, ref: dict):
    for k in INT_FIELDS:
        np.testing.assert_array_equal(getattr(got, k), ref[k], err_msg=k)
    for k in ("p50_us", "p99_us"):
        np.testing.assert_array_equal(getattr(got, k), ref[k], err_msg=k)  # NaNs compare equal
        assert np.array_equal(getattr(got, k), ref[k], equal_nan=True), k


def class_shares(sp, self_us) -> tuple[float, float, float]:
    """Shares of the spans with self == 0, with 0 < self < dur, and with
    self == dur > 0."""
    s, d = self_us.astype(np.int64), sp.dur_us.astype(np.int64)
    n = max(1, sp.n_spans)
    zero = int((s == 0).sum())
    part = int(((s > 0) & (s < d)).sum())
    full = int(((s > 0) & (s == d)).sum())
    return zero / n, part / n, full / n


def add_delay(sp, service: str, d: int, par=None):
    """sp with d microseconds added to every span of `service` and, along the
    reference's parent chain, to every ancestor of such a span (an ancestor
    gains d once per delayed span of its subtree)."""
    par = parents_ref(sp) if par is None else par
    c = sp.services.index(service)
    gain = np.zeros(sp.n_spans, np.int64)
    plist = par.tolist()
    for i in np.nonzero(sp.svc == c)[0].tolist():
        j, steps = i, 0
        while j != NO_PARENT and steps <= sp.n_spans:   # (a reference cycle ends the walk)
            gain[j] += d
            j = plist[j]
            steps += 1
    dur = sp.dur_us.astype(np.int64) + gain
    assert dur.max() < 2**32
    return with_dur(sp, dur.astype(np.uint32))


def ancestors_and_descendants(sp, service: str, par=None) -> tuple[set, set]:
    """Services (other than `service`) holding a span above / below a span of
    `service` along the reference's parent chain."""
    par = parents_ref(sp) if par is None else par
    c = sp.services.index(service)
    svc = sp.svc.tolist()
    plist = par.tolist()
    anc, desc = set(), set()
    for i in range(sp.n_spans):
        j, steps, below = plist[i], 0, svc[i] == c
        while j != NO_PARENT and steps <= sp.n_spans:
            if below and svc[j] != c:
                anc.add(svc[j])
            if svc[j] == c and svc[i] != c:
                desc.add(svc[i])
            j = plist[j]
            steps += 1
    return anc, desc

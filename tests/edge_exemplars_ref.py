"""Reference for the edge exemplars (a plain helper, not a conftest).

Edge rows come from the C oracle (oracle.native.span_edges: the first-match
parent rule of the aggregation) and the in-trace mask is built as in
edge_load_ref.py.  Two forms of the definition of include/anomod.h
(anomod_edge_exemplars_spans) that must agree:

  exemplars_brute  per row, Python's sorted() over (-dur_us, position)
  exemplars_ref    one np.lexsort over (row, -dur_us, position) and a rank
                   inside each row

and `cascade_model`, the insertion the kernel performs on a row's K slots, as
a step machine a test drives under arbitrary schedules.

Every value is an integer: results are compared bit for bit."""
import numpy as np

from anomod.spans import EdgeExemplars, edge_rows
from oracle import native

FIELDS = ("n_found",) + EdgeExemplars.COLUMNS


def _rows(sp):
    """(edge row, qualifying-position mask of `which` = 0) per span position."""
    S = len(sp.services)
    edges = native.span_edges(sp, S).astype(np.int64) if sp.n_spans else np.zeros(0, np.int64)
    pos = np.arange(sp.n_spans)
    lo, hi = (int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])) if len(sp.trace_ptr) else (0, 0)
    return edges, (pos >= lo) & (pos < hi)


def _fill(ref, sp, row, slot, pos):
    """Write span positions `pos` into (row, slot) of the table."""
    pos = np.asarray(pos, np.int64)
    ref.position[row, slot] = pos.astype(np.uint64)
    # trace_ptr[t] <= pos < trace_ptr[t + 1]: the last t with trace_ptr[t] <= pos
    ref.trace[row, slot] = (np.searchsorted(sp.trace_ptr, pos.astype(np.uint64), side="right")
                            - 1).astype(np.uint64)
    ref.span_id[row, slot] = sp.span_id[pos]
    ref.dur_us[row, slot] = sp.dur_us[pos]
    ref.flags[row, slot] = sp.flags[pos]
    if sp.start_us is not None:
        ref.start_us[row, slot] = sp.start_us[pos]


def exemplars_brute(sp, k, which=0) -> EdgeExemplars:
    ref = EdgeExemplars.empty(sp.services, k, which)
    edges, ok = _rows(sp)
    if which:
        ok = ok & ((sp.flags & 1) != 0)
    per_row: dict[int, list] = {}
    for i in np.nonzero(ok)[0].tolist():
        per_row.setdefault(int(edges[i]), []).append((-int(sp.dur_us[i]), i))
    for r, items in per_row.items():
        top = [i for _, i in sorted(items)[:k]]
        ref.n_found[r] = len(top)
        _fill(ref, sp, r, np.arange(len(top)), top)
    return ref


def exemplars_ref(sp, k, which=0) -> EdgeExemplars:
    ref = EdgeExemplars.empty(sp.services, k, which)
    edges, ok = _rows(sp)
    if which:
        ok = ok & ((sp.flags & 1) != 0)
    pos = np.nonzero(ok)[0]
    if pos.size == 0:
        return ref
    row = edges[pos]
    order = np.lexsort((pos, -sp.dur_us[pos].astype(np.int64), row))
    pos, row = pos[order], row[order]
    first = np.r_[0, np.nonzero(np.diff(row))[0] + 1]          # start of each row's run
    rank = np.arange(pos.size) - np.repeat(first, np.diff(np.r_[first, pos.size]))
    keep = rank < k
    _fill(ref, sp, row[keep], rank[keep], pos[keep])
    np.add.at(ref.n_found, row[keep], 1)
    return ref


def assert_exemplars_equal(got: EdgeExemplars, ref: EdgeExemplars, fields=FIELDS):
    assert (got.k, got.which, got.services) == (ref.k, ref.which, ref.services)
    for name in fields:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        np.testing.assert_array_equal(a, b, err_msg=name)


def span_keys(durs, positions):
    """The kernel's key of a span: dur << 32 | (2^32 - 1 - position)."""
    return [(int(d) << 32) | (0xFFFFFFFF - int(p)) for d, p in zip(durs, positions)]


def cascade_model(keys, K, rng, concurrency, stale=True, peek=False):
    """The K slots after every key was inserted the way the kernel does it,
    with up to `concurrency` inserters in flight and the next step taken by one
    of them chosen at random.  A step is one memory operation: the read of
    a[K - 1] in front (a key below it is dropped), a read of the binary search
    for the first slot that may hold less than the key (a list is descending
    at every instant), or an atomicMax of the cascade from that slot on.  With
    `stale`, a read may return any value the slot held since the inserter
    started (slots only grow, so that is a smaller one).  With `peek` (the
    global lists) every slot of the cascade is read first, as a step of its
    own, and passed without the atomic when the read shows more than the key."""
    a = [0] * K
    history = [[0] for _ in range(K)]          # every value a slot ever held
    pending = list(keys)[::-1]
    live = []                                  # inserters: dicts of x, phase, lo, hi, i, marks

    def read(i, marks):
        if not stale:
            return a[i]
        return history[i][int(rng.integers(marks[i], len(history[i])))]

    while pending or live:
        while pending and len(live) < concurrency:
            live.append({"x": pending.pop(), "phase": "skip", "lo": 0, "hi": K - 1,
                         "marks": [len(h) - 1 for h in history]})
        j = int(rng.integers(len(live)))
        st = live[j]
        x = st["x"]
        done = False
        if st["phase"] == "skip":
            if x < read(K - 1, st["marks"]):
                done = True
            else:
                st["phase"] = "search"
        elif st["phase"] == "search":
            if st["lo"] < st["hi"]:
                mid = (st["lo"] + st["hi"]) // 2
                if read(mid, st["marks"]) > x:
                    st["lo"] = mid + 1
                else:
                    st["hi"] = mid
            if st["lo"] >= st["hi"]:
                st["phase"], st["i"] = "max", st["lo"]
        elif st["phase"] == "max" and peek and not st.get("peeked"):
            st["peeked"] = True
            if read(st["i"], st["marks"]) > x:
                st["i"], st["peeked"] = st["i"] + 1, False
                done = st["i"] == K
        elif st["phase"] == "max":
            i = st["i"]
            st["peeked"] = False
            old = a[i]                         # atomicMax: reads the slot as it is
            if old < x:
                a[i] = x
                history[i].append(x)
                st["x"] = old
            st["i"] = i + 1
            done = st["x"] == 0 or st["i"] == K
        if done:
            live.pop(j)
    for i in range(K - 1):                     # descending, empties last
        assert a[i] > a[i + 1] or a[i + 1] == 0
    return a

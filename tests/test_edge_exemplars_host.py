"""Edge exemplars, host side (no GPU): the two restatements of the definition
against each other, the cascade insertion under random schedules (the argument
csrc/edge_exemplars.hip rests on), the EdgeExemplars helpers and the ABI."""
import ctypes as C
import re

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import EdgeExemplars, edge_rows
from conftest import ROOT

from edge_exemplars_ref import (assert_exemplars_equal, cascade_model, exemplars_brute,
                                exemplars_ref, span_keys)

U32 = 2**32 - 1
U64 = 2**64 - 1


def chain_set(durs, svc=None, flags=None, S=2, trace_len=1, trace_ptr=None):
    """Spans in traces of `trace_len`: the first span of a trace is a root and
    every other one a child of the span before it."""
    n = len(durs)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    first = np.arange(n) % trace_len == 0
    parent = np.where(first, 0, ids - np.uint64(1)).astype(np.uint64)
    ptr = (np.r_[np.arange(0, n, trace_len), n].astype(np.uint64) if trace_ptr is None
           else np.asarray(trace_ptr, np.uint64))
    return anomod.SpanSet([f"s{i}" for i in range(S)], ptr, np.repeat(ids[first], trace_len)[:n],
                          ids, parent, np.zeros(n, np.uint16) if svc is None else svc,
                          np.zeros(n, np.uint16) if flags is None else flags,
                          np.asarray(durs, np.uint32), unique_ids=True)


def ties_set(n=6000):
    """Row ROOT -> s0: n root spans of one duration; row ROOT -> s1: n // 2
    spans whose durations take two values.  Positions interleave."""
    svc = (np.arange(n + n // 2) % 3 == 2).astype(np.uint16)
    durs = np.where(svc == 0, 777, np.where(np.arange(svc.size) % 2 == 0, 40, 41))
    return chain_set(durs, svc=svc)


def order_sets(K=8):
    """name -> set: every span inserts (ascending by position), none after the
    first K does (descending), the extremes of dur_us, and rows of exactly K
    and K - 1 spans."""
    n = 5000
    sets = {
        "ascending": chain_set(np.arange(1, n + 1)),
        "descending": chain_set(np.arange(n, 0, -1)),
        "extremes": chain_set(np.where(np.arange(n) % 7 == 3, U32, np.where(np.arange(n) % 5 == 1, 0, 9))),
    }
    svc = np.r_[np.zeros(K, np.uint16), np.ones(K - 1, np.uint16)]
    sets["k_and_k_minus_1"] = chain_set(np.arange(2 * K - 1) % 4, svc=svc)
    return sets


def cut_set():
    """trace_ptr[0] > 0 and spans after trace_ptr[-1]; the slowest spans lie outside."""
    n = 4101
    durs = np.arange(n) % 1000 + 1
    durs[[0, 1, 2, 4098, 4099, 4100]] = 10**6
    flags = (np.arange(n) % 11 == 0).astype(np.uint16)
    return chain_set(durs, svc=(np.arange(n) % 2).astype(np.uint16), flags=flags,
                     trace_ptr=[3, 4, 4, 2050, 4098])


@pytest.fixture(scope="module")
def sn_set():
    return anomod.synth_generate_host(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)


# ------------------------------------------------------------------ the references
def test_abi_has_the_entry_point():
    assert "anomod_edge_exemplars_spans" in anomod.EXPORTED_SYMBOLS
    assert hasattr(anomod.Context, "edge_exemplars")
    assert hasattr(anomod.lib(), "anomod_edge_exemplars_spans")
    assert L.STAGE_EDGE_EXEMPLARS == 14 and L.STAGE_EDGE_EXEMPLARS_KERNEL == 15
    assert L.ABI_VERSION == 2 and anomod.lib().anomod_abi_version() == 2


def test_struct_matches_the_header():
    text = (ROOT / "include" / "anomod.h").read_text()
    assert "#define ANOMOD_ABI_VERSION 2\n" in text
    body = re.search(r"typedef struct \{([^}]*)\} anomod_edge_exemplars;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint\d+_t)\s*(\*?)\s*(\w+);", body)
    ctype = {"uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    want = [(name, C.POINTER(ctype[t]) if star else ctype[t]) for t, star, name in fields]
    assert len(want) == 10
    assert [(n, t) for n, t in L.EdgeExemplarsC._fields_] == want


@pytest.mark.parametrize("which", [0, 1])
def test_brute_equals_lexsort_on_sn(sn_set, which):
    for k in (1, 8, 64):
        ref = exemplars_ref(sn_set, k, which)
        assert_exemplars_equal(ref, exemplars_brute(sn_set, k, which))
    if which == 0:
        assert ref.n_found.max() == 64 and (ref.n_found > 0).sum() > 10
    else:
        assert ref.n_found.sum() == int((sn_set.flags & 1).sum()) > 0  # fewer than 64 an edge
        assert (ref.flags[ref.position != U64] & 1).all()


def test_brute_equals_lexsort_on_the_crafted_sets():
    sets = dict(order_sets(), ties=ties_set(), cut=cut_set())
    for name, sp in sets.items():
        for which in (0, 1):
            ref = exemplars_ref(sp, 8, which)
            assert_exemplars_equal(ref, exemplars_brute(sp, 8, which))
    # ties go by position: the 8 smallest positions of the one-duration row
    ref = exemplars_ref(sets["ties"], 8)
    r0 = ref.row("ROOT", "s0")
    assert ref.position[r0].tolist() == [0, 1, 3, 4, 6, 7, 9, 10]
    r1 = ref.row("ROOT", "s1")
    assert (ref.dur_us[r1] == 41).all() and ref.position[r1].tolist() == sorted(ref.position[r1].tolist())
    # spans outside every trace are never exemplars
    cut = exemplars_ref(sets["cut"], 8)
    used = cut.position[cut.position != U64]
    assert used.min() >= 3 and used.max() < 4098 and cut.dur_us.max() <= 1000
    tp = sets["cut"].trace_ptr
    t = cut.trace[cut.position != U64].astype(np.int64)
    assert (tp[t] <= used).all() and (used < tp[t + 1]).all()
    # exactly K and K - 1 spans
    kk = exemplars_ref(sets["k_and_k_minus_1"], 8)
    assert kk.n_found[kk.row("ROOT", "s0")] == 8 and kk.n_found[kk.row("ROOT", "s1")] == 7
    assert (kk.position[kk.row("ROOT", "s1"), 7], kk.dur_us[kk.row("ROOT", "s1"), 7]) == (U64, 0)


# ------------------------------------------------------------------ the cascade
@pytest.mark.parametrize("concurrency", [1, 4, 64])
@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_cascade(concurrency, order):
    """Whatever the schedule, the K slots end as the sorted top K: slot values
    only grow, and a value passes slot i only after it met something larger in
    every slot before it."""
    rng = np.random.default_rng(concurrency * 7 + len(order))
    for K in (1, 2, 3, 8):
        for n in (K - 1, K, 200):
            for trial in range(8):
                durs = rng.integers(0, 6, n)          # many ties: decided by position
                keys = span_keys(durs, np.arange(n))
                assert len(set(keys)) == n and (n == 0 or min(keys) >= 1)
                if order == "ascending":
                    keys.sort()
                elif order == "descending":
                    keys.sort(reverse=True)
                else:
                    keys = [keys[i] for i in rng.permutation(n)]
                got = cascade_model(keys, K, rng, concurrency, stale=bool(trial % 2),
                                    peek=bool(trial // 2 % 2))
                want = sorted(keys, reverse=True)[:K]
                assert got == want + [0] * (K - len(want)), (K, n, trial)


# ------------------------------------------------------------------ the helpers
def test_helpers(sn_set):
    ex = exemplars_ref(sn_set, 4)
    S = sn_set.n_services
    svcs = sn_set.services
    assert ex.row("ROOT", svcs[3]) == S * S + 3
    assert ex.row("ORPHAN", svcs[0]) == (S + 1) * S
    assert ex.row(svcs[2], svcs[5]) == 2 * S + 5
    table = anomod.EdgeTable.empty(svcs)
    for p in (0, S, S + 1):
        assert ex.row(table.parent_name(p), svcs[1]) == p * S + 1
    with pytest.raises(ValueError):
        ex.row("no-such-service", svcs[0])
    row = int(np.argmax(ex.n_found))
    assert ex.n_found[row] == 4
    idx = ex.trace_indices(row)
    assert idx.dtype == np.int64 and idx.tolist() == ex.trace[row].tolist()
    # without SpanSet.trace_ids: the trace hash of the trace's first span
    assert sn_set.trace_ids is None
    first = sn_set.trace_ptr[idx].astype(np.int64)
    assert ex.trace_ids(sn_set, row) == [f"{int(h):016x}" for h in sn_set.trace_hash[first]]
    # with them
    named = sn_set.select_traces(np.ones(sn_set.n_traces, bool))
    named.trace_ids = [f"trace-{t}" for t in range(named.n_traces)]
    assert ex.trace_ids(named, row) == [f"trace-{t}" for t in idx.tolist()]
    # select: the exemplar traces, whole, in trace order
    sel = ex.select(named, row)
    uniq = sorted(set(idx.tolist()))
    assert sel.trace_ids == [f"trace-{t}" for t in uniq]
    assert sel.n_spans == sum(int(sn_set.trace_ptr[t + 1] - sn_set.trace_ptr[t]) for t in uniq)
    assert set(ex.span_id[row].tolist()) <= set(sel.span_id.tolist())
    # a row without spans
    none = int(np.argmin(ex.n_found))
    assert ex.n_found[none] == 0 and ex.trace_ids(named, none) == []
    assert ex.select(named, none).n_traces == 0


def test_empty_table():
    ex = EdgeExemplars.empty(["a", "b"], 3, 1)
    E = edge_rows(2)
    assert (ex.k, ex.which) == (3, 1) and ex.n_found.shape == (E,) and not ex.n_found.any()
    assert ex.position.shape == (E, 3) and (ex.position == U64).all() and (ex.trace == U64).all()
    for name, dt in (("span_id", np.uint64), ("dur_us", np.uint32), ("flags", np.uint16),
                     ("start_us", np.uint64)):
        a = getattr(ex, name)
        assert a.dtype == dt and a.shape == (E, 3) and not a.any()

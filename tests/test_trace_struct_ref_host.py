"""The trace-structure model of trace_struct_ref.py against the reference
goldens and against the C oracle (oracle_trace_structure) on every builder
the GPU test uses, and the premises of those builders (no GPU).

The model and the oracle share no method: the oracle scans the trace per span
and relaxes the depth edges until nothing changes (at most 2L + 2 sweeps, then
d < L); the model uses dicts, reachability and Kahn's order.  Where they
agree, the oracle's bounded relaxation is shown to implement the definition
in include/anomod.h (0 when no root reaches the node or a reached cycle feeds
it), which agreement between the oracle and the kernels alone does not show."""
import numpy as np
import pytest

import trace_struct_ref as R
from oracle import native
from test_trace_structure import GOLDENS, _check_against_reference, _golden_set, _random_set

CASES = R.case_names()


def _assert_equal(got, ref, what):
    for k in R.FIELDS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("name", GOLDENS)
def test_model_matches_reference_build_span_records(golden, name):
    sp, kept = _golden_set(golden, name)
    _check_against_reference(sp, kept, R.trace_structure_ref(sp))


@pytest.mark.parametrize("seed", [5, 6])
def test_model_matches_oracle_on_random_sets(seed):
    sp = _random_set(np.random.default_rng(seed), 70, 400, 60)
    _assert_equal(R.trace_structure_ref(sp), native.trace_structure(sp), f"seed {seed}")


def test_model_counts_span_id_zero_as_an_id():
    """Builders never make span id 0 (reserved), but decoded data may hold it
    (test_long_traces.py sets some): it is an id like any other, while a
    parent reference of 0 names nothing."""
    sp = _random_set(np.random.default_rng(7), 5, 200, 30)
    sp.span_id[np.random.default_rng(8).random(sp.n_spans) < 0.05] = 0
    _assert_equal(R.trace_structure_ref(sp), native.trace_structure(sp), "id 0")


@pytest.mark.parametrize("name", CASES)
def test_model_matches_oracle(name):
    c = R.case(name)
    _assert_equal(c.model, native.trace_structure(c.sp), name)


def test_case_list():
    """Every shape in every regime that applies to it; shapes that hold a
    duplicated id by construction in D alone."""
    assert len(CASES) == len(set(CASES))
    shapes = {n.rsplit("-", 1)[0] for n in CASES}
    assert shapes == set(R.SHAPES)
    for s in shapes:
        reg = {n.rsplit("-", 1)[1] for n in CASES if n.rsplit("-", 1)[0] == s}
        assert reg == {"D"} or {"U", "G"} <= reg, (s, reg)
        if s != "pack_only_empty" and reg != {"D"}:
            assert "Din" in reg, s
    for kind in ("fwd", "rev", "shuf"):
        for L in (1, 2, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8193):
            assert f"chain_{kind}_{L}-U" in CASES
    # the chunk-path chains that leave room for a second trace come in Dout too
    assert "chain_rev_129-Dout" in CASES and "chain_rev_255-Dout" not in CASES


@pytest.mark.parametrize("name", CASES)
def test_builder_premises(name):
    c = R.case(name)
    sp, f, m = c.sp, c.facts, c.model
    sl = c.target_slice()
    L = sl.stop - sl.start
    # the regime is what it says
    declared = sp.unique_ids
    assert declared == (c.regime == "U")
    try:  # check_unique_ids() sets the flag of the cached set
        assert sp.check_unique_ids() == (c.regime in ("U", "G"))
    finally:
        sp.unique_ids = declared
    assert not (sp.span_id == 0).any()
    lens = np.diff(sp.trace_ptr.astype(np.int64))
    # where the device runs the shape: all of it in the dynamic tail, one run
    chunks = R.tail_chunks(lens.tolist())
    if name.startswith(("many_long", "pack_only_empty")):
        assert c.first == 0
    else:
        assert c.first == sp.n_traces - sp.n_traces // 2 == chunks[0][0]
        assert sp.n_traces - c.first <= R.DYN_SEG and c.target >= c.first
        assert (lens[:c.first] == 1).all()
    mine = [ch for ch in chunks if ch[0] <= c.target < ch[0] + max(ch[1], 1)]
    assert len(mine) == 1
    if "chunks" in f and c.regime in ("U", "G"):
        assert [(k, n) for _, k, n in chunks] == f["chunks"]
    if c.regime == "Dout":  # the added trace shares the target's chunk
        assert mine[0][0] <= c.target - 1 and mine[0][1] >= 2
        d = int(sp.trace_ptr[c.target - 1])
        assert lens[c.target - 1] == 2 and sp.span_id[d] == sp.span_id[d + 1]
        assert np.unique(sp.span_id).shape[0] == sp.n_spans - 1
    if c.regime == "Din":
        ids = sp.span_id[sl]
        assert np.unique(ids).shape[0] == L - 1 and ids[-1] in ids[:-1]
    depth = m["depth"][sl].astype(np.int64)
    if "max_depth" in f:
        assert int(depth.max()) == f["max_depth"]
    if "n_roots" in f:
        assert int(m["n_roots"][c.target]) == f["n_roots"]
    if "depth" in f:
        np.testing.assert_array_equal(depth[:len(f["depth"])], f["depth"])
    if "zero" in f:
        assert not depth[f["zero"]].any()
    if "len" in f:
        assert L == f["len"]
    if "set_spans" in f:
        assert sp.n_spans == f["set_spans"]
    if "empty_traces" in f:  # at the start, in the middle and at the end of the target's chunk
        t0, k, _ = mine[0]
        mid = lens[t0 + 1:t0 + k - 1]
        assert int((lens == 0).sum()) == f["empty_traces"]
        assert lens[t0] == 0 and lens[t0 + k - 1] == 0 and (mid == 0).any() and (mid > 0).any()
    if "reached" in f:  # a root reaches the cycle: its depths are 0 by the cycle rule
        reach = R.reachable_positions(sp.span_id[sl], sp.parent_span_id[sl])
        assert set(f["reached"]) <= set(reach)
        assert int(m["n_roots"][c.target]) >= 1
    if "entry_parent" in f:
        a = f["max_depth"] + 1  # the entry node's first span follows the chain
        assert int(m["parent_pos"][sl][a]) == f["entry_parent"]
    if "parent_at" in f:
        for pos, par in f["parent_at"].items():
            assert int(m["parent_pos"][sl][pos]) == par
    if "children_at" in f:
        for pos, k in f["children_at"].items():
            assert int(m["n_children"][sl][pos]) == k
    if "windows" in f:  # the duplicated id sits in two table windows of one long trace
        assert L > 2 * R.BIG_WIN
        for x, pos in f["windows"]:
            at = np.nonzero(sp.span_id[sl] == np.uint64(x))[0].tolist()
            assert at == pos and at[0] // R.BIG_WIN != at[-1] // R.BIG_WIN
            fl = m["span_flags"][sl]
            assert fl[at[0]] & R.SPAN_FIRST and not fl[at[-1]] & R.SPAN_FIRST
            assert int(m["n_children"][sl][at[0]]) >= 2  # referenced: pf must be the first
    if "cluster" in f:
        slot, size = f["cluster"]
        assert L > R.STAGE and L <= R.BIG_WIN  # one window of the long-trace table
        assert size >= 40 and int((R.big_slot(sp.span_id[sl]) == slot).sum()) >= size
        assert slot == R.BIG_SLOTS - 1 and (R.big_slot(sp.span_id[sl]) < 40).sum() >= 40
    if "low_twins" in f:
        i, j = f["low_twins"]
        ids = sp.span_id[sl]
        assert ids[i] != ids[j] and (int(ids[i]) ^ int(ids[j])) & 0xFFFFFFFF == 0
    if "svc_present" in f:
        words = m["svc_mask"].shape[1]
        assert words == (len(sp.services) + 63) // 64
        have = np.bitwise_or.reduce(m["svc_mask"], axis=0)
        bits = [w * 64 + b for w in range(words) for b in range(64) if (int(have[w]) >> b) & 1]
        assert bits == f["svc_present"]
        assert len({tuple(r) for r in m["svc_mask"].tolist()}) > 1 or len(bits) == 1
    if "long_traces" in f:
        n_long = int((lens > R.STAGE).sum())
        assert n_long == f["long_traces"] > 2 * R.MI355X_CUS
        assert lens[-1] > R.STAGE and (np.diff(lens[lens > R.STAGE]) != 0).all()
        assert 150_000 < sp.n_spans < 190_000


def test_big_slot_restates_the_multiply_shift():
    for x in (1, 0x9E3779B97F4A7C15, 2**64 - 1, 0x0123456789ABCDEF):
        want = ((x * 0x9E3779B97F4A7C15) % 2**64) >> 51
        assert int(R.big_slot(np.array([x], np.uint64))[0]) == want

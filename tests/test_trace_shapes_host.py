"""CPU: properties of the trace shape model (tests/trace_shapes_ref.py) and of
the Python pieces around the census (TraceShapes.novel / service_sets /
novelty, the features() flag, the CLI flag, the exported symbol)."""
import ctypes as C
import inspect
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import TraceShapes
from conftest import PKG_DIR

from self_time_ref import parents_ref
from trace_shapes_ref import (SEED_ORPHAN, SEED_ROOT, SEED_SELF, B, M64, census_ref, chain,
                              from_trees, jump_ref, label_keys, mix64, novelty_ref,
                              path_hash_ref, random_tree, shapes_ref, shuffled, without_subtrees)


def _shape1(tree, **kw):
    return int(shapes_ref(from_trees([tree]), **kw)[0])


# ------------------------------------------------------------------ surface
def test_library_exports_the_entry_point():
    assert "anomod_trace_shapes_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    cs = L.TraceShapesC(1)
    assert lib.anomod_trace_shapes_spans(None, None, C.byref(cs)) == L.EINVAL
    assert b"anomod_trace_shapes_spans" in lib.anomod_last_error(None)


def test_python_surface():
    p = inspect.signature(anomod.features).parameters
    assert "shapes" in p and p["shapes"].default is False
    assert "shapes" in anomod.Features.__dataclass_fields__
    q = inspect.signature(anomod.Context.trace_shapes).parameters
    assert list(q)[1:] == ["spans", "trace_class", "use_errors", "cap", "per_trace", "per_span",
                           "svc_key"]
    assert q["svc_key"].default == "names" and q["use_errors"].default is False
    assert anomod.TraceShapes is TraceShapes


def test_cli_lists_the_flag():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--shapes" in r.stdout


# ------------------------------------------------------------------ the model
def test_definition_on_a_small_tree():
    """root(0) -> a(1) -> b(2), worked by hand from the definition."""
    sp = from_trees([[(1, 0, 0), (2, 1, 1), (3, 2, 2)]])
    K = label_keys(sp)
    p0 = (SEED_ROOT * B + K[0]) & M64
    p1 = (p0 * B + K[1]) & M64
    p2 = (p1 * B + K[2]) & M64
    P, on = path_hash_ref(sp)
    assert P.tolist() == [p0, p1, p2] and on.all()
    assert int(shapes_ref(sp)[0]) == (mix64(p0) + mix64(p1) + mix64(p2)) & M64
    assert label_keys(sp, svc_key=None) == [mix64(1), mix64(2), mix64(3)]


def test_permutation_invariance_with_unique_ids():
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=5, p_orphan_ppm=20000), 300)
    a = shapes_ref(sp)
    for seed in (1, 2):
        np.testing.assert_array_equal(shapes_ref(shuffled(sp, seed)), a)
    assert np.unique(a).shape[0] > 3


def test_equal_label_siblings_share_children():
    """A->(B->C, B->D) == A->(B->(C, D), B); another leaf label differs."""
    split = [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 3, 3)]
    joined = [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 2, 3)]
    other = [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 2, 4)]
    deeper = [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 4, 3)]   # D below C
    assert _shape1(split) == _shape1(joined)
    assert len({_shape1(joined), _shape1(other), _shape1(deeper)}) == 3


def test_head_kinds_differ():
    root, orphan, own = [(7, 0, 0)], [(7, 99, 0)], [(7, 7, 0)]
    got = [_shape1(t) for t in (root, orphan, own)]
    assert len(set(got)) == 3
    K = label_keys(from_trees([root]))[0]
    assert got == [mix64(s * B + K) for s in (SEED_ROOT, SEED_ORPHAN, SEED_SELF)]


def test_cycle_and_its_tail_are_off_the_tree():
    """1 <-> 2 reference each other, 3 hangs off 2, 4 is a root with child 5."""
    sp = from_trees([[(1, 2, 0), (2, 1, 1), (3, 2, 2), (4, 0, 0), (5, 4, 1)]])
    P, on = path_hash_ref(sp)
    assert on.tolist() == [False, False, False, True, True] and not P[:3].any()
    assert int(shapes_ref(sp)[0]) == _shape1([(4, 0, 0), (5, 4, 1)])
    Pj, onj, _ = jump_ref(sp)
    np.testing.assert_array_equal(Pj, P)
    np.testing.assert_array_equal(onj, on)
    # a trace with nothing on the tree, and an empty one: shape 0
    sp = from_trees([[(1, 2, 0), (2, 1, 1)], [], [(3, 0, 0)]], S=2)
    assert shapes_ref(sp).tolist()[:2] == [0, 0]


def test_duplicated_ids_follow_the_first_match():
    """Two spans carry id 2: the child (id 3) hangs below the first of them."""
    first_b = [(1, 0, 0), (2, 1, 1), (2, 1, 2), (3, 2, 3)]
    first_c = [(1, 0, 0), (2, 1, 2), (2, 1, 1), (3, 2, 3)]
    sp = from_trees([first_b, first_c], unique=False)
    par = parents_ref(sp)
    assert par[3] == 1 and par[7] == 5
    a, b = shapes_ref(sp).tolist()
    assert a != b
    assert a == _shape1([(1, 0, 0), (2, 1, 1), (4, 1, 2), (3, 2, 3)])


def test_use_errors_changes_only_flagged_traces():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=2, p_error_ppm=50000), 500)
    plain, err = shapes_ref(sp), shapes_ref(sp, use_errors=True)
    flagged = np.zeros(sp.n_traces, bool)
    flagged[sp.trace_of_span()[(sp.flags & 1) != 0]] = True
    assert 0 < flagged.sum() < sp.n_traces
    np.testing.assert_array_equal(plain != err, flagged)


def test_jumping_form_equals_the_sequential_definition():
    rng = np.random.default_rng(11)
    sp = random_tree(rng, rng.integers(1, 80, 200), orphan=0.05, self_ref=0.02)
    # duplicated ids and cycles: overwrite some ids / references inside traces
    sid, pid = sp.span_id.copy(), sp.parent_span_id.copy()
    ptr = sp.trace_ptr.astype(np.int64)
    for t in range(0, 200, 3):
        a, b = ptr[t], ptr[t + 1]
        if b - a >= 4:
            sid[a + 1] = sid[a + 2]                 # a duplicated id
            pid[a], pid[a + 3] = sid[a + 3], sid[a]  # a 2-cycle
    sp = anomod.SpanSet(sp.services, sp.trace_ptr, sid, sid, pid, sp.svc, sp.flags, sp.dur_us)
    P, on = path_hash_ref(sp, use_errors=True)
    Pj, onj, _ = jump_ref(sp, use_errors=True)
    assert 0 < (~on).sum() < sp.n_spans
    np.testing.assert_array_equal(onj, on)
    np.testing.assert_array_equal(Pj, P)


@pytest.mark.parametrize("N,rounds", [(256, 8), (257, 9)])
def test_rounds_a_chain_needs(N, rounds):
    sp = from_trees([chain(N)])
    P, on = path_hash_ref(sp)
    Pj, onj, used = jump_ref(sp, max_rounds=64)
    assert used == rounds and onj.all()
    np.testing.assert_array_equal(Pj, P)
    _, short, _ = jump_ref(sp, max_rounds=rounds - 1)
    assert not short.all()


# ------------------------------------------------------------------ census
def test_census_order_with_count_ties():
    shape = np.array([9, 5, 9, 7, 5, 3, 9, 7], np.uint64)
    cls = np.array([0, 1, 1, 0, 2, 0, 0, 0], np.uint8)
    c = census_ref(shape, cls)
    assert c.shape.tolist() == [9, 5, 7, 3]            # 3, then the tie 5 < 7, then 1
    assert c.count.tolist() == [3, 2, 2, 1]
    assert c.abnormal.tolist() == [1, 2, 0, 0]
    assert c.first_trace.tolist() == [0, 1, 3, 5]
    big = np.array([1 << 63, 1, 1 << 63, 1], np.uint64)    # ties by unsigned value
    assert census_ref(big).shape.tolist() == [1, 1 << 63]


def _census(services, shape, count, first, n_shapes=None):
    u = lambda a: np.asarray(a, np.uint64)  # noqa: E731
    return TraceShapes(list(services), u(shape), u(count), u(np.zeros(len(shape))), u(first),
                       len(shape) if n_shapes is None else n_shapes, 0)


def test_novel_and_novelty_on_hand_made_censuses():
    # traces: 0 = {a, b}, 1 = {a}, 2 = {b, c}, 3 = {a}
    sp = from_trees([[(1, 0, 0), (2, 1, 1)], [(3, 0, 0)], [(4, 0, 1), (5, 4, 2)], [(6, 0, 0)]],
                    S=4)
    cur = _census(sp.services, [10, 20, 30], [5, 3, 2], [0, 1, 2])
    base = _census(sp.services, [20, 99], [7, 1], [0, 1])
    np.testing.assert_array_equal(cur.novel(base), [True, False, True])
    np.testing.assert_array_equal(cur.service_sets(sp),
                                  [[1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0]])
    # a: (5) / (5 + 3); b: (5 + 2) / (5 + 2); c: 2 / 2; d: in no exemplar
    np.testing.assert_array_equal(cur.novelty(sp, base), [5 / 8, 1.0, 1.0, 0.0])
    np.testing.assert_array_equal(cur.novelty(sp, cur), np.zeros(4))
    assert not cur.truncated and not cur.novel(cur).any()
    cut = _census(sp.services, [20], [7], [0], n_shapes=2)
    assert cut.truncated
    with pytest.raises(ValueError, match="truncated"):
        cur.novel(cut)
    with pytest.raises(ValueError, match="truncated"):
        cur.novelty(sp, cut)
    assert cut.novel(base).tolist() == [False]       # a truncated census may still ask


def test_removed_subtrees_make_novel_shapes_in_the_model():
    """The construction of the features() test, on the model alone: the
    altered traces, and only they, have shapes the baseline lacks."""
    base = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=4), 600)
    cur, altered = without_subtrees(base, "home-timeline-service")
    assert 10 <= altered.sum() <= 60 and cur.n_spans < base.n_spans
    sb, sc = shapes_ref(base), shapes_ref(cur)
    np.testing.assert_array_equal(~np.isin(sc, sb), altered)
    nov = novelty_ref(cur, sc, sb)
    in_altered = np.zeros(cur.n_services, bool)
    in_altered[cur.svc[np.repeat(altered, np.diff(cur.trace_ptr).astype(np.int64))]] = True
    np.testing.assert_array_equal(nov > 0, in_altered)
    # TraceShapes.novelty is that formula
    c = census_ref(sc)
    got = TraceShapes(list(cur.services), c.shape, c.count, c.abnormal, c.first_trace,
                      c.shape.shape[0], 0).novelty(
        cur, _census(base.services, np.unique(sb), np.ones(np.unique(sb).shape[0]),
                     np.zeros(np.unique(sb).shape[0])))
    np.testing.assert_array_equal(got, nov)


def test_cli_shapes_object():
    from anomod.__main__ import shapes_doc
    sp = from_trees([[(1, 0, 0), (2, 1, 1)], [(3, 0, 0)], [(4, 0, 1), (5, 4, 2)], [(6, 0, 0)]],
                    S=4)
    cur = _census(sp.services, [10, 1 << 63, 30], [5, 3, 2], [0, 1, 2])
    cur.off_tree_spans = 4
    base = _census(sp.services, [1 << 63], [7], [0])
    doc = shapes_doc(cur, sp, base, top=2)
    assert doc["distinct"] == 3 and doc["off_tree_spans"] == 4 and len(doc["top"]) == 2
    assert doc["top"][0] == {"shape": "000000000000000a", "count": 5, "abnormal": 0,
                             "exemplar_trace": 0, "exemplar_spans": 2,
                             "services": ["svc00", "svc01"], "new": True}
    assert doc["top"][1]["shape"] == "8000000000000000" and doc["top"][1]["new"] is False
    assert [r["new"] for r in shapes_doc(cur, sp)["top"]] == [None, None, None]
    import json
    json.dumps(doc)

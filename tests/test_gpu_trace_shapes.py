"""GPU: the trace shape census (csrc/trace_shapes.hip) against the exact host
model (tests/trace_shapes_ref.py), bit for bit — trace_shape, path_hash,
off_tree_spans and the whole census with its order — plus argument handling,
what the call leaves unchanged, and the novelty term through features()."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.engine import Experiment

from trace_shapes_ref import (B, M64, SEED_ROOT, census_ref, chain, from_trees, mix64,
                              novelty_ref, path_hash_ref, random_tree, service_keys, shapes_ref,
                              shuffled, spanset, without_subtrees)
from trace_shapes_ref import label_keys
from test_gpu_self_time import window_border_case

pytestmark = pytest.mark.gpu


def _ref(sp, **kw):
    P, on = path_hash_ref(sp, **kw)
    return P, on, shapes_ref(sp, P, on)


def _assert_census(got, shape, trace_class=None, cap=None):
    c = census_ref(shape, trace_class)
    k = c.shape.shape[0] if cap is None else min(cap, c.shape.shape[0])
    assert got.n_shapes == c.shape.shape[0]
    assert got.truncated == (k < got.n_shapes)
    for name in ("shape", "count", "abnormal", "first_trace"):
        np.testing.assert_array_equal(getattr(got, name), getattr(c, name)[:k], err_msg=name)


def _check(ctx, sp, dev=None, ref=None, trace_class=None, use_errors=False, svc_key="names"):
    """Everything the call returns for `sp` (or its device twin) == the model."""
    P, on, shape = _ref(sp, use_errors=use_errors, svc_key=svc_key) if ref is None else ref
    got = ctx.trace_shapes(sp if dev is None else dev, trace_class=trace_class,
                           use_errors=use_errors, per_trace=True, per_span=True, svc_key=svc_key)
    np.testing.assert_array_equal(got.path_hash, P, err_msg="path_hash")
    np.testing.assert_array_equal(got.trace_shape, shape, err_msg="trace_shape")
    lo, hi = int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])
    assert got.off_tree_spans == int((~on[lo:hi]).sum())
    _assert_census(got, shape, trace_class)
    return got


# ------------------------------------------------------------------ hand-made
def test_hand_made_traces(ctx):
    trees = [
        [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 3, 3)],      # A->(B->C, B->D)
        [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 2, 3)],      # A->(B->(C, D), B)
        [(1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (5, 2, 4)],      # another leaf
        [(7, 0, 0)], [(7, 99, 0)], [(7, 7, 0)],                       # ROOT / ORPHAN / SELF
        [(1, 2, 0), (2, 1, 1), (3, 2, 2), (4, 0, 0), (5, 4, 1)],      # 2-cycle + tail + a tree
        [(1, 2, 0), (2, 1, 1)],                                       # nothing on the tree
        [],
        [(1, 0, 0), (2, 1, 1), (2, 1, 2), (3, 2, 3)],                 # duplicated id: first match
        [(1, 0, 0), (2, 1, 2), (2, 1, 1), (3, 2, 3)],
        [(5, 4, 1), (4, 0, 0)],                                       # the child first
    ]
    sp = from_trees(trees, unique=False)
    got = _check(ctx, sp, trace_class=np.arange(len(trees)) % 2)
    ts = got.trace_shape.tolist()
    assert ts[0] == ts[1] and ts[2] != ts[1]
    assert len(set(ts[3:6])) == 3
    key = service_keys(sp)[0]
    assert ts[3] == mix64((SEED_ROOT * B + key) & M64)
    assert got.off_tree_spans == 5 and ts[7] == 0 and ts[8] == 0
    assert ts[9] != ts[10] and ts[6] == ts[11]
    assert not got.path_hash[[18, 19, 20, 23, 24]].any()
    _check(ctx, sp, use_errors=True, svc_key=None)


# ------------------------------------------------------------------ synthetic sets
@pytest.fixture(scope="module", params=["SN", "TT"])
def synth_case(request):
    sp = anomod.synth_generate_host(anomod.SynthSpec(request.param, seed=1, p_orphan_ppm=2000),
                                    2000)
    return request.param, sp, _ref(sp)


def test_synthetic_declared_unique(ctx, synth_case, monkeypatch, capfd):
    """As generated (unique ids, collector order): the scans from both ends."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    topo, sp, ref = synth_case
    assert sp.unique_ids
    got = _check(ctx, sp, ref=ref)
    want = {"SN": "trace_shapes_kernel<bidir>", "TT": "trace_shapes_kernel<split>"}[topo]
    assert want + ", 0 long traces" in capfd.readouterr().err
    assert 3 <= got.n_shapes < sp.n_traces and int(got.count.sum()) == sp.n_traces
    assert got.off_tree_spans == 0


def test_synthetic_not_declared_unique(ctx, synth_case, monkeypatch, capfd):
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    _, sp, ref = synth_case
    plain = sp.take(np.arange(sp.n_spans), sp.trace_ptr)
    plain.unique_ids = False
    _check(ctx, plain, ref=ref)
    assert "trace_shapes_kernel<forward>" in capfd.readouterr().err


def test_synthetic_shuffled_inside_traces(ctx, synth_case):
    """Children before parents: other path_hash positions, the same shapes."""
    _, sp, (_, _, shape) = synth_case
    sh = shuffled(sp, seed=5)
    assert sh.unique_ids and not np.array_equal(sh.span_id, sp.span_id)
    got = _check(ctx, sh)
    np.testing.assert_array_equal(got.trace_shape, shape)
    np.testing.assert_array_equal(np.sort(got.trace_shape), np.sort(shape))


def test_synthetic_use_errors_and_classes(ctx, synth_case):
    topo, sp, _ = synth_case
    cls = (np.arange(sp.n_traces) % 3 == 0).astype(np.uint8) * 7     # any non-zero value
    got = _check(ctx, sp, trace_class=cls, use_errors=True)
    assert 0 < int(got.abnormal.sum()) == int((cls != 0).sum())
    _check(ctx, sp, svc_key=None)
    # keys of the caller's own, at the C ABI
    keys = np.arange(1, sp.n_services + 1, dtype=np.uint64) * np.uint64(0x100000001B3)
    shape = np.zeros(sp.n_traces, np.uint64)
    d = ctx.upload(sp)
    try:
        cs = L.TraceShapesC(sp.n_services, 0, L.ptr(keys, C.c_uint64), None, 0, 0, 0, None, None,
                            None, None, L.ptr(shape, C.c_uint64), None)
        assert anomod.lib().anomod_trace_shapes_spans(ctx.handle, d.handle, C.byref(cs)) == L.OK
    finally:
        d.free()
    np.testing.assert_array_equal(shape, shapes_ref(sp, svc_key=keys))
    assert cs.n_shapes == np.unique(shape).shape[0]


def test_device_generated_set(ctx):
    """2^14 traces generated on the device; compared after the download."""
    d = ctx.generate(anomod.SynthSpec("SN", seed=3, p_orphan_ppm=2000), 1 << 14)
    try:
        host = d.download()
        assert host.n_traces == 1 << 14
        got = _check(ctx, host, dev=d)
        assert got.n_shapes > 3
    finally:
        d.free()


# ------------------------------------------------------------------ hand-built shapes
def test_sixty_five_one_span_traces(ctx):
    """More one-span traces than a chunk's 64; every span is a head.  (The
    share policy packs only the last 16 of them into one chunk: the 64-trace
    limit itself is met in test_gpu_walk_borders.py.)"""
    n = 65
    sp = spanset(3, [1] * n, np.arange(1, n + 1), np.zeros(n))
    got = _check(ctx, sp)
    assert got.n_shapes == 3 and got.count.tolist() == [22, 22, 21]
    assert got.shape[0] < got.shape[1] and got.first_trace.tolist()[2] == 2


@pytest.mark.parametrize("kind", ["tree", "chain"])
@pytest.mark.parametrize("L_", [256, 257])
def test_trace_at_the_chunk_limit(ctx, L_, kind, monkeypatch, capfd):
    """A random tree and a pure chain at 256 (one chunk, all 8 rounds for the
    chain) and at 257 spans (long-trace kernel, 9 rounds), between short
    traces (each of the three a chunk of its own: no dynamic tail, nothing is
    packed)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    if kind == "tree":
        sp = random_tree(np.random.default_rng(31), [3, L_, 3], self_ref=0.01)
    else:
        sp = from_trees([chain(3, 1), chain(L_, 10), chain(3, 1000)], unique=True)
    got = _check(ctx, sp)
    assert f", {L_ - 256} long traces" in capfd.readouterr().err
    assert got.off_tree_spans == 0
    if kind == "chain":
        assert got.n_shapes == 2 and got.count.tolist() == [2, 1]


def test_long_chain_and_long_tree(ctx, monkeypatch, capfd):
    """A shuffled 5,000-span chain (13 rounds) and a 5,000-span random tree."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    ch = shuffled(from_trees([chain(5000, 1, S=9)], S=9), seed=3)
    tr = random_tree(np.random.default_rng(21), [5000])
    sid = np.r_[ch.span_id, tr.span_id]
    sp = spanset(9, [5000, 5000], sid, np.r_[ch.parent_span_id, tr.parent_span_id],
                 np.r_[ch.svc, tr.svc], np.r_[ch.flags, tr.flags])
    _check(ctx, sp, use_errors=True)
    assert "trace_shapes_kernel<forward>, 2 long traces" in capfd.readouterr().err


def test_cycle_in_a_long_trace(ctx):
    """700 spans: a 300-span reference cycle, a 100-span chain hanging off it,
    and a 300-span tree; the cycle and its tail are off the tree."""
    cyc = [(1 + k, 1 + (k + 1) % 300, k % 4) for k in range(300)]
    tail = [(1000 + k, 1000 + k - 1 if k else 17, k % 3) for k in range(100)]
    tree = [(5000 + k, 5000 + (k - 1) // 2 if k else 0, k % 5) for k in range(300)]
    sp = shuffled(from_trees([[(9, 0, 0)], cyc + tail + tree, [(9, 0, 1)]], unique=True), seed=8)
    got = _check(ctx, sp)
    assert got.off_tree_spans == 400
    only_tree = from_trees([tree])
    assert int(got.trace_shape[1]) == int(shapes_ref(only_tree)[0])
    # the same in a chunk: a 30-span cycle with a tail
    small = from_trees([cyc[:29] + [(30, 1, 0)] + [(1000, 17, 0), (1001, 1000, 1)] + tree[:50]])
    assert _check(ctx, small).off_tree_spans == 32


def test_duplicated_ids(ctx):
    """Ids overwritten inside short and long traces: the first match rules."""
    rng = np.random.default_rng(41)
    lens = np.r_[rng.integers(2, 120, 80), [400, 256, 2500]]
    sp = random_tree(rng, lens, self_ref=0.01)
    sid = sp.span_id.copy()
    dup = rng.random(sp.n_spans) < 0.15
    ptr = sp.trace_ptr.astype(np.int64)
    t_of = sp.trace_of_span()
    src = ptr[t_of] + (rng.random(sp.n_spans) * (ptr[t_of + 1] - ptr[t_of])).astype(np.int64)
    sid[dup] = sp.span_id[src[dup]]
    sp = anomod.SpanSet(sp.services, sp.trace_ptr, sid, sid, sp.parent_span_id, sp.svc, sp.flags,
                        sp.dur_us)
    assert not sp.check_unique_ids()
    got = _check(ctx, sp)
    assert got.off_tree_spans > 0          # some overwrites close reference cycles


def test_duplicated_ids_at_window_and_block_borders(ctx, monkeypatch, capfd):
    """test_gpu_self_time.window_border_case: children of an id carried twice
    belong to the first carrier, across the lookup's window and block borders;
    every span of the case is on its tree."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, want = window_border_case()
    got = _check(ctx, sp, use_errors=True)
    assert "trace_shapes_kernel<forward>, 3 long traces" in capfd.readouterr().err
    assert got.off_tree_spans == 0
    # span 2049 continues the path of span 2047, the first carrier of its
    # parent id, not that of span 2048, the later one
    K = label_keys(sp, use_errors=True)[2049]
    assert want[2049] == 2047
    assert int(got.path_hash[2049]) == (int(got.path_hash[2047]) * B + K) & M64
    assert int(got.path_hash[2049]) != (int(got.path_hash[2048]) * B + K) & M64


def test_empty_traces_and_no_spans(ctx):
    sp = from_trees([[], [(1, 0, 0), (2, 1, 1)], [], [], [(3, 0, 0), (4, 3, 1)], []], S=2)
    got = _check(ctx, sp, trace_class=np.array([1, 0, 0, 1, 1, 0]))
    assert got.shape.tolist()[0] == 0 and got.count.tolist() == [4, 2]
    assert got.abnormal.tolist() == [2, 1] and got.first_trace.tolist() == [0, 1]
    only_empty = spanset(2, [0, 0, 0], [], [])
    got = _check(ctx, only_empty, trace_class=np.array([0, 3, 0]))
    assert (got.n_shapes, got.shape.tolist(), got.count.tolist(), got.abnormal.tolist(),
            got.first_trace.tolist()) == (1, [0], [3], [1], [0])
    none = spanset(2, [], [], [])
    got = _check(ctx, none)
    assert got.n_shapes == 0 and got.shape.shape == (0,) and got.trace_shape.shape == (0,)
    assert got.path_hash.shape == (0,) and got.off_tree_spans == 0


def test_one_shape_and_all_distinct(ctx):
    """5,000 traces of one shape; 300 traces (root + k children) all
    distinct."""
    one = from_trees([[(3 * t + 1, 0, 0), (3 * t + 2, 3 * t + 1, 1), (3 * t + 3, 3 * t + 1, 1)]
                      for t in range(5000)])
    got = _check(ctx, one, trace_class=(np.arange(5000) % 7 == 3))
    assert got.n_shapes == 1 and got.count.tolist() == [5000]
    assert got.abnormal.tolist() == [714] and got.first_trace.tolist() == [0]
    stars = [[(1000 * t + 1, 0, 0)] + [(1000 * t + 2 + k, 1000 * t + 1, 1) for k in range(t)]
             for t in range(300)]
    got = _check(ctx, from_trees(stars))
    assert got.n_shapes == 300 and (got.count == 1).all()
    assert (got.shape[1:] > got.shape[:-1]).all()              # ties: by value ascending


def test_many_distinct_shapes(ctx):
    """3 * 2^18 two-span traces root(a) -> child(b) over 1,024 services, every
    (a, b) pair at most once: more distinct shapes than a workgroup of the
    class pass keeps in LDS.  The model of this set is two multiplications per
    trace, taken in numpy u64."""
    S, nt = 1024, 3 << 18
    rng = np.random.default_rng(5)
    pair = rng.permutation(S * S)[:nt]
    a, b = pair // S, pair % S
    sid = np.arange(1, 2 * nt + 1, dtype=np.uint64)
    pid = np.zeros(2 * nt, np.uint64)
    pid[1::2] = sid[0::2]
    svc = np.empty(2 * nt, np.int64)
    svc[0::2], svc[1::2] = a, b
    sp = spanset(S, np.full(nt, 2), sid, pid, svc, unique=True)
    cls = (rng.random(nt) < 0.3).astype(np.uint8)
    K = np.asarray(service_keys(sp, None), np.uint64)

    def vmix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over="ignore"):
        p0 = np.uint64(SEED_ROOT) * np.uint64(B) + K[a]
        p1 = p0 * np.uint64(B) + K[b]
        shape = vmix(p0) + vmix(p1)
    assert int(shape[0]) == int(shapes_ref(from_trees([[(1, 0, int(a[0])), (2, 1, int(b[0]))]],
                                                      S=S), svc_key=None)[0])
    assert np.unique(shape).shape[0] == nt
    got = ctx.trace_shapes(sp, trace_class=cls, per_trace=True, svc_key=None)
    np.testing.assert_array_equal(got.trace_shape, shape)
    order = np.argsort(shape, kind="stable")
    assert got.n_shapes == nt and (got.count == 1).all()
    np.testing.assert_array_equal(got.shape, shape[order])
    np.testing.assert_array_equal(got.first_trace, order.astype(np.uint64))
    np.testing.assert_array_equal(got.abnormal, cls[order].astype(np.uint64))


# ------------------------------------------------------------------ arguments
def test_cap_and_size_query(ctx, synth_case):
    _, sp, (_, _, shape) = synth_case
    lib = anomod.lib()
    S = sp.n_services
    d = ctx.upload(sp)
    try:
        n_all = census_ref(shape).shape.shape[0]
        cs = L.TraceShapesC(S, 0, None, None, 0, 77, 77, None, None, None, None, None, None)
        assert lib.anomod_trace_shapes_spans(ctx.handle, d.handle, C.byref(cs)) == L.OK
        assert cs.n_shapes == n_all and cs.off_tree_spans == 0
        for cap in (1, 2, n_all - 1, n_all, n_all + 5):
            got = ctx.trace_shapes(d, cap=cap)
            _assert_census(got, shape, cap=cap)
            assert got.trace_shape is None and got.path_hash is None
        # a cap with a NULL array
        cs = L.TraceShapesC(S, 0, None, None, 4, 0, 0, None, None, None, None, None, None)
        assert lib.anomod_trace_shapes_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
    finally:
        d.free()


def test_error_codes(ctx):
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1), 200)
    lib = anomod.lib()
    S = sp.n_services
    d = ctx.upload(sp)
    loose = ctx.upload_ungrouped(sp.take(np.arange(sp.n_spans),
                                         np.array([0, sp.n_spans], np.uint64)))
    try:
        q = lambda s: L.TraceShapesC(s, 0, None, None, 0, 0, 0, None, None, None, None, None,  # noqa: E731
                                     None)
        cs = q(S)
        assert lib.anomod_trace_shapes_spans(ctx.handle, loose.handle, C.byref(cs)) == L.ESTATE
        assert b"not grouped" in lib.anomod_last_error(ctx.handle)
        cs = q(S - 1)
        assert lib.anomod_trace_shapes_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
        assert b"service index" in lib.anomod_last_error(ctx.handle)
        cs = q(0)
        assert lib.anomod_trace_shapes_spans(ctx.handle, d.handle, C.byref(cs)) == L.EINVAL
        assert lib.anomod_trace_shapes_spans(ctx.handle, d.handle, None) == L.EINVAL
        with pytest.raises(ValueError):
            ctx.trace_shapes(d, trace_class=np.zeros(3, np.uint8))
        with pytest.raises(ValueError):
            ctx.trace_shapes(d, svc_key="index")
        # spans outside every trace: path_hash 0, not counted
        cut = sp.trace_ptr[3:-3]
        part = anomod.SpanSet(sp.services, cut, sp.trace_hash, sp.span_id, sp.parent_span_id,
                              sp.svc, sp.flags, sp.dur_us)
        got = _check(ctx, part)
        assert not got.path_hash[:int(cut[0])].any() and not got.path_hash[int(cut[-1]):].any()
        assert got.path_hash[int(cut[0]):int(cut[-1])].all()
    finally:
        loose.free()
        d.free()


def test_hints_and_later_results_unchanged(ctx):
    """The call leaves the set's hints alone, and edge_aggregate, self_time
    and trace_spectrum after it equal what they gave before it."""
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=1, p_orphan_ppm=2000), 1500)
    d = ctx.upload(sp)
    fields = ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us")
    try:
        before = (ctx.edge_aggregate(d), ctx.self_time(d), ctx.trace_spectrum(d))
        hints = d.hints
        first = ctx.trace_shapes(d, per_trace=True)
        assert d.hints == hints
        after = (ctx.edge_aggregate(d), ctx.self_time(d), ctx.trace_spectrum(d))
        again = ctx.trace_shapes(d, per_trace=True)
        assert d.hints == hints
        for k in fields:
            np.testing.assert_array_equal(getattr(after[0], k), getattr(before[0], k), err_msg=k)
            np.testing.assert_array_equal(getattr(after[1], k), getattr(before[1], k), err_msg=k)
        for k in ("n_traces", "svc_traces", "edge_traces", "bad_spans", "trace_abnormal"):
            np.testing.assert_array_equal(getattr(after[2], k), getattr(before[2], k), err_msg=k)
        for k in ("shape", "count", "abnormal", "first_trace", "trace_shape"):
            np.testing.assert_array_equal(getattr(again, k), getattr(first, k), err_msg=k)
    finally:
        d.free()


# ------------------------------------------------------------------ through features()
def test_novelty_through_features(ctx):
    """A run equal to its baseline has novelty 0 everywhere; with the sub-tree
    of one service removed from a tenth of its traces, novelty > 0 exactly for
    the services of the altered traces, equal to the host formula."""
    base = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=4), 2000)
    cur, altered = without_subtrees(base, "home-timeline-service")
    assert 30 <= altered.sum() <= 200
    fb = anomod.features(Experiment("base", base), ctx, shapes=True, spectrum=True)
    assert fb.shapes is not None and "shape_novelty" not in fb.params["components"]
    _assert_census(fb.shapes, shapes_ref(base), fb.spectrum.trace_abnormal)
    same = anomod.features(Experiment("same", base), ctx, shapes=True, baseline=fb)
    assert not same.params["components"]["shape_novelty"].any()
    fc = anomod.features(Experiment("cur", cur), ctx, shapes=True, baseline=fb)
    sb, sc = shapes_ref(base), shapes_ref(cur)
    _assert_census(fc.shapes, sc)
    nov = fc.params["components"]["shape_novelty"]
    np.testing.assert_array_equal(nov, novelty_ref(cur, sc, sb))
    in_altered = np.zeros(cur.n_services, bool)
    in_altered[cur.svc[np.repeat(altered, np.diff(cur.trace_ptr).astype(np.int64))]] = True
    np.testing.assert_array_equal(nov > 0, in_altered)
    assert 0 < in_altered.sum() < cur.n_services
    plain = anomod.features(Experiment("cur", cur), ctx, baseline=fb)
    np.testing.assert_array_equal(fc.service_scores, plain.service_scores + 0.25 * nov)


def test_cli_writes_the_shapes_object(golden, tmp_path):
    """python -m anomod features --shapes --baseline on the golden Jaeger dump,
    the run as its own baseline: the census of the model, nothing new."""
    import json

    from anomod.__main__ import main
    src, out = str(golden / "jaeger_small.json"), tmp_path / "features.json"
    assert main(["features", src, "--shapes", "--baseline", src, "--out", str(out)]) == 0
    doc = json.loads(out.read_text())
    sp = anomod.load_experiment(src).spans
    P, on, shape = _ref(sp)
    c = census_ref(shape)
    got = doc["shapes"]
    assert got["distinct"] == c.shape.shape[0] and got["off_tree_spans"] == int((~on).sum())
    assert len(got["top"]) == min(20, c.shape.shape[0]) >= 1
    ptr = sp.trace_ptr.astype(np.int64)
    for k, row in enumerate(got["top"]):
        t = int(c.first_trace[k])
        assert row["shape"] == f"{int(c.shape[k]):016x}" and row["count"] == int(c.count[k])
        assert row["abnormal"] == 0 and row["exemplar_trace"] == t and row["new"] is False
        assert row["exemplar_spans"] == ptr[t + 1] - ptr[t]
        assert row["services"] == [sp.services[s] for s in np.unique(sp.svc[ptr[t]:ptr[t + 1]])]


def test_default_unchanged(ctx):
    exp = anomod.load_experiment(anomod.SynthSpec("SN", seed=4,
                                                  fault_service="home-timeline-service"),
                                 n_traces=400)
    a = anomod.features(exp, ctx)
    c = anomod.features(exp, ctx, shapes=True)
    b = anomod.features(exp, ctx)
    assert a.shapes is None and b.shapes is None and c.shapes is not None
    assert set(a.params["components"]) == {"error_rate", "latency", "metric"}
    assert c.params["components"].keys() == a.params["components"].keys()
    for f in (b, c):
        np.testing.assert_array_equal(f.service_scores, a.service_scores)
        for k in ("count", "errors", "sum_us", "min_us", "max_us", "hist", "p50_us", "p99_us"):
            np.testing.assert_array_equal(getattr(f.edges, k), getattr(a.edges, k), err_msg=k)

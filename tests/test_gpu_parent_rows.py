"""Parent rows of a resident span set: the first grouped aggregation resolves
every span's first-match parent once and keeps its service row with the set
(2 B/span); later aggregations and the exact quantiles stream svc_flags,
dur_us and that column (edge_row_kernel) instead of walking the traces again.

Every table — first call, later calls, under launch caps, with another S at
the C ABI — equals the CPU oracle bit for bit, and the column equals a numpy
model of the first-match parent rule."""
import ctypes as C

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import EdgeTable
from oracle import native, spec

pytestmark = pytest.mark.gpu

FIELDS = ("count", "errors", "sum_us", "min_us", "max_us")
WALK, STREAM = "edge_agg_kernel<", "edge_row_kernel<"
FILLS = "+ parent rows"  # the walk's log line when it also fills the set's column


def assert_table_equal(gpu: anomod.EdgeTable, ref: dict):
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(gpu, k), ref[k], err_msg=k)
    if gpu.hist is not None:
        np.testing.assert_array_equal(gpu.hist, ref["hist"], err_msg="hist")
    ref = native.finalize(ref)
    np.testing.assert_array_equal(gpu.p50_us, ref["p50_us"])  # NaN == NaN here
    np.testing.assert_array_equal(gpu.p99_us, ref["p99_us"])


def _random_spanset(rng, S, n_traces, max_len, orphan=0.05, dup=0.0, lens=None, self_ref=0.0):
    """tests/test_gpu_edge.py's generator (random ancestors, orphans,
    duplicated ids), plus spans that reference their own id."""
    if lens is None:
        lens = rng.integers(0, max_len + 1, n_traces)
    lens = np.asarray(lens, np.int64)
    n_traces = lens.shape[0]
    ptr = np.zeros(n_traces + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    n = int(ptr[-1])
    sid = rng.integers(1, 2**63, n, dtype=np.uint64)
    pid = np.zeros(n, np.uint64)
    t_of = np.repeat(np.arange(n_traces), lens)
    starts = ptr[:-1].astype(np.int64)[t_of]
    pos = np.arange(n) - starts
    has_parent = pos > 0
    pick = starts + (rng.random(n) * np.maximum(pos, 1)).astype(np.int64)
    pid[has_parent] = sid[pick[has_parent]]
    orph = has_parent & (rng.random(n) < orphan)
    pid[orph] = rng.integers(1, 2**63, int(orph.sum()), dtype=np.uint64)
    if dup:
        d = has_parent & (rng.random(n) < dup)
        sid[d] = sid[pick[d]]  # duplicate span ids inside a trace
    if self_ref:
        s = rng.random(n) < self_ref
        pid[s] = sid[s]
    svc = rng.integers(0, S, n).astype(np.uint16)
    flg = (rng.random(n) < 0.1).astype(np.uint16)
    dur = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dur[rng.random(n) < 0.7] %= 20000
    return anomod.SpanSet([f"svc{i:03d}" for i in range(S)], ptr, sid.copy(), sid, pid, svc, flg,
                          dur)


def model_rows(sp: anomod.SpanSet, S: int) -> np.ndarray:
    """The first-match parent rule per trace: S for a span without a parent
    reference (root), S + 1 when the reference is no id of the trace (orphan),
    else the service of the FIRST span of the trace that carries the id — the
    span itself when it references its own id and no earlier span has it.
    Positions outside every trace: 0xFFFF."""
    out = np.full(sp.n_spans, 0xFFFF, np.uint16)
    ptr = sp.trace_ptr.astype(np.int64)
    sid, pid, svc = sp.span_id.tolist(), sp.parent_span_id.tolist(), sp.svc.tolist()
    for t in range(sp.n_traces):
        first = {}
        for i in range(ptr[t], ptr[t + 1]):
            first.setdefault(sid[i], i)
        for i in range(ptr[t], ptr[t + 1]):
            out[i] = S if pid[i] == 0 else svc[first[pid[i]]] if pid[i] in first else S + 1
    return out


def get_rows(ctx, dev, S=None):
    """(status, column) of anomod_spans_parent_rows."""
    out = np.zeros(dev.n_spans, np.uint16)
    rc = L.lib().anomod_spans_parent_rows(ctx.handle, dev.handle, L.ptr(out, C.c_uint16),
                                          len(dev.services) if S is None else S)
    return rc, out


def check_set(ctx, sp, calls=3):
    """Upload once, aggregate `calls` times, every table == the oracle's, the
    column == the model.  Returns the device set (caller frees)."""
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    assert get_rows(ctx, dev)[0] == L.ESTATE  # none before the first aggregation
    for _ in range(calls):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    rc, rows = get_rows(ctx, dev)
    assert rc == 0
    np.testing.assert_array_equal(rows, model_rows(sp, len(sp.services)))
    return dev


def test_model_covers_the_rule():
    """The numpy model on a hand-made trace: root, orphan, first occurrence of
    a repeated id, a span referencing its own id."""
    sid = np.array([5, 7, 7, 9, 11, 12], np.uint64)
    pid = np.array([0, 5, 7, 99, 11, 7], np.uint64)
    svc = np.array([0, 1, 2, 0, 2, 1], np.uint16)
    sp = anomod.SpanSet(["a", "b", "c"], np.array([0, 6], np.uint64), sid.copy(), sid, pid, svc,
                        np.zeros(6, np.uint16), np.ones(6, np.uint32))
    np.testing.assert_array_equal(model_rows(sp, 3), [3, 0, 1, 4, 2, 1])


def _table_from_edges(edges, sp, E):
    """count / errors / sum / min / max / p50 / p99 per edge from per-span
    edge indices, in numpy (no E x 896 histogram)."""
    d = sp.dur_us.astype(np.uint64)
    edges = np.asarray(edges, np.int64)
    tab = {"count": np.bincount(edges, minlength=E).astype(np.uint64),
           "errors": np.bincount(edges, weights=(sp.flags & 1), minlength=E).astype(np.uint64),
           "sum_us": np.zeros(E, np.uint64), "min_us": np.full(E, 0xFFFFFFFF, np.uint32),
           "max_us": np.zeros(E, np.uint32), "p50_us": np.full(E, np.nan),
           "p99_us": np.full(E, np.nan)}
    np.add.at(tab["sum_us"], edges, d)
    np.minimum.at(tab["min_us"], edges, sp.dur_us)
    np.maximum.at(tab["max_us"], edges, sp.dur_us)
    bins = spec.hist_bins_np(sp.dur_us)
    order = np.lexsort((bins, edges))
    es, bs = edges[order], bins[order]
    start = np.r_[0, np.cumsum(tab["count"])[:-1]].astype(np.int64)
    for e in np.flatnonzero(tab["count"]):
        c = int(tab["count"][e])
        for q, k in ((50, "p50_us"), (99, "p99_us")):
            lo, hi = spec.hist_bounds(int(bs[start[e] + (c * q) // 100]))
            tab[k][e] = 0.5 * (lo + hi)
    assert es.shape == edges.shape
    return tab


def test_hbm_tables(ctx):
    """S = 2188: (edge, bin) keys no longer fit the LDS slots' 31 bits, so
    histogram and stats live in HBM (edge_row_kernel<hbm_hist,hbm_stats>).
    The oracle's E x 896 histogram would take 34 GB of host memory at this
    width, so the reference is built in numpy from the oracle's per-span edges
    — the same construction is first held to native.edge_aggregate at S = 12 —
    and the histogram is checked through count and p50 / p99."""
    rng = np.random.default_rng(2188)
    small = _random_spanset(rng, 12, 1500, 30, dup=0.01)
    ref = native.finalize(native.edge_aggregate(small))
    mine = _table_from_edges(native.span_edges(small, 12), small, 14 * 12)
    for k in FIELDS + ("p50_us", "p99_us"):
        np.testing.assert_array_equal(mine[k], ref[k], err_msg=k)
    S = 2188
    sp = _random_spanset(rng, S, 400, 40, dup=0.01, self_ref=0.01)
    E = (S + 2) * S
    want = _table_from_edges(native.span_edges(sp, S), sp, E)
    dev = ctx.upload(sp)
    for _ in range(3):
        got = ctx.edge_aggregate(dev, with_hist=False)
        for k in FIELDS + ("p50_us", "p99_us"):
            np.testing.assert_array_equal(getattr(got, k), want[k], err_msg=k)
    rc, rows = get_rows(ctx, dev)
    assert rc == 0
    np.testing.assert_array_equal(rows, model_rows(sp, S))
    dev.free()


@pytest.mark.parametrize("case", ["sn_width", "shuffled_unique", "wide", "slot"])
def test_forms_and_scans(ctx, case):
    """S = 12 with orphans, duplicated ids (forward scan) and empty traces;
    the same shape declared unique and shuffled inside its traces (order
    probe, then the forward scan); S = 46 (wide stats); E > 2304 (slot
    stats)."""
    rng = np.random.default_rng(len(case) * 101)
    if case == "sn_width":
        sp = _random_spanset(rng, 12, 3000, 40, orphan=0.03, dup=0.01, self_ref=0.01)
        assert (np.diff(sp.trace_ptr.astype(np.int64)) == 0).any()
    elif case == "shuffled_unique":
        sp = _random_spanset(rng, 12, 3000, 40, orphan=0.03)
        assert sp.check_unique_ids()
        tmp = ctx.upload(sp)
        shuf = ctx.shuffle(tmp, seed=5, window_traces=0)
        sp = shuf.download()
        tmp.free()
        shuf.free()
        assert sp.unique_ids
        sp.scan_order = -1
    elif case == "wide":
        sp = _random_spanset(rng, 46, 2000, 40, dup=0.01)
    else:
        sp = _random_spanset(rng, 60, 1500, 40, dup=0.01)
    dev = check_set(ctx, sp)
    if case == "shuffled_unique":
        assert dev.scan_order == 0
    dev.free()


def test_chunk_borders_and_long_traces(ctx):
    """Traces of exactly 255, 256, 257, 300 and 5000 spans among short ones
    (the chunk border; the long-trace pass writes into the same column), and
    a run of more than 64 one-span traces (the chunk's trace limit)."""
    rng = np.random.default_rng(17)
    lens = np.r_[rng.integers(0, 30, 300), [255, 256, 257, 300, 5000], np.ones(150, np.int64),
                 rng.integers(0, 30, 300), [256, 257]]
    sp = _random_spanset(rng, 12, 0, 0, lens=lens, dup=0.01, self_ref=0.01)
    check_set(ctx, sp).free()
    rng.shuffle(lens)
    check_set(ctx, _random_spanset(rng, 12, 0, 0, lens=lens, dup=0.01)).free()


def _offset_set(core: anomod.SpanSet, head: int, tail: int, rng):
    """core with `head` spans before its first trace and `tail` after its last
    that belong to no trace."""
    junk = _random_spanset(rng, len(core.services), 0, 0, lens=[head + tail])
    cat = lambda a, b: np.concatenate([b[:head], a, b[head:]])  # noqa: E731
    sid = cat(core.span_id, junk.span_id)
    return anomod.SpanSet(core.services, core.trace_ptr + np.uint64(head), sid.copy(), sid,
                          cat(core.parent_span_id, junk.parent_span_id), cat(core.svc, junk.svc),
                          cat(core.flags, junk.flags), cat(core.dur_us, junk.dur_us))


@pytest.mark.parametrize("n_range", [8191, 8192, 8193])
@pytest.mark.parametrize("head", [0, 1, 2, 3])
def test_stream_borders(ctx, n_range, head):
    """Stream ranges of 8191 / 8192 / 8193 spans (one load round of a
    1024-thread workgroup is 8192 spans) starting at span position 0..3, with
    spans outside every trace before and after: the 16-B and 8-B loads start
    at the first 4-aligned position, the spans around them are read singly."""
    rng = np.random.default_rng(n_range * 4 + head)
    lens = []
    while sum(lens) < n_range:
        lens.append(int(min(rng.integers(0, 40), n_range - sum(lens))))
    core = _random_spanset(rng, 12, 0, 0, lens=lens, dup=0.01)
    assert core.n_spans == n_range
    sp = _offset_set(core, head, 5, rng) if head else core
    ref = native.edge_aggregate(core)
    dev = ctx.upload(sp)
    for _ in range(3):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    rc, rows = get_rows(ctx, dev)
    assert rc == 0
    want = model_rows(sp, 12)
    assert (want[:head] == 0xFFFF).all() and (head == 0 or (want[-5:] == 0xFFFF).all())
    np.testing.assert_array_equal(rows, want)
    dev.free()


@pytest.mark.parametrize("cap", [1000, 4096])
def test_launch_caps(ctx, monkeypatch, cap):
    """ANOMOD_MAX_LAUNCH_SPANS on a set with a 5000-span trace: the first call
    fills the column launch by launch, later calls cut the stream by span
    count; once more without the cap."""
    rng = np.random.default_rng(cap)
    sp = anomod.SpanSet.concat([_random_spanset(rng, 12, 1500, 12, dup=0.01),
                                _random_spanset(rng, 12, 0, 0, lens=[5000, 300]),
                                _random_spanset(rng, 12, 500, 3)])
    assert int(np.diff(sp.trace_ptr.astype(np.int64)).max()) == 5000  # alone over either cap
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    monkeypatch.setenv("ANOMOD_MAX_LAUNCH_SPANS", str(cap))
    for _ in range(3):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    monkeypatch.delenv("ANOMOD_MAX_LAUNCH_SPANS")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    np.testing.assert_array_equal(get_rows(ctx, dev)[1], model_rows(sp, 12))
    dev.free()


def _aggregate_abi(ctx, dev, S):
    table = EdgeTable.empty([f"svc{i:03d}" for i in range(S)], True)
    cs = table.c_struct()
    L.check(L.lib().anomod_edge_aggregate_spans(ctx.handle, dev.handle, S, C.byref(cs)),
            ctx.handle)
    table.hist = table.hist.reshape(-1, L.HIST_BINS)
    return table


@pytest.mark.parametrize("first", [12, 15])
def test_another_service_count(ctx, first):
    """The same resident set aggregated at the C ABI with S and S + 3, either
    one first: root / orphan rows do not depend on the S that filled them."""
    rng = np.random.default_rng(first)
    sp = _random_spanset(rng, 12, 2000, 30, dup=0.01)
    refs = {}
    for S in (12, 15):
        wide = anomod.SpanSet([f"svc{i:03d}" for i in range(S)], sp.trace_ptr, sp.trace_hash,
                              sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us)
        refs[S] = native.edge_aggregate(wide)
    dev = ctx.upload(sp)
    for S in (first, 27 - first, first, 27 - first):
        assert_table_equal(_aggregate_abi(ctx, dev, S), refs[S])
    for S in (12, 15):
        np.testing.assert_array_equal(get_rows(ctx, dev, S)[1], model_rows(sp, S))
    dev.free()


def _kernels(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if "edge aggregation kernel" in ln]


def test_switch_and_overrides(ctx, monkeypatch, capfd):
    """ANOMOD_PARENT_ROWS=0: equal tables, no column, the walk kernel on every
    call.  Without it the later calls name edge_row_kernel, and
    ANOMOD_UNIQUE_SCAN=0 on a set that holds rows bypasses them."""
    rng = np.random.default_rng(33)
    sp = _random_spanset(rng, 12, 3000, 30, dup=0.01)
    ref = native.edge_aggregate(sp)
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_PARENT_ROWS", "0")
    dev = ctx.upload(sp)
    capfd.readouterr()
    for _ in range(3):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    names = _kernels(capfd)
    assert len(names) == 3 and all(WALK in n and FILLS not in n for n in names), names
    assert get_rows(ctx, dev)[0] == L.ESTATE
    monkeypatch.delenv("ANOMOD_PARENT_ROWS")
    for _ in range(3):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    names = _kernels(capfd)
    assert WALK in names[0] and FILLS in names[0], names
    assert all(STREAM in n for n in names[1:]) and len(names) == 3, names
    monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "0")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    names = _kernels(capfd)
    assert len(names) == 1 and WALK in names[0] and FILLS not in names[0], names
    monkeypatch.delenv("ANOMOD_UNIQUE_SCAN")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert STREAM in _kernels(capfd)[0]
    dev.free()


def test_exact_quantiles_from_rows(ctx, monkeypatch, capfd):
    """edge_quantiles_exact on a set with rows == the numpy sort model == the
    result under ANOMOD_PARENT_ROWS=0 (the key walk); the log says which of
    the two wrote the keys."""
    key_stream = "edge key kernel edge_row_kernel<keys>"
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(44)
    sp = anomod.SpanSet.concat([_random_spanset(rng, 12, 3000, 24, dup=0.02),
                                _random_spanset(rng, 12, 0, 0, lens=[700, 2500])])
    q = (0, 50, 57, 95, 99)
    want = native.exact_quantiles(sp, q)
    dev = ctx.upload(sp)
    ctx.edge_aggregate(dev)
    assert get_rows(ctx, dev)[0] == 0
    capfd.readouterr()
    got, cnt = ctx.edge_quantiles_exact(dev, q)
    assert key_stream in capfd.readouterr().err
    np.testing.assert_array_equal(got, want)
    assert int(cnt.sum()) == sp.n_spans
    monkeypatch.setenv("ANOMOD_PARENT_ROWS", "0")
    got0, cnt0 = ctx.edge_quantiles_exact(dev, q)
    assert key_stream not in capfd.readouterr().err
    np.testing.assert_array_equal(got0, got)
    np.testing.assert_array_equal(cnt0, cnt)
    dev.free()


def test_hints_learned_and_kept(ctx):
    """A generated SN set learns the pair form, a LONG set of 2^16 traces the
    compact form, from the first call; set_hints, unique_ids and set_start_us
    afterwards leave the later (streamed) tables equal."""
    dev = ctx.generate(anomod.SynthSpec("SN", seed=3, p_orphan_ppm=500), 20000)
    assert dev.hints[1] == -1
    ref = native.edge_aggregate(dev.download())
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert dev.hints[1] == 0
    dev.set_hints(-1, -1)
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    dev.unique_ids = False
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    dev.unique_ids = True
    dev.set_hints(0, 1)
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    dev.set_start_us(np.arange(dev.n_spans, dtype=np.uint64) + np.uint64(10**15))
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert get_rows(ctx, dev)[0] == 0
    dev.free()
    dev = ctx.generate(anomod.SynthSpec("LONG", seed=9), 1 << 16)
    ref = native.edge_aggregate(dev.download())
    for _ in range(2):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
        assert dev.hints[1] == 1
    dev.free()


def test_host_set_builds_no_column(ctx, monkeypatch, capfd):
    """A host SpanSet passed straight to edge_aggregate (uploaded per call):
    equal tables and the walk kernel both times."""
    rng = np.random.default_rng(55)
    sp = _random_spanset(rng, 12, 3000, 30, dup=0.01)
    ref = native.edge_aggregate(sp)
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    capfd.readouterr()
    for _ in range(2):
        assert_table_equal(ctx.edge_aggregate(sp), ref)
    names = _kernels(capfd)
    assert len(names) == 2 and all(WALK in n and FILLS not in n for n in names), names


def _device_free_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    assert L.lib().hipMemGetInfo(C.byref(free), C.byref(total)) == 0  # (libanomod's HIP runtime)
    return free.value


@pytest.mark.parametrize("fused", ["0", None])
def test_ungrouped_set_builds_no_column(ctx, monkeypatch, capfd, fused):
    """An ungrouped set (spans of every 64 traces interleaved).  With
    ANOMOD_UNGROUPED_FUSED=0 each call groups it into the context's workspace
    and aggregates a view of that workspace, which is gone after the call:
    the walk kernel every time, never filling a column, and device memory
    does not shrink from call to call (a column allocated for the view would
    leak 2 B/span per call: 4 x 4.4 MB here against a 2.2 MB allowance).
    The default (fused) path records from the join and walks nothing."""
    if fused is not None:
        monkeypatch.setenv("ANOMOD_UNGROUPED_FUSED", fused)
    dev = ctx.generate(anomod.SynthSpec("SN", seed=12, p_orphan_ppm=500), 1 << 18)
    ref = native.edge_aggregate(dev.download())
    ung = ctx.shuffle(dev, seed=6, window_traces=64)
    assert not ung.grouped
    assert_table_equal(ctx.edge_aggregate(ung), ref)  # workspaces grow here
    ctx.synchronize()
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    capfd.readouterr()
    free0 = _device_free_bytes()
    for _ in range(4):
        assert_table_equal(ctx.edge_aggregate(ung), ref)
    ctx.synchronize()
    shrunk = free0 - _device_free_bytes()
    names = _kernels(capfd)
    if fused == "0":
        assert len(names) == 4 and all(WALK in n and FILLS not in n for n in names), names
    else:
        assert names == []
    assert shrunk < ung.n_spans, (shrunk, ung.n_spans)
    assert get_rows(ctx, ung)[0] == L.ESTATE
    ung.free()
    dev.free()

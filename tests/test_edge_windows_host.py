"""Span start times and the windowed edge series, host side (no GPU): the
start_us column of both decoders against the reference's own CSV, the SpanSet
operations that carry it, EdgeWindows.matrix, and the trace anomaly score end
to end on the CPU restatement of the per-window edge table."""
import json
from datetime import datetime, timezone

import numpy as np
import pytest

import anomod
from anomod import decode
from anomod.spans import EdgeWindows
from oracle import native

from edge_windows_ref import edge_windows_ref, formula_starts

FAULT = "home-timeline-service"
T0 = 1_762_000_005_000_000  # a multiple of 15 s
STEP = 15_000_000
T = 120


def fault_set(n_traces=3000):
    """A normal half then a faulted half, spread in order over T windows."""
    sp = anomod.SpanSet.concat([
        anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1), n_traces),
        anomod.synth_generate_host(anomod.SynthSpec("SN", seed=1, fault_service=FAULT), n_traces,
                                   shard=1)])
    sp.start_us = formula_starts(sp, T0, T * STEP, 50)
    return sp


# ------------------------------------------------------------------ decoders
def test_jaeger_start_us_equals_reference_csv(golden):
    """Both decoders' start_us == the start_time column jaeger_to_csv.py wrote
    (datetime.fromtimestamp(startTime / 1e6) under TZ=UTC, microseconds kept)."""
    import csv

    with open(golden / "jaeger_small.csv", newline="") as fh:
        rows = list(csv.DictReader(fh))
    epoch = datetime(1970, 1, 1, tzinfo=timezone.utc)
    want = []
    for r in rows:
        t = datetime.strptime(r["start_time"], "%Y-%m-%d %H:%M:%S.%f").replace(tzinfo=timezone.utc)
        d = t - epoch
        want.append((d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds)
    want = np.asarray(want, np.uint64)
    data = (golden / "jaeger_small.json").read_bytes()
    py = decode.decode_jaeger(json.loads(data))
    nat = anomod.decode_native(data, "jaeger")
    assert py.start_us.dtype == nat.start_us.dtype == np.uint64
    assert len(want) == py.n_spans and want.min() > 0
    np.testing.assert_array_equal(py.start_us, want)
    np.testing.assert_array_equal(nat.start_us, want)
    np.testing.assert_array_equal(anomod.load_trace_file(golden / "jaeger_small.json").start_us, want)


def _payload_from_raw(traces):
    """Collector payload of raw GraphQL span lists (the fields the decoders read)."""
    out = []
    for spans in traces:
        nodes, parents, kept = decode.skywalking_parents(list(spans))
        if not kept:
            continue
        out.append({"summary": {"trace_id": str(kept[0].get("traceId") or "")},
                    "spans": [{"node_id": n, "parent_node_id": p,
                               "service_code": s.get("serviceCode") or "",
                               "start_timestamp_ms": s.get("startTime"),
                               "end_timestamp_ms": s.get("endTime"),
                               "is_error": bool(s.get("isError", False))}
                              for n, p, s in zip(nodes, parents, kept)]})
    return {"metadata": {}, "traces": out}


@pytest.mark.parametrize("name", ["skywalking_small.json", "skywalking_dups.json"])
def test_skywalking_start_us_native_equals_python(golden, name):
    g = json.loads((golden / name).read_text())
    raw = decode.decode_skywalking_raw(g["inputs"])
    want = np.asarray([s["startTime"] * 1000 for spans in g["inputs"]
                       for s in decode.skywalking_parents(list(spans))[2]], np.uint64)
    np.testing.assert_array_equal(raw.start_us, want)
    assert want.min() > 0
    for payload in filter(None, [g.get("payload"), _payload_from_raw(g["inputs"])]):
        py = decode.decode_skywalking_payload(payload)
        nat = anomod.decode_native(json.dumps(payload).encode(), "skywalking")
        assert py.n_spans == nat.n_spans > 0
        np.testing.assert_array_equal(nat.start_us, py.start_us)
        starts = [s.get("start_timestamp_ms") for t in payload["traces"] for s in t["spans"]]
        np.testing.assert_array_equal(py.start_us, np.asarray(starts, np.uint64) * np.uint64(1000))


BAD_STARTS = [None, -5, 1.5, 1762180839724.0, "1762180839724", True, [1], 2**64, 2**63]


def test_missing_or_non_integer_start_gives_zero():
    """Missing, negative, non-integer (float, string, bool, container) and
    out-of-range starts give 0 in both decoders; integers pass through."""
    good = 1762207158839501
    spans = [{"traceID": "t", "spanID": "%016x" % (k + 1), "processID": "p", "duration": 5,
              "startTime": v} for k, v in enumerate(BAD_STARTS + [good, 0])]
    spans.append({"traceID": "t", "spanID": "ff", "processID": "p", "duration": 5})  # missing
    doc = {"data": [{"traceID": "t", "spans": spans, "processes": {"p": {"serviceName": "a"}}}]}
    # Jaeger takes the value itself: 2^63 fits a u64, 2^64 does not
    want = np.asarray([0] * 7 + [0, 2**63, good, 0, 0], np.uint64)
    np.testing.assert_array_equal(decode.decode_jaeger(doc).start_us, want)
    np.testing.assert_array_equal(
        anomod.decode_native(json.dumps(doc).encode(), "jaeger").start_us, want)

    ms = 1762180839724
    recs = [{"node_id": f"s:{k}", "parent_node_id": None, "service_code": "a",
             "start_timestamp_ms": v, "end_timestamp_ms": ms + 3}
            for k, v in enumerate(BAD_STARTS + [ms, 2**64 // 1000 + 1])]
    recs.append({"node_id": "s:x", "parent_node_id": None, "service_code": "a"})
    payload = {"metadata": {}, "traces": [{"summary": {"trace_id": "t"}, "spans": recs}]}
    want = np.asarray([0] * 9 + [ms * 1000, 0, 0], np.uint64)  # x 1000 must fit a u64
    np.testing.assert_array_equal(decode.decode_skywalking_payload(payload).start_us, want)
    np.testing.assert_array_equal(
        anomod.decode_native(json.dumps(payload).encode(), "skywalking").start_us, want)
    raw = [[{"traceId": "t", "segmentId": "s", "spanId": k, "serviceCode": "a", "startTime": v,
             "endTime": ms} for k, v in enumerate([ms, None, -1, 2.5, "7"])]]
    np.testing.assert_array_equal(decode.decode_skywalking_raw(raw).start_us,
                                  np.asarray([ms * 1000, 0, 0, 0, 0], np.uint64))


# ------------------------------------------------------------------ SpanSet
def test_span_set_operations_carry_start_us():
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=5), 300)
    assert sp.start_us is None
    start = np.arange(sp.n_spans, dtype=np.uint64) * np.uint64(7) + np.uint64(10**15)
    sp.start_us = start
    sid_to_start = dict(zip(zip(sp.trace_hash.tolist(), sp.span_id.tolist()), start.tolist()))

    def check(sub):
        assert sub.start_us is not None and sub.start_us.dtype == np.uint64
        want = [sid_to_start[k] for k in zip(sub.trace_hash.tolist(), sub.span_id.tolist())]
        np.testing.assert_array_equal(sub.start_us, np.asarray(want, np.uint64))

    mask = np.arange(sp.n_traces) % 3 == 1
    check(sp.select_traces(mask))
    parts = [sp.shard(4, r) for r in range(4)]
    for p in parts:
        check(p)
    assert sum(p.n_spans for p in parts) == sp.n_spans
    order = np.random.default_rng(0).permutation(sp.n_spans)
    check(sp.take(order, np.array([0, sp.n_spans], np.uint64)))
    cat = anomod.SpanSet.concat(parts)
    check(cat)
    assert cat.n_spans == sp.n_spans
    few = sp.select_traces(np.arange(sp.n_traces) < 3)
    obs = few.observed_services()
    assert len(obs.services) < len(few.services)
    np.testing.assert_array_equal(obs.start_us, few.start_us)
    # concat: None unless every part has the column
    bare = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=6), 10)
    assert anomod.SpanSet.concat([sp, bare]).start_us is None
    # positional construction still works and the length is validated
    pos = anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id, sp.parent_span_id,
                         sp.svc, sp.flags, sp.dur_us)
    assert pos.start_us is None
    with pytest.raises(ValueError):
        anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id, sp.parent_span_id,
                       sp.svc, sp.flags, sp.dur_us, start_us=start[:-1])


# ------------------------------------------------------------------ matrix
def test_edge_windows_matrix_hand_made():
    svcs = ["a", "b"]
    S, E = 2, 8
    win = EdgeWindows.empty(svcs, 3_000_000, 500_000, 3)
    assert win.count.shape == (3, E) and win.max_us.dtype == np.uint32
    root_b = S * S + 1       # ROOT -> b
    a_b = 0 * S + 1          # a -> b
    orph_a = (S + 1) * S     # ORPHAN -> a
    win.count[:, a_b] = [7, 4, 0]
    win.sum_us[:, a_b] = [700, 400, 0]
    win.count[:, root_b] = [5, 0, 1]
    win.sum_us[:, root_b] = [15, 0, 9]
    win.count[2, orph_a] = 2**33
    win.sum_us[2, orph_a] = 2**35
    mm = win.matrix(min_count=5)
    assert isinstance(mm, anomod.MetricMatrix)
    assert mm.X.dtype == np.float32 and mm.X.shape == (3, 6)
    lab = lambda p, c: (("parent", p), ("child", c))  # noqa: E731
    assert mm.series == [("edge_count", lab("a", "b")), ("edge_mean_us", lab("a", "b")),
                         ("edge_count", lab("ROOT", "b")), ("edge_mean_us", lab("ROOT", "b")),
                         ("edge_count", lab("ORPHAN", "a")), ("edge_mean_us", lab("ORPHAN", "a"))]
    nan = np.nan
    want = np.array([
        [np.log2(8.0), np.log2(101.0), np.log2(6.0), np.log2(4.0), 0.0, nan],
        [np.log2(5.0), nan, 0.0, nan, 0.0, nan],
        [0.0, nan, 1.0, nan, np.log2(1.0 + 2.0**33), np.log2(5.0)]], np.float64)
    np.testing.assert_array_equal(mm.X, want.astype(np.float32))
    np.testing.assert_array_equal(mm.timestamps, np.array([3.0, 3.5, 4.0]))
    # min_count moves the NaN threshold only
    mm1 = win.matrix(min_count=1)
    assert np.isfinite(mm1.X[1, 1]) and np.isnan(mm1.X[2, 1]) and np.isfinite(mm1.X[2, 3])
    np.testing.assert_array_equal(mm1.X[:, 0::2], mm.X[:, 0::2])
    # an all-empty table gives a [T, 0] matrix
    assert EdgeWindows.empty(svcs, 0, 1, 4).matrix().X.shape == (4, 0)


def test_trace_window_scores_pure():
    svcs = ["a", "b", "c"]
    S = 3
    win = EdgeWindows.empty(svcs, 0, 1, 4)
    rows = [0 * S + 1, 1 * S + 2, S * S + 1]   # a->b, b->c, ROOT->b
    for r in rows:
        win.count[0, r] = 1
    Z = np.zeros((41, 6), np.float32)
    Z[0] = 1e6                   # the first score window is dropped
    Z[5, 0], Z[9, 0] = 4.0, 2.0  # a->b count column: top-2 mean = 3
    Z[7, 3] = 8.0                # b->c mean column: top-2 mean = 4
    Z[3, 5], Z[4, 5] = 10.0, 6.0  # ROOT->b mean column: 8 > 3
    got = anomod.trace_window_scores(Z, win, S)
    np.testing.assert_allclose(got, [0.0, 8.0, 4.0])
    assert anomod.trace_window_scores(Z[:1], win, S).tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ end to end
def test_fault_ranked_first_through_the_restatement():
    """Restated per-window table -> matrix -> oracle EWMA/z (eps 1e-2) ->
    trace_window_scores: the faulted service leads by at least 2x."""
    sp = fault_set()
    W = 6
    win = edge_windows_ref(sp, T0, STEP, T)
    assert win.outside == 0 and int(win.count.sum()) == sp.n_spans
    mm = win.matrix(5).pad_to_multiple(W)
    Z = native.ewma_z(mm.X, 2.0 / (W + 1), W, eps=1e-2)
    ts = anomod.trace_window_scores(Z, win, sp.n_services)
    order = np.argsort(-ts)
    print("trace scores:", dict(zip(sp.services, np.round(ts, 2))))
    assert sp.services[order[0]] == FAULT
    assert ts[order[0]] / ts[order[1]] >= 2.0

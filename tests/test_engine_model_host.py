"""features() / rank() against the plain model of tests/engine_ref.py, on the
CPU: every Context call is answered by RefContext from the references the
kernels are held to, so the whole composition — column scores, squashing,
series -> service, error / latency / z terms, the score sum, the
personalization — runs here and is compared with hand-computed literals and
with the model (rtol 1e-12: float64 arithmetic on the same tables)."""
import math

import numpy as np
import pytest

import anomod
from anomod.decode import MetricMatrix
from oracle import native

import engine_ref as R
from engine_ref import ALL_ON, RefContext, STEP_S

FLAG_ERROR = anomod.FLAG_ERROR
SWITCHES = {
    "trace": dict(trace_step_s=STEP_S),
    "self_time": dict(self_time=True),
    "spectrum": dict(spectrum=True),
    "spectrum_all": dict(spectrum=True, spectrum_rows="all"),
    "critical_path": dict(critical_path=True),
    "trace_quantile": dict(trace_step_s=STEP_S, trace_quantile=90),
    "shapes": dict(shapes=True),
    "error_origins": dict(error_origins=True),
    "trace_load": dict(trace_step_s=STEP_S, trace_load=True),
    "exemplars": dict(exemplars=4),
}


@pytest.fixture(scope="module")
def cache():
    return {}


def check(exp, f, base, zs):
    m = R.model(R.inputs_of(exp, f, base, zs))
    R.assert_model_equals(f, m)
    return m


# ------------------------------------------------------- hand-computed runs
HAND_T0 = 1_700_000_010_000_000   # a multiple of 15 s


def hand_experiment(services, dur, n_traces=20, err_db=5, err_api=2, no_web_from=None):
    """n_traces traces of four spans: api (a root) calls db and web, and an
    auth span refers to a parent no span carries (ORPHAN -> auth).  db fails
    in the first err_db traces, api relays the failure in the first err_api;
    the traces from no_web_from on lack the web span.  Trace t starts in
    window t."""
    ix = {s: services.index(s) for s in ("api", "db", "web", "auth")}
    sid, pid, svc, flags, durs, start, ptr = [], [], [], [], [], [], [0]
    for t in range(n_traces):
        b = 10 * t
        t_us = HAND_T0 + t * int(STEP_S * 1e6)
        for k, (name, parent) in enumerate((("api", 0), ("db", b + 1), ("web", b + 1),
                                             ("auth", b + 9))):
            if name == "web" and no_web_from is not None and t >= no_web_from:
                continue
            sid.append(b + 1 + k)
            pid.append(parent)
            svc.append(ix[name])
            err = (name == "db" and t < err_db) or (name == "api" and t < err_api)
            flags.append(FLAG_ERROR if err else 0)
            durs.append(dur[name])
            start.append(t_us + 10 * k)
        ptr.append(len(sid))
    trace_hash = np.repeat(np.arange(n_traces) + 1, np.diff(ptr))
    return anomod.SpanSet(list(services), ptr, trace_hash, sid, pid, svc, flags, durs, None, True,
                          start_us=np.asarray(start, np.uint64))


HAND_SERVICES = ["api", "db", "web", "auth"]
HAND_SERIES = [("cpu", (("pod", "db-0"),)),                     # db
               ("cpu", (("pod", "web-api"),)),                  # api and web tie: api is first
               ("cpu", (("node", "node7"),)),                   # no service
               ("mem", (("pod", "web-1"), ("svc", "api"))),     # the tie across two values: api
               ("mem", (("pod", "auth-db"),))]                  # the longer name: auth
HAND_Z = {
    "metric": np.array([[3.0, 0.5, 100.0, 0.25, 1.0],
                        [1.0, 1.0, 7.0, 0.125, 4.0],
                        [0.0, 0.25, 0.0, 0.0, 2.0],
                        [2.0, 0.0, 50.0, 0.0, 0.0]], np.float32),
    # active rows: api->db (1), api->web (2), ROOT->api (16), ORPHAN->auth (23);
    # columns (count, mean) per row; the first window is dropped
    "trace": np.array([[1e6] * 8,
                       [0.0, 3.0, 1.0, 0.0, 9.0, 0.0, 0.0, 0.25],
                       [0.5, 1.0, 0.5, 0.5, 1.0, 2.0, 1 / 3, 0.125],
                       [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32),
    "load": np.array([[1e6] * 4,
                      [1.0, 0.0, 0.0, 3.0],
                      [0.0, 0.0, 4.0, 0.0],
                      [0.5, 0.0, 1.0, 1.0]], np.float32),
}
THIRD = float(np.float32(1 / 3))


def hand_hook(name, Z):
    assert Z.shape == HAND_Z[name].shape, (name, Z.shape)
    return HAND_Z[name].copy()


def hand_pair(**kw):
    # the baseline lists the services in another order and one more of them
    base_sp = hand_experiment(["auth", "extra", "web", "db", "api"],
                              dict(api=30, db=4, web=20, auth=2))
    cur_sp = hand_experiment(HAND_SERVICES, dict(api=30, db=16, web=2, auth=4), **kw)
    X = np.zeros((240, 5), np.float32)
    cur = anomod.Experiment("hand", cur_sp, MetricMatrix(X, np.arange(240) * 15.0, HAND_SERIES))
    return cur, anomod.Experiment("hand_base", base_sp, None)


def test_hand_computed_components():
    cur, base = hand_pair()
    ctx = RefContext(z_hook=hand_hook)
    fb, _ = R.run(base, ctx, self_time=True)
    kw = dict(trace_step_s=STEP_S, trace_load=True)
    f, zs = R.run(cur, ctx, baseline=fb, **kw)
    assert set(zs) == {"metric", "trace", "load"}
    m = check(cur, f, fb, zs)
    comp = f.params["components"]
    want = {
        # api relays 2 of db's 5 failures over 20 calls each; web and auth never fail
        "error_rate": [0.1, 0.25, 0.0, 0.0],
        # p99 x 1 (ROOT -> api), x 4 (api -> db), / 10 (api -> web: no growth),
        # x 2 (ORPHAN -> auth); durations below 64 us have histogram bins of
        # their own, so the quantiles are the durations
        "latency": [0.0, 2.0, 0.0, 1.0],
        # k = 1 of 4 windows, the first kept: api max(1, 0.25) -> 1/2, db 3 -> 3/4,
        # auth 4 -> 4/5; the node7 series (100) belongs to nobody
        "metric": [0.5, 0.75, 0.0, 0.8],
        # k = 1 of the 3 windows left: db 3 -> 3/4, web 1 -> 1/2, api 9 -> 9/10,
        # auth max(1/3, 1/4) -> (1/3) / (4/3)
        "trace": [0.9, 0.75, 0.5, THIRD / (1 + THIRD)],
        # rows 1, 2, 16, 23 -> db 1 -> 1/2, web 0, api 4 -> 4/5, auth 3 -> 3/4
        "load": [0.8, 0.5, 0.0, 0.75],
    }
    for k, v in want.items():
        np.testing.assert_allclose(comp[k], v, rtol=1e-15, atol=0, err_msg=k)
        np.testing.assert_allclose(m[k], v, rtol=1e-15, atol=0, err_msg=k)
    score = [e + l + 0.25 * (a + b + c) for e, l, a, b, c in
             zip(*(want[k] for k in ("error_rate", "latency", "metric", "trace", "load")))]
    np.testing.assert_allclose(f.service_scores, score, rtol=1e-15)
    np.testing.assert_allclose(f.trace_window_scores, [9.0, 3.0, 1.0, THIRD], rtol=0)
    # the origin rate: only db's failures start anywhere
    fo, zs = R.run(cur, ctx, baseline=fb, error_origins=True, **kw)
    check(cur, fo, fb, zs)
    assert fo.params["components"]["error_rate"].tolist() == [0.0, 0.25, 0.0, 0.0]
    assert fo.params["components"]["error_kind"] == "origin"
    # self time: api's own time doubled (30 - 16 - 2 against 30 - 4 - 20) under
    # the same duration, the leaves keep theirs: the ROOT row counts too
    fs, zs = R.run(cur, ctx, baseline=fb, self_time=True, **kw)
    check(cur, fs, fb, zs)
    assert fs.params["components"]["latency"].tolist() == [1.0, 2.0, 0.0, 1.0]
    assert fs.params["components"]["latency_kind"] == "self"
    # ... and without the baseline's table the inclusive term stays
    fb0, _ = R.run(base, ctx)
    fi, zs = R.run(cur, ctx, baseline=fb0, self_time=True, **kw)
    check(cur, fi, fb0, zs)
    assert fi.params["components"]["latency"].tolist() == want["latency"]
    assert fi.params["components"]["latency_kind"] == "inclusive"


def test_hand_computed_spectrum_and_shape_novelty():
    """Every trace holds every service; 5 of 20 are abnormal (db's failures:
    no duration passes the baseline's p99 of its ROOT row) -> Ochiai 5 /
    sqrt(5 * 20) = 1/2 for all.  Without the web span in the last 4 traces
    there are two shapes, the new one in 4 of 20 traces; web is in no
    exemplar of it, and in 16 traces of which all 5 abnormal ones."""
    ctx = RefContext(z_hook=hand_hook)
    for kw, och, nov in (({}, [0.5, 0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0]),
                         (dict(no_web_from=16), [0.5, 0.5, 5 / math.sqrt(5.0 * 16), 0.5],
                          [0.2, 0.2, 0.0, 0.2])):
        cur, base = hand_pair(**kw)
        fb, _ = R.run(base, ctx, shapes=True)
        f, zs = R.run(cur, ctx, baseline=fb, spectrum=True, shapes=True)
        m = check(cur, f, fb, zs)
        comp = f.params["components"]
        assert comp["spectrum_thresholds"] == "baseline"
        assert f.spectrum.n_traces.tolist() == [15, 5] and f.shapes.n_shapes == (2 if kw else 1)
        for k, v in (("spectrum", och), ("shape_novelty", nov)):
            np.testing.assert_allclose(comp[k], v, rtol=1e-15, atol=0, err_msg=k)
            np.testing.assert_allclose(m[k], v, rtol=1e-15, atol=0, err_msg=k)
        base_score = R.run(cur, ctx, baseline=fb)[0].service_scores
        np.testing.assert_allclose(f.service_scores, base_score + 0.25 * (np.array(och) + nov),
                                   rtol=1e-15)


def test_hand_computed_ranking():
    cur, base = hand_pair()
    ctx = RefContext(z_hook=hand_hook)
    fb, _ = R.run(base, ctx)
    f, zs = R.run(cur, ctx, baseline=fb, trace_step_s=STEP_S)
    score = [0.1 + 0.0 + 0.25 * (0.5 + 0.9), 0.25 + 2.0 + 0.25 * (0.75 + 0.75),
             0.25 * 0.5, 1.0 + 0.25 * (0.8 + THIRD / (1 + THIRD))]
    total = sum(score)
    p = [s + 1e-9 * total for s in score]
    np.testing.assert_allclose(R.personalization(f.service_scores), p, rtol=1e-15)
    # the call graph: api -> db and api -> web, 20 calls each; ROOT and ORPHAN rows dropped
    row_ptr, col, w = f.edges.call_graph()
    assert (row_ptr.tolist(), col.tolist(), w.tolist()) == ([0, 2, 2, 2, 2], [1, 2], [20.0, 20.0])
    ranking = anomod.rank(f, ctx=ctx)
    xr, _ = native.pagerank(row_ptr, col, w, np.asarray(p), 0.85, iters=100, tol=1e-10)
    assert [s for s, _ in ranking] == [HAND_SERVICES[i] for i in np.argsort(-xr, kind="stable")]
    assert [s for s, _ in ranking][0] == "db"
    assert sum(abs(dict(ranking)[s] - x) for s, x in zip(HAND_SERVICES, xr)) <= 1e-12


# ------------------------------------------------- the model against features()
def lattice():
    pts = {k: dict(v) for k, v in SWITCHES.items()}
    pts["none"] = {}
    pts["all"] = dict(ALL_ON)
    pts["quantile_load"] = dict(trace_step_s=STEP_S, trace_quantile=50, trace_load=True)
    pts["self_and_critical"] = dict(self_time=True, critical_path=True)
    return pts


@pytest.mark.parametrize("name", ["SN", "TT"])
def test_model_equals_features_over_the_switch_lattice(name, cache):
    exp, bexp = R.case(name)
    ctx = RefContext(cache=cache)
    bases = {"plain": R.run(bexp, ctx)[0], "full": R.run(bexp, ctx, **ALL_ON)[0],
             "self": R.run(bexp, ctx, self_time=True)[0],
             "critical": R.run(bexp, ctx, critical_path=True)[0]}
    seen = set()
    for point, kw in lattice().items():
        for bname, base in [("none", None)] + list(bases.items()):
            f, zs = R.run(exp, ctx, baseline=base, **kw)
            m = check(exp, f, base, zs)
            seen.add(m.get("latency_kind"))
            # the latency kind: the first of critical / self whose table both runs hold
            if "latency_kind" in m:
                cp = kw.get("critical_path") and base is not None and base.cp_edges is not None
                st = kw.get("self_time") and base is not None and base.self_edges is not None
                assert m["latency_kind"] == ("critical" if cp else "self" if st else "inclusive")
            assert ("shape_novelty" in m) == bool(kw.get("shapes") and bname == "full")
    assert seen == {None, "critical", "self", "inclusive"}
    # the three kinds differ on these inputs, so a swapped precedence shows
    full = bases["full"]
    lat = {k: R.run(exp, ctx, baseline=full, **kw)[0].params["components"]["latency"]
           for k, kw in (("critical", dict(self_time=True, critical_path=True)),
                         ("self", dict(self_time=True)), ("inclusive", {}))}
    assert not np.array_equal(lat["critical"], lat["self"])
    assert not np.array_equal(lat["self"], lat["inclusive"])


def _same(a, b, what):
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), what
    else:
        assert a == b, what


@pytest.mark.parametrize("name", ["SN", "TT"])
def test_switch_independence(name, cache):
    """A switch leaves every component and table it shares with the run
    without it bit-identical, and moves the score by exactly its term."""
    exp, bexp = R.case(name)
    ctx = RefContext(cache=cache)
    base = R.run(bexp, ctx, **ALL_ON)[0]
    additive = {"trace": "trace", "spectrum": "spectrum", "spectrum_all": "spectrum",
                "shapes": "shape_novelty", "trace_load": "load"}
    on_trace = ("trace_load", "trace_quantile")     # these two need the trace series on
    for off_kw, points in (({}, [p for p in SWITCHES if p not in on_trace]),
                           (dict(trace_step_s=STEP_S), on_trace)):
        f0, _ = R.run(exp, ctx, baseline=base, **off_kw)
        t0 = R.integer_tables(f0)
        for point in points:
            kw = dict(off_kw, **SWITCHES[point])
            f1, _ = R.run(exp, ctx, baseline=base, **kw)
            c0, c1 = f0.params["components"], f1.params["components"]
            replaced = {"self_time": {"latency"}, "critical_path": {"latency"},
                        "error_origins": {"error_rate"},
                        "trace_quantile": {"trace"} if off_kw else set()}.get(point, set())
            for k in c0:
                if k not in replaced:
                    _same(c0[k], c1[k], (point, k))
            t1 = R.integer_tables(f1)
            for k in t0:
                if not (point == "trace_quantile" and k in ("edge_windows.q_pct",
                                                            "edge_windows.outside")):
                    _same(t0[k], t1[k], (point, k))
            if f0.window_scores is not None:
                _same(f0.window_scores, f1.window_scores, point)
            comp = additive.get(point)
            if comp is not None:
                want = f0.service_scores + 0.25 * c1[comp]
                assert np.array_equal(f1.service_scores, want), point
                assert c1[comp].any() or (point, name) == ("shapes", "SN"), point
            elif point == "exemplars":
                assert np.array_equal(f1.service_scores, f0.service_scores)
                assert f1.exemplars.k == 4 and f1.error_exemplars.which == 1
                assert int(f1.exemplars.n_found.sum()) > 0
            elif point in ("self_time", "critical_path", "error_origins"):
                k = next(iter(replaced))
                rest0 = f0.service_scores - c0[k]
                np.testing.assert_allclose(f1.service_scores - c1[k], rest0, rtol=1e-12)
                assert not np.array_equal(c0[k], c1[k]), point


def test_switch_prerequisites():
    exp, _ = R.case("SN")
    ctx = RefContext()
    with pytest.raises(ValueError, match="trace_load"):
        anomod.features(exp, ctx, trace_load=True)
    with pytest.raises(ValueError, match="trace_quantile"):
        anomod.features(exp, ctx, trace_quantile=50)
    for q in (-1, 100):
        with pytest.raises(ValueError, match="percentage"):
            anomod.features(exp, ctx, trace_step_s=STEP_S, trace_quantile=q)
    assert not ctx.log and not ctx.cache    # refused before any table is computed


# ------------------------------------------------------------ degenerate shapes
SMALL = dict(topology="SN", n_traces=200, seed=5)


@pytest.mark.parametrize("n_windows", [4, 6])
def test_one_score_window_gives_no_trace_or_load_term(n_windows):
    """T < W and T == W: the only score window is the dropped one."""
    exp = R.synth_experiment(fault="media-service", n_windows=n_windows, **SMALL)
    f, zs = R.run(exp, RefContext(), trace_step_s=STEP_S, trace_W=6, trace_load=True)
    assert f.edge_windows.n_windows == n_windows and zs["trace"].shape[0] == 1
    check(exp, f, None, zs)
    comp = f.params["components"]
    assert not comp["trace"].any() and not comp["load"].any()
    assert not f.trace_window_scores.any()


@pytest.mark.parametrize("n_scores", [20, 21, 40, 41])
def test_top_k_at_its_steps(n_scores):
    """k = max(1, n // 20): 1 up to 39 windows, 2 from 40; the trace and load
    series count the windows left after the drop."""
    exp = R.synth_experiment(fault="media-service", n_windows=2 * n_scores,
                             metric_steps=12 * n_scores, **SMALL)
    f, zs = R.run(exp, RefContext(), W=12, trace_step_s=STEP_S, trace_W=2, trace_load=True)
    assert zs["metric"].shape[0] == zs["trace"].shape[0] == zs["load"].shape[0] == n_scores
    m = check(exp, f, None, zs)
    # the raw trace score is the plain top-k mean of the best column
    S = len(exp.services)
    k = 2 if n_scores == 41 else 1
    rows = R.active_rows(f.edge_windows.count)
    best = [0.0] * S
    for j in range(zs["trace"].shape[1]):
        col = sorted(zs["trace"][1:, j].astype(np.float64).tolist())
        best[rows[j // 2] % S] = max(best[rows[j // 2] % S], sum(col[-k:]) / k)
    np.testing.assert_allclose(f.trace_window_scores, best, rtol=1e-15)
    np.testing.assert_allclose(m["trace_raw"], best, rtol=1e-15)


def test_no_metrics_and_a_matrix_without_series(cache):
    exp, bexp = R.case("SN")
    ctx = RefContext(cache=cache)
    none = anomod.Experiment("none", exp.spans, None)
    empty = anomod.Experiment("empty", exp.spans,
                              MetricMatrix(np.zeros((24, 0), np.float32), np.arange(24.0), []))
    base = R.run(bexp, ctx)[0]
    fs = []
    for e in (none, empty):
        f, zs = R.run(e, ctx, baseline=base, trace_step_s=STEP_S)
        assert "metric" not in zs and f.window_scores is None and f.series is None
        check(e, f, base, zs)
        assert not f.params["components"]["metric"].any()
        fs.append(f)
    assert np.array_equal(fs[0].service_scores, fs[1].service_scores)
    with_m, _ = R.run(exp, ctx, baseline=base, trace_step_s=STEP_S)
    assert np.array_equal(with_m.service_scores,
                          (fs[0].service_scores - 0.25 * fs[0].params["components"]["trace"]
                           + 0.25 * with_m.params["components"]["metric"])
                          + 0.25 * with_m.params["components"]["trace"])


def test_baseline_over_a_disjoint_service_set(cache):
    exp, _ = R.case("SN")
    _, other = R.case("TT")
    ctx = RefContext(cache=cache)
    base = R.run(other, ctx, **ALL_ON)[0]
    assert not set(base.edges.services) & set(exp.services)
    f, zs = R.run(exp, ctx, baseline=base, **ALL_ON)
    m = check(exp, f, base, zs)
    assert m["latency_kind"] == "critical" and not any(m["latency"])
    # no threshold can be taken from such a baseline: the labels are the error flags'
    assert (f.spectrum.thr_us == 0xFFFFFFFF).all()
    # every shape is new
    held = np.asarray(m["shape_novelty"])
    assert set(held.tolist()) <= {0.0, 1.0} and held.any()


def test_empty_span_set():
    svcs = ["a", "b", "c"]
    z = np.zeros(0, np.uint64)
    sp = anomod.SpanSet(svcs, np.zeros(1, np.uint64), z, z, z, z, z, z, None, True, start_us=z)
    exp = anomod.Experiment("empty", sp, None)
    ctx = RefContext()
    f, zs = R.run(exp, ctx, **ALL_ON)
    assert zs == {} and f.edge_windows.n_windows == 1
    m = check(exp, f, None, zs)
    assert f.service_scores.tolist() == [0.0, 0.0, 0.0] == m["score"]
    # nothing positive: the uniform restart
    assert m["personalization"] == [1.0 + 3e-9] * 3
    ranking = anomod.rank(f, ctx=ctx)
    np.testing.assert_allclose([x for _, x in ranking], 1 / 3, rtol=1e-12)


# ------------------------------------------------------------ non-finite inputs
def _uniform(ctx, f):
    """Whether rank(f) answers what the uniform restart vector gives."""
    row_ptr, col, w = f.edges.call_graph()
    xu, _ = native.pagerank(row_ptr, col, w, np.ones(len(f.edges.services)), 0.85, 100, 1e-10)
    got = dict(anomod.rank(f, ctx=ctx))
    return np.abs(np.array([got[s] for s in f.edges.services]) - xu).sum() < 1e-9


@pytest.mark.parametrize("kind", ["inf", "nan", "f32_range"])
def test_bad_metric_series_stays_with_its_service(kind, cache):
    exp, bexp = R.case("SN")
    ctx = RefContext(cache=cache)
    base = R.run(bexp, ctx)[0]
    f0, _ = R.run(exp, ctx, baseline=base, trace_step_s=STEP_S)
    bad = R.with_bad_series(exp, kind)
    f1, zs = R.run(bad, ctx, baseline=base, trace_step_s=STEP_S)
    col = zs["metric"][:, -1]
    if kind == "nan":
        assert not col.any()              # a series without a sample scores nothing
    else:
        assert np.isposinf(col[-1]) and np.isfinite(col[:-1]).all()
    m = check(bad, f1, base, zs)
    assert np.isfinite(f1.service_scores).all()
    assert np.array_equal(f1.service_scores[:-1], f0.service_scores[:-1])
    ms0, ms1 = f0.params["components"]["metric"], f1.params["components"]["metric"]
    assert ms1[-1] == (ms0[-1] if kind == "nan" else 1.0) == m["metric"][-1]
    assert not _uniform(ctx, f1)
    # the ranking is the model's personalization through the oracle's PageRank
    row_ptr, col_, w = f1.edges.call_graph()
    xr, _ = native.pagerank(row_ptr, col_, w, np.asarray(m["personalization"]), 0.85, 100, 1e-10)
    ranking = anomod.rank(f1, ctx=ctx)
    assert [s for s, _ in ranking] == [exp.services[i] for i in np.argsort(-xr, kind="stable")]


@pytest.mark.parametrize("value", [np.inf, np.nan])
@pytest.mark.parametrize("which", ["metric", "trace", "load"])
def test_non_finite_window_score_in_one_column(which, value, cache):
    """A kernel's window score may itself be inf or NaN (the oracle never
    answers NaN): inject one into a column of each scored series."""
    exp, bexp = R.case("SN")
    base = R.run(bexp, RefContext(cache=cache))[0]
    kw = dict(trace_step_s=STEP_S, trace_load=True)
    f0, zs0 = R.run(exp, RefContext(cache=cache), baseline=base, **kw)
    S = len(exp.services)
    if which == "metric":
        j = 4
        victim = R.series_service(f0.series[j], exp.services)
    else:
        rows = (R.active_rows(f0.edge_windows.count) if which == "trace"
                else R.active_rows(f0.edge_load.busy_us, f0.edge_load.carried))
        j = 5
        victim = rows[j // 2 if which == "trace" else j] % S

    def hook(name, Z):
        if name == which:
            Z = Z.copy()
            Z[2, j] = value
        return Z

    ctx = RefContext(cache=cache, z_hook=hook)
    f1, zs = R.run(exp, ctx, baseline=base, **kw)
    assert not np.isfinite(zs[which][2, j])
    m = check(exp, f1, base, zs)
    assert np.isfinite(f1.service_scores).all()
    others = np.arange(S) != victim
    assert np.array_equal(f1.service_scores[others], f0.service_scores[others])
    c0, c1 = f0.params["components"][which], f1.params["components"][which]
    if value == np.inf:
        assert c1[victim] == 1.0
    else:
        # the column is skipped: the service keeps the best of its other columns
        skipped = zs0[which].astype(np.float64).copy()
        skipped[:, j] = 0.0
        x = R.inputs_of(exp, f0, base, dict(zs0, **{which: skipped.astype(zs0[which].dtype)}))
        assert c1[victim] == R.model(x)[which][victim] <= c0[victim]
    assert not _uniform(ctx, f1)


def test_rank_keeps_the_finite_scores():
    """rank() itself: a non-finite score counts as 0, the rest still steer the
    restart; the uniform vector only when nothing positive remains."""
    exp, _ = R.case("SN")
    ctx = RefContext()
    f, _ = R.run(exp, ctx)
    row_ptr, col, w = f.edges.call_graph()
    good = f.service_scores.copy()
    for bad in (np.nan, np.inf, -np.inf):
        f.service_scores = good.copy()
        f.service_scores[3] = bad
        p = R.personalization(f.service_scores)
        assert math.isclose(p[3], 1e-9 * float(np.delete(good, 3).sum()), rel_tol=1e-12)
        xr, _ = native.pagerank(row_ptr, col, w, np.asarray(p), 0.85, 100, 1e-10)
        got = dict(anomod.rank(f, ctx=ctx))
        assert np.abs(np.array([got[s] for s in exp.services]) - xr).sum() <= 1e-12
        assert not _uniform(ctx, f)
    for nothing in (np.zeros_like(good), np.full_like(good, np.nan)):
        f.service_scores = nothing
        assert R.personalization(nothing) == [1.0 + len(good) * 1e-9] * len(good)
        assert _uniform(ctx, f)


# ---------------------------------------------------------------------- ranking
@pytest.mark.parametrize("name", ["SN", "TT"])
def test_ranking_equals_model_personalization_through_pagerank(name, cache):
    exp, bexp = R.case(name)
    ctx = RefContext(cache=cache)
    base = R.run(bexp, ctx, **ALL_ON)[0]
    for kw in ({}, ALL_ON):
        f, zs = R.run(exp, ctx, baseline=base, **kw)
        m = check(exp, f, base, zs)
        row_ptr, col, w = f.edges.call_graph()
        xr, _ = native.pagerank(row_ptr, col, w, np.asarray(m["personalization"]), 0.85,
                                iters=100, tol=1e-10)
        ranking = anomod.rank(f, ctx=ctx)
        assert [s for s, _ in ranking] == [exp.services[i] for i in np.argsort(-xr, kind="stable")]
        got = dict(ranking)
        assert np.abs(np.array([got[s] for s in exp.services]) - xr).sum() <= 1e-12
        assert np.abs(np.asarray(m["personalization"]) - np.asarray(m["score"])
                      - 1e-9 * sum(m["score"])).max() <= 1e-15


# ------------------------------------------------- the enclosure is not vacuous
@pytest.mark.parametrize("name,point", [(n, p) for n in R.GPU_POINTS for p in R.GPU_POINTS[n]])
def test_score_interval_is_narrow_beside_the_score_gaps(name, point, cache):
    """The GPU test encloses the kernels' service scores in the model's
    interval over Z_ref -+ bound.  From the references alone: the interval is
    at most 1/100 of the smallest non-zero gap between two services'
    reference scores, so a score inside it cannot have changed places."""
    exp, bexp = R.case(name)
    ctx = RefContext(cache=cache)
    kw = R.gpu_point(point)
    base = R.run(bexp, ctx, **kw)[0]
    f, _ = R.run(exp, ctx, baseline=base, **kw)
    lo, mid, hi = R.score_interval(exp, f, base, [c[:5] for c in ctx.log])
    assert (lo <= mid).all() and (mid <= hi).all()
    width, gap = float((hi - lo).max()), R.smallest_gap(mid)
    print(f"{name}/{point}: width {width:.3e}, smallest gap {gap:.3e}")
    assert width <= gap / 100
    # and the oracle's f32 scores, a kernel within the bound, lie inside
    assert (lo - 1e-12 <= f.service_scores).all() and (f.service_scores <= hi + 1e-12).all()

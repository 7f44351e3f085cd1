"""GPU: features() / rank() on the real context against the same composition
on RefContext (tests/engine_ref.py), over the SN (~2,000 traces) and TT (~300
traces) experiments of engine_ref.CASES at engine_ref.GPU_POINTS:

* every integer table of Features equals the references', bit for bit;
* the service scores lie inside the model's interval over the double-double
  EWMA reference's window scores -+ the kernels' bound (every squashed z-term
  is monotone non-decreasing in each window score), padded by 1e-12 —
  tests/test_engine_model_host.py shows from the references alone that this
  interval is under 1/100 of the smallest gap between two services' scores;
* the ranking order equals RefContext's;
* a series with an inf sample leaves the scores finite, the other services
  inside their intervals and the restart vector steered by the scores."""
import numpy as np
import pytest

import anomod

import engine_ref as R
from engine_ref import RefContext

pytestmark = pytest.mark.gpu

POINTS = [(n, p) for n in R.GPU_POINTS for p in R.GPU_POINTS[n]]


@pytest.fixture(scope="module")
def cache():
    return {}


def both(ctx, cache, exp, bexp, kw):
    """(GPU features, reference features, reference baseline, EWMA calls)."""
    rctx = RefContext(cache=cache)
    base_r = R.run(bexp, rctx, **kw)[0]
    f_r, _ = R.run(exp, rctx, baseline=base_r, **kw)
    calls = [c[:5] for c in rctx.log]
    base_g = anomod.features(bexp, ctx, **kw)
    R.assert_integer_tables_equal(base_g, base_r)
    f_g = anomod.features(exp, ctx, baseline=base_g, **kw)
    return f_g, f_r, base_r, calls


def assert_enclosed(scores, lo, hi, who=slice(None)):
    s = np.asarray(scores)[who]
    print("score - low:", (s - lo[who]).min(), " high - score:", (hi[who] - s).min(),
          " width:", (hi[who] - lo[who]).max())
    assert np.isfinite(s).all()
    assert (lo[who] - 1e-12 <= s).all() and (s <= hi[who] + 1e-12).all()


@pytest.mark.parametrize("name,point", POINTS)
def test_tables_and_score_enclosure(ctx, cache, name, point):
    exp, bexp = R.case(name)
    kw = R.gpu_point(point)
    f_g, f_r, base_r, calls = both(ctx, cache, exp, bexp, kw)
    R.assert_integer_tables_equal(f_g, f_r)
    assert f_g.series == f_r.series
    for k in ("latency_kind", "error_kind", "spectrum_thresholds"):
        assert f_g.params["components"].get(k) == f_r.params["components"].get(k)
    lo, mid, hi = R.score_interval(exp, f_r, base_r, calls)
    assert_enclosed(f_g.service_scores, lo, hi)


@pytest.mark.parametrize("name", list(R.GPU_POINTS))
def test_ranking_order(ctx, cache, name):
    exp, bexp = R.case(name)
    f_g, f_r, _, _ = both(ctx, cache, exp, bexp, R.gpu_point("all"))
    got = anomod.rank(f_g, ctx=ctx)
    want = anomod.rank(f_r, ctx=RefContext())
    assert [s for s, _ in got] == [s for s, _ in want]
    np.testing.assert_allclose([x for _, x in got], [x for _, x in want], rtol=0, atol=1e-6)


def test_inf_sample_stays_with_its_service(ctx, cache):
    exp, bexp = R.case("SN")
    bad = R.with_bad_series(exp, "inf")
    kw = R.gpu_point("trace_load")
    f_g, f_r, base_r, calls = both(ctx, cache, bad, bexp, kw)
    R.assert_integer_tables_equal(f_g, f_r)
    lo, mid, hi = R.score_interval(bad, f_r, base_r, calls)
    others = slice(0, len(exp.services) - 1)    # the bad series belongs to the last service
    assert np.isfinite(f_g.service_scores).all()
    assert_enclosed(f_g.service_scores, lo, hi, others)
    # the restart vector is the scores', not the uniform one
    row_ptr, col, w = f_g.edges.call_graph()
    xu, _ = ctx.pagerank(row_ptr, col, w, np.ones(len(exp.services)))
    got = dict(anomod.rank(f_g, ctx=ctx))
    x = np.array([got[s] for s in exp.services])
    p = np.asarray(R.personalization(f_g.service_scores))
    xp, _ = ctx.pagerank(row_ptr, col, w, p)
    assert np.abs(x - xp).sum() <= 1e-12 and np.abs(x - xu).sum() > 1e-3

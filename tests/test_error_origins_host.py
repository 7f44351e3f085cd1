"""Error origins, host side (no GPU): the C entry point's export and NULL
handling, the reference model (tests/error_origins_ref.py) on a hand-made
trace and its invariants on synthetic sets with propagated errors, the
conditions the GPU parity inputs must meet, the helpers of ErrorOrigins and the
CLI flag."""
import ctypes as C
import inspect
import subprocess
import sys

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from conftest import PKG_DIR
from oracle import native

from error_origins_ref import (ABSORBER, CONTAINED, LOOP, ORIGIN, PROPAGATED, SURFACED, build,
                               hand_made, inclusive_error_rate, origins_ref, propagate_errors,
                               span_classes_ref)
from self_time_ref import parents_ref
from test_self_time_host import FAULTS, synth

# propagate_errors parameters of the synthetic parity sets (CPU here, GPU in
# test_gpu_error_origins): half of the fault service's spans fail, and a
# failure climbs to the caller with probability 0.7 per step
SHARE, P_UP, SEED = 0.5, 0.7, 7


def propagated(topo, n_traces):
    sp = synth(topo, n_traces)
    return propagate_errors(sp, FAULTS[topo], SHARE, P_UP, np.random.default_rng(SEED))


# ------------------------------------------------------------------ surface
def test_library_exports_the_entry_point():
    assert "anomod_error_origins_spans" in anomod.EXPORTED_SYMBOLS
    lib = anomod.lib()
    cs = L.ErrorOriginsC(1)
    assert lib.anomod_error_origins_spans(None, None, C.byref(cs)) == L.EINVAL
    assert b"anomod_error_origins_spans" in lib.anomod_last_error(None)


def test_python_surface():
    p = inspect.signature(anomod.features).parameters
    assert "error_origins" in p and p["error_origins"].default is False
    assert "error_origins" in anomod.Features.__dataclass_fields__
    q = inspect.signature(anomod.Context.error_origins).parameters
    assert list(q)[1:] == ["spans", "per_span"] and q["per_span"].default is False


def test_cli_lists_the_flag():
    r = subprocess.run([sys.executable, "-m", "anomod", "features", "--help"], cwd=PKG_DIR,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--error-origins" in r.stdout


# ------------------------------------------------------------------ the model
def test_reference_on_the_hand_made_trace():
    sp, cls, fate, hops = hand_made()
    par = parents_ref(sp)
    assert par.tolist() == [1, -1, 1, 1, 3, 4, 5, -1, -1, 1, 1, 9]
    assert span_classes_ref(sp, par) == (cls, fate, hops)
    r = origins_ref(sp, par)
    S = 3
    row = lambda p, c: p * S + c  # noqa: E731  (ROOT = S, ORPHAN = S + 1)
    assert r.error_spans == 9 and r.loop_spans == 0
    want = np.zeros((S + 2) * S, np.int64)
    for p, c in ((1, 0), (1, 2), (2, 0), (1, 1), (S + 1, 2), (0, 2)):   # spans 0, 2, 6, 7, 8, 11
        want[row(p, c)] += 1
    np.testing.assert_array_equal(r.origin, want)
    assert r.propagated[row(S, 1)] == 1 and r.propagated[row(0, 1)] == 1      # spans 1, 4
    assert r.propagated[row(1, 2)] == 1 and int(r.propagated.sum()) == 3      # span 5
    assert r.stopped[row(0, 1)] == 1 and r.stopped[row(0, 2)] == 1 and int(r.stopped.sum()) == 2
    assert int(r.surfaced.sum()) == 4 and r.surfaced[row(2, 0)] == 0          # span 6: contained
    assert r.absorbers[row(1, 0)] == 2 and int(r.absorbers.sum()) == 2        # spans 3, 9
    assert r.hops_sum[row(2, 0)] == 2 and r.hops_max[row(2, 0)] == 2          # span 6
    assert int(r.hops_sum.sum()) == 4 and r.hops_max[row(1, 0)] == 1
    np.testing.assert_array_equal(r.origin + r.propagated, native.edge_aggregate(sp)["errors"])


def test_reference_cycle_is_a_loop_and_a_self_reference_is_not():
    """1 -> 2 -> 3 -> 1 all flagged, 4 hangs off 1; 9 names itself."""
    ids, pids = [1, 2, 3, 4, 9, 10], [2, 3, 1, 1, 9, 9]
    sp = build(2, [(ids, pids, [1, 1, 1, 1, 1, 1], [0, 1, 0, 1, 0, 1])])
    cls, fate, hops = span_classes_ref(sp)
    assert fate == [LOOP, LOOP, LOOP, LOOP, SURFACED, SURFACED]
    assert hops == [0, 0, 0, 0, 0, 1]
    assert cls == [PROPAGATED, PROPAGATED, PROPAGATED, ORIGIN, PROPAGATED, ORIGIN]
    r = origins_ref(sp)
    assert r.loop_spans == 4 and r.error_spans == 6 and int(r.stopped.sum()) == 0
    # an unflagged member ends every chain of the cycle
    sp = build(2, [(ids, pids, [1, 0, 1, 1, 1, 1], [0, 1, 0, 1, 0, 1])])
    cls, fate, hops = span_classes_ref(sp)
    assert fate[:4] == [CONTAINED, 0, CONTAINED, CONTAINED] and hops[:4] == [0, 0, 1, 1]
    assert cls[1] == ABSORBER and origins_ref(sp).loop_spans == 0


@pytest.fixture(scope="module", params=["SN", "TT"])
def small_case(request):
    sp = propagated(request.param, 3000)
    return request.param, sp, origins_ref(sp)


def test_reference_invariants(small_case):
    topo, sp, r = small_case
    S, c = sp.n_services, sp.services.index(FAULTS[topo])
    np.testing.assert_array_equal(r.origin + r.propagated, native.edge_aggregate(sp)["errors"])
    off = np.arange((S + 2) * S) % S != c
    assert r.origin[~off].sum() > 0 and not r.origin[off].any()
    assert (np.delete(inclusive_error_rate(sp), c) > 0).any()
    # every origin is surfaced, contained or in a loop; hops only for origins' chains
    org = r.cls == ORIGIN
    assert int(r.surfaced.sum()) == int((org & (r.fate == SURFACED)).sum())
    assert r.loop_spans == 0 and int(r.hops_sum.sum()) == int(r.hops[org].sum())
    assert int(r.hops_max.max()) == int(r.hops[org].max())
    # one stopped span per contained chain top: an absorber sits above each
    assert 0 < int(r.stopped.sum()) <= int(r.propagated.sum() + r.origin.sum())
    assert int(r.absorbers.sum()) <= int(r.stopped.sum())


@pytest.mark.parametrize("topo", ["SN", "TT"])
def test_parity_inputs_are_not_degenerate(topo):
    """The conditions on the 20,000-trace sets the GPU parity test uses."""
    sp = propagated(topo, 20000)
    r = origins_ref(sp)
    n = sp.n_spans
    shares = {k: float((r.cls == v).sum()) / n
              for k, v in (("origin", ORIGIN), ("propagated", PROPAGATED), ("absorber", ABSORBER))}
    org = r.cls == ORIGIN
    fates = {k: int((org & (r.fate == v)).sum()) for k, v in (("surfaced", SURFACED),
                                                              ("contained", CONTAINED))}
    print(topo, "class shares:", shares, "origin fates:", fates, "max hops:",
          int(r.hops[org].max()))
    assert min(shares.values()) >= 0.01
    assert min(fates.values()) >= 100
    assert int(r.hops[org].max()) >= 3


# ------------------------------------------------------------------ helpers
def test_error_origins_helpers():
    eo = anomod.ErrorOrigins.empty(["a", "b"])
    E = 8
    assert all(getattr(eo, k).shape == (E,) for k in eo.TABLES) and eo.span_state is None
    eo.origin[[0, 2, 5]] = [3, 1, 2]          # rows p * 2 + c: a -> a, b -> a, ROOT -> b
    eo.surfaced[[0, 5]] = [1, 2]
    eo.hops_sum[[0, 5]] = [6, 1]
    count = np.array([10, 0, 0, 0, 10, 4, 0, 0], np.uint64)
    np.testing.assert_array_equal(eo.origin_rate(count), [4 / 20, 2 / 4])
    np.testing.assert_array_equal(eo.origin_rate(np.array([0, 8])), [0.0, 2 / 8])
    np.testing.assert_array_equal(eo.surfaced_share(), [1 / 4, 1.0])
    np.testing.assert_array_equal(eo.mean_hops(), [6 / 4, 1 / 2])
    with pytest.raises(ValueError):
        eo.origin_rate(np.zeros(3))
    from anomod.__main__ import error_origins_doc
    eo.error_spans, eo.loop_spans = 9, 1
    doc = error_origins_doc(eo)
    assert doc["loop_spans"] == 1 and doc["error_spans"] == 9
    assert doc["services"]["a"] == {"origin": 4, "propagated": 0, "surfaced": 1, "mean_hops": 1.5}
    import json
    json.dumps(doc)

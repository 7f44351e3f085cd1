"""GPU: the five passes that resolve parents through the shared span walk
(csrc/walk.h, csrc/chunk.h: self time, critical path, trace shapes, trace
spectrum, error origins) on the border cases of tests/walk_ref.py — chunks
closed by the 64-trace limit, by the 256-span sum and by a segment border,
trace starts on the mask-word borders, parents at every slot of the scans'
blocks with decoys in the neighbouring traces, the long-trace table with a
wrapping cluster and parents on its window and block borders — each against
the pass's own reference helper, bit for bit: every value is an integer, no
tolerance anywhere (p50 / p99 with NaNs equal).

A case is uploaded once and the five passes run on the same device set; the
logged kernel variant and long-trace count must be the model's (a silent
fallback to another scan fails), and an edge aggregation after the passes must
still equal the C oracle's.  test_walk_ref_host.py proves on the host that
every case reaches the border it names.  Not covered: big_parents' guard for a
trace of 2^32 - 2 spans (no test can hold such a set)."""
import numpy as np
import pytest

import walk_ref as W
from oracle import native
from self_time_ref import assert_table_equal
from test_gpu_critical_path import _check as check_critical_path
from test_gpu_error_origins import _check as check_error_origins
from test_gpu_spectrum import _check as check_spectrum
from test_gpu_summaries import _cus
from test_gpu_trace_shapes import _check as check_trace_shapes

pytestmark = pytest.mark.gpu

CASES = W.case_names()


@pytest.fixture(scope="module")
def n_cus() -> int:
    return _cus()


def _logged(capfd, kernel, c):
    err = capfd.readouterr().err
    if c.sp.n_spans:   # (a set without spans returns before any kernel is picked)
        want = f"{kernel}<{W.SCAN_LOG[c.scan]}>, {c.n_long} long traces"
        assert want in err, (want, err)


@pytest.mark.parametrize("name", CASES)
def test_case_through_the_five_passes(ctx, monkeypatch, capfd, request, name):
    many = name.startswith("many_long")   # sized by the device: its long-trace grid is 2 per CU
    c = W.case(name, request.getfixturevalue("n_cus")) if many else W.case(name)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    sp, r = c.sp, c.refs
    if many:
        assert c.n_long == 2 * request.getfixturevalue("n_cus") + 88
    d = ctx.upload(sp)

    def self_time():
        su, tab = r["self_time"] if r else (np.zeros(0, np.uint32), None)
        got, got_su = ctx.self_time(d, per_span=True)
        np.testing.assert_array_equal(got_su, su, err_msg="self_us")
        if tab is not None:
            assert_table_equal(got, tab)
        _logged(capfd, "self_time_kernel", c)

    def critical_path():
        check_critical_path(ctx, sp, dev=d, ref=r.get("critical_path"))
        _logged(capfd, "critical_path_kernel", c)

    def trace_shapes():
        check_trace_shapes(ctx, sp, dev=d, ref=r.get("trace_shapes"))
        _logged(capfd, "trace_shapes_kernel", c)

    def spectrum():
        rows = r["spectrum"][0] if r else None
        _, ref_sp = check_spectrum(ctx, sp, c.thr, True, dev=d, rows=rows)
        if r:   # (the helper's reference is the one the host test looked at)
            for k in ref_sp:
                np.testing.assert_array_equal(ref_sp[k], r["spectrum"][1][k], err_msg=k)
        err = capfd.readouterr().err
        if sp.n_spans:
            assert f"long pass {'on' if c.n_long else 'off'}" in err, err

    def error_origins():
        check_error_origins(ctx, sp, dev=d, ref=r.get("error_origins"))
        _logged(capfd, "error_origins_kernel", c)

    def edges_after():   # the passes left the set and its hints alone
        assert_table_equal(ctx.edge_aggregate(d), native.finalize(native.edge_aggregate(sp)))

    # Every pass runs whatever the one before it found, so a failure names all
    # the passes that diverge on the case.
    failed = []
    try:
        capfd.readouterr()
        for check in (self_time, critical_path, trace_shapes, spectrum, error_origins,
                      edges_after):
            assert check.__name__ in W.PASSES + ("edges_after",)
            try:
                check()
            except AssertionError as e:
                failed.append((check.__name__, str(e).strip().splitlines()[:6]))
    finally:
        d.free()
    assert not failed, (name, [f[0] for f in failed], failed)

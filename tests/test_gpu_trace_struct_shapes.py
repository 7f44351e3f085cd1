"""The trace-structure kernels (csrc/trace_struct.hip: ts_chunk<UNI>,
ts_big_kernel, on the chunk walk of csrc/chunk.h) against the graph model of
trace_struct_ref.py on adversarial trace shapes: chains as deep as the chunk
and the long-trace pointer jumping allow, in forward, reversed and shuffled
order; chunks packed to their limits and chunks with empty traces; cycles no
root reaches and cycles a root reaches; a node with a shallow and a deep
parent; ids and parents split across the 4096-id table windows of a long
trace, a cluster of ids in one table slot; more long traces than workgroups;
service indices on the word borders; a set whose longest trace is unknown.
Every shape runs declared-unique (U), undeclared (G) and with a duplicated id
(Din / Dout / D), see trace_struct_ref.py.

Everything is integer-exact: assert_array_equal on all six outputs.
test_trace_struct_ref_host.py holds the model to the C oracle and to the
reference goldens on the same inputs, and checks that every builder reaches
the path it was written for."""
import numpy as np
import pytest

import trace_struct_ref as R
from test_gpu_summaries import _cus

pytestmark = pytest.mark.gpu

CASES = R.case_names()


def _assert_equal(got, ref, what):
    for k in R.FIELDS:
        np.testing.assert_array_equal(getattr(got, k), ref[k], err_msg=f"{what}: {k}")


def _assert_same(a, b, what):
    for k in R.FIELDS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what}: {k}")


@pytest.fixture(scope="module")
def n_cus() -> int:
    """The device's CU count, read as test_gpu_summaries.py reads it."""
    return _cus()


@pytest.mark.parametrize("name", CASES)
def test_shape_matches_model(ctx, monkeypatch, request, name):
    """The reached cycles run the relaxation for all of its 2L + 2
    workgroup-wide rounds by design (16 388 at 8193 spans, tens of
    milliseconds); no case needs a time limit of its own."""
    many = name.startswith("many_long")  # sized by the device: one workgroup per CU
    c = R.case(name, request.getfixturevalue("n_cus")) if many else R.case(name)
    got = ctx.trace_structure(c.sp)
    _assert_equal(got, c.model, name)
    # the same context again: the tail counter and the long-trace counters are
    # re-zeroed, the scratch is reused
    _assert_same(ctx.trace_structure(c.sp), got, f"{name}, second call")
    if c.regime == "U":  # the declaration only picks the kernel
        monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "0")
        _assert_same(ctx.trace_structure(c.sp), got, f"{name}, general scan")


def test_many_long_traces_outnumber_the_workgroups(n_cus):
    c = R.case("many_long-U", n_cus)
    lens = np.diff(c.sp.trace_ptr.astype(np.int64))
    assert int((lens > R.STAGE).sum()) > 2 * n_cus and lens[-1] > R.STAGE


@pytest.mark.parametrize("regime", ["U", "G", "Din"])
def test_unknown_longest_trace_grouped_on_device(ctx, regime):
    """Uploaded in arrival order (the trace of a span known by its hash alone)
    and grouped on the device, a set does not know its longest trace, so the
    long-trace list is sized for the worst case; the grouped download is the
    model's input.  The spans arrive in random order, so the 4097-span chain
    comes out shuffled within its trace, still 4096 deep."""
    c = R.case(f"ungrouped_4097-{regime}")
    order = np.random.default_rng(3).permutation(c.sp.n_spans)
    loose = c.sp.take(order, np.array([0, c.sp.n_spans], np.uint64))
    loose.unique_ids = c.sp.unique_ids
    d = ctx.upload_ungrouped(loose)
    g = ctx.group(d)
    try:
        host = g.download()
        assert host.unique_ids == (regime == "U")
        assert int(np.diff(host.trace_ptr.astype(np.int64)).max()) >= 4097
        ref = R.trace_structure_ref(host)
        assert int(ref["depth"].max()) == 4096
        _assert_equal(ctx.trace_structure(g), ref, f"grouped on the device, {regime}")
    finally:
        g.free()
        d.free()

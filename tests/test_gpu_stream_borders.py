"""GPU: the four passes that run on the shared edge stream (csrc/edge_stream.h,
csrc/edge_stream.hip: the windowed edge table, the edge load, the per-window
quantiles, the edge exemplars) on the border cases of tests/stream_ref.py — a
workgroup range that ends inside a batch, on a batch border or after one span,
a grid that shrinks below its cap, dead spans in front of trace_ptr[0] that end
inside a 16-B vector of either lane layout, on the batch border or cover a
whole batch or a whole workgroup, columns longer than trace_ptr[-1], the window
ring wrapping exactly at Wt, jumping by a whole tile, going backwards, meeting
batches without a window, straddling its tile and cut by T in finish(), a cell
border of the sorted keys on a wave's first lane, a run start, a batch, a range
and the sentinel run, exemplar winners on both sides of a range border — each
against the pass's own reference helper, bit for bit: every value is an
integer, no tolerance anywhere.

A case is uploaded once: its passes run on the device set in the keys form,
then, after one edge aggregation has left the parent rows in place, in the rows
form (the windowed table and the quantiles have the keys form only and run
twice).  Every launch must log the modelled form, tile windows, grid and spans
per workgroup (ANOMOD_LOG_KERNEL=1), so a silent change of geometry that takes
a case off its border fails; an edge aggregation after the passes must still
equal the C oracle's.  test_stream_ref_host.py proves on the host that every
case reaches the border it names.

Not covered: the kStreamMaxRange clamp of 2^31 spans per workgroup (no test can
hold such a set) and the occupancy-derived default grid (it depends on the
device; the per-pass tests run it without a workgroup cap)."""
import ctypes as C
import os

import numpy as np
import pytest

import stream_ref as S
from anomod import _lib as L
from edge_exemplars_ref import assert_exemplars_equal
from edge_load_ref import FIELDS as LOAD_FIELDS
from edge_load_ref import assert_load_equal
from edge_window_quantiles_ref import assert_quantiles_equal
from edge_windows_ref import assert_windows_equal
from oracle import native
from self_time_ref import assert_table_equal

pytestmark = pytest.mark.gpu

CASES = S.case_names()
CAPS = sorted({v for pair in S.ENV.values() for v in pair if v} | {"ANOMOD_EXEMPLARS_LDS",
                                                                   "ANOMOD_LOG_KERNEL"})


@pytest.fixture(autouse=True)
def caps_restored():
    """Set up before monkeypatch, so torn down after it: the caps a test set
    through monkeypatch are gone again when it ends."""
    before = {k: os.environ.get(k) for k in CAPS}
    yield
    assert {k: os.environ.get(k) for k in CAPS} == before


def _setenv(monkeypatch, c, tile="case", lds=None):
    env = c.env(tile=tile, lds=lds)
    for k in CAPS:
        if k in env:
            monkeypatch.setenv(k, env[k])
        elif k != "ANOMOD_LOG_KERNEL":
            monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    assert all(os.environ[k] == v for k, v in env.items())


def _logged(capfd, kernel, form, grid, per_wg, tile=None, lists=None):
    err = capfd.readouterr().err
    want = (f"anomod: stream {kernel}<{form}>"
            + (f", tile {tile} windows" if tile is not None else "")
            + (f", lists {lists}" if lists else "")
            + f", grid {grid}, {per_wg} spans per workgroup\n")
    assert want in err, (want, err)


@pytest.mark.parametrize("name", CASES)
def test_case_through_its_passes(ctx, monkeypatch, capfd, name):
    c = S.case(name)
    sp, refs = c.sp, c.refs()
    t0, step, T = c.t0, c.step, c.T
    d = ctx.upload(sp)

    def windows(form, tile="case"):
        _setenv(monkeypatch, c, tile)
        capfd.readouterr()
        got = ctx.edge_windows(d, t0, step, T)
        (k, _, grid, per_wg), = S.geometry(c, "windows")
        t = c.tile if tile == "case" else tile
        Wt = S.tile_of("windows", c.E, T, S.NO_CAP if t is None else t)
        _logged(capfd, k, "keys", grid, per_wg, tile=Wt)
        assert_windows_equal(got, refs["windows"])
        return got

    def load(form, tile="case", outputs=LOAD_FIELDS):
        _setenv(monkeypatch, c, tile)
        capfd.readouterr()
        got = ctx.edge_load(d, t0, step, T, outputs=outputs)
        (k, _, grid, per_wg), = S.geometry(c, "load")
        t = c.tile if tile == "case" else tile
        Wt = S.tile_of("load", c.E, T, S.NO_CAP if t is None else t, busy="busy_us" in outputs)
        _logged(capfd, k, form, grid, per_wg, tile=Wt)
        assert_load_equal(got, refs["load"], fields=outputs)
        for f in LOAD_FIELDS:
            if f not in outputs:
                assert not getattr(got, f).any()   # never written
        return got

    def quantiles(form):
        _setenv(monkeypatch, c)
        capfd.readouterr()
        got = ctx.edge_window_quantiles(d, t0, step, T, with_table=False)
        err = capfd.readouterr().err
        for k, _, grid, per_wg in S.geometry(c, "quantiles"):
            want = f"anomod: stream {k}<keys>, grid {grid}, {per_wg} spans per workgroup\n"
            assert want in err, (want, err)
        assert_quantiles_equal(got, refs["quantiles"])

    def exemplars(form):
        (kern, _, grid, per_wg), = S.geometry(c, "exemplars")
        for k in c.ks:
            for place in c.places:
                lds = {"lds": None, "global": 0, "cached": c.E * 8}[place]
                _setenv(monkeypatch, c, lds=lds)
                capfd.readouterr()
                got = ctx.edge_exemplars(d, k, errors_only=c.errors_only)
                lists = S.exemplars_place(c.E, k, S.NO_CAP if lds is None else lds)
                assert lists == place or (k == 1 and place == "cached")   # E * 8 holds K = 1
                _logged(capfd, kern, form, grid, per_wg, lists=lists)
                try:
                    assert_exemplars_equal(got, refs["exemplars"][k])
                except AssertionError as e:
                    raise AssertionError(f"k={k} lists {place}: {e}") from None

    def ring_extra(form):
        """c8: tile 0, every span to global atomics — equal to the tiled run;
        the load pass with only one of its tables asked for."""
        tiled_w, tiled_l = windows(form), load(form)
        flat_w, flat_l = windows(form, tile=0), load(form, tile=0)
        for f in ("count", "errors", "sum_us", "max_us"):
            np.testing.assert_array_equal(getattr(flat_w, f), getattr(tiled_w, f), err_msg=f)
        for f in LOAD_FIELDS:
            np.testing.assert_array_equal(getattr(flat_l, f), getattr(tiled_l, f), err_msg=f)
        load(form, outputs=("carried",))   # no ring at all
        load(form, outputs=("busy_us",))

    def rows_in_place():
        ctx.edge_aggregate(d, with_hist=False)
        out = np.zeros(d.n_spans, np.uint16)
        assert L.lib().anomod_spans_parent_rows(ctx.handle, d.handle, L.ptr(out, C.c_uint16),
                                                len(sp.services)) == L.OK

    def edges_after():   # the passes left the set and its hints alone
        assert_table_equal(ctx.edge_aggregate(d), native.finalize(native.edge_aggregate(sp)))

    checks = {"windows": windows, "load": load, "quantiles": quantiles, "exemplars": exemplars}
    # Every pass runs whatever the one before it found, so a failure names all
    # the passes and forms that diverge on the case.
    failed = []
    try:
        for form in ("keys", "rows"):
            if form == "rows":
                rows_in_place()
            todo = [checks[p] for p in c.passes] + ([ring_extra] if c.ring_extra else [])
            for check in todo:
                try:
                    check(form)
                except AssertionError as e:
                    failed.append((check.__name__, form, str(e).strip().splitlines()[:8]))
        try:
            edges_after()
        except AssertionError as e:
            failed.append(("edges_after", "", str(e).strip().splitlines()[:8]))
    finally:
        d.free()
    assert not failed, (name, [f[:2] for f in failed], failed)

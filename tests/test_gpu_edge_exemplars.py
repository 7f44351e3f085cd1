"""GPU: the edge exemplars (csrc/edge_exemplars.hip) against the reference
helper (tests/edge_exemplars_ref.py), bit for bit, in both forms of the stream
kernel (parent rows of a resident set; edge keys from the aggregation's walk)
and both placements of the lists (LDS; global), plus the plumbing, features()
and the CLI.

ANOMOD_EXEMPLARS_WGS / ANOMOD_EXEMPLARS_LDS cap the stream kernel's workgroups
and its LDS budget (0: the lists in global memory, no threshold cache): the
small sets here would otherwise give every workgroup a single batch — results
must not depend on them."""
import ctypes as C
import json
import shutil

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from anomod.spans import EdgeExemplars, edge_rows

from edge_exemplars_ref import assert_exemplars_equal, exemplars_brute, exemplars_ref
from test_edge_exemplars_host import U32, U64, chain_set, cut_set, order_sets, ties_set

pytestmark = pytest.mark.gpu

# (workgroup cap, LDS budget): default geometry, one workgroup walking the whole
# set, three workgroups, the lists in global memory, both
GEOMETRIES = [(None, None), ("1", None), ("3", None), (None, "0"), ("3", "0")]


def _geometry(monkeypatch, geom):
    for name, v in zip(("ANOMOD_EXEMPLARS_WGS", "ANOMOD_EXEMPLARS_LDS"), geom):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def resident(ctx, sp):
    """The set on the device with its parent rows in place (one aggregation)."""
    dev = ctx.upload(sp)
    ctx.edge_aggregate(dev, with_hist=False)
    out = np.zeros(dev.n_spans, np.uint16)
    assert L.lib().anomod_spans_parent_rows(ctx.handle, dev.handle, L.ptr(out, C.c_uint16),
                                            len(dev.services)) == L.OK
    return dev


def _logged(capfd, form, lists=None):
    err = capfd.readouterr().err
    assert f"edge_exemplars_kernel<{form}>" in err, err
    if lists is not None:
        assert f"lists {lists}" in err, err


def both_forms(ctx, sp, cases, capfd, monkeypatch, lists=None, dev=None):
    """Every (k, which, reference) of `cases` in the rows form (a resident set
    after one aggregation) and in the keys form (the host set, uploaded for the
    call): both equal the reference, and the kernel log names the form."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    own = dev is None
    dev = resident(ctx, sp) if own else dev
    for k, which, ref in cases:
        capfd.readouterr()
        got = ctx.edge_exemplars(dev, k, errors_only=bool(which))
        _logged(capfd, "rows", lists)
        assert_exemplars_equal(got, ref)
        keys = ctx.edge_exemplars(sp, k, errors_only=bool(which))
        _logged(capfd, "keys", lists)
        assert_exemplars_equal(keys, ref)
    if own:
        dev.free()


def check_unused(ex):
    """Slots past n_found hold the documented values, the others a position."""
    unused = np.arange(ex.k)[None, :] >= ex.n_found[:, None]
    assert ((ex.position == U64) == unused).all() and ((ex.trace == U64) == unused).all()
    for name in ("span_id", "dur_us", "flags", "start_us"):
        assert not getattr(ex, name)[unused].any(), name


@pytest.fixture(scope="module")
def sn_set():
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)
    sp.start_us = (1_762_000_000_000_000 + np.arange(sp.n_spans, dtype=np.uint64) * np.uint64(37))
    return sp


@pytest.fixture(scope="module")
def sn_refs(sn_set):
    return [(k, which, exemplars_ref(sn_set, k, which)) for k in (1, 8, 64) for which in (0, 1)]


# 1
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_sn(ctx, sn_set, sn_refs, monkeypatch, capfd, geom):
    _geometry(monkeypatch, geom)
    edges = ctx.edge_aggregate(sn_set, with_hist=False)
    dev = resident(ctx, sn_set)
    both_forms(ctx, sn_set, sn_refs, capfd, monkeypatch, dev=dev)
    for k, which, ref in sn_refs:
        got = ctx.edge_exemplars(dev, k, errors_only=bool(which))
        total = edges.errors if which else edges.count
        np.testing.assert_array_equal(got.n_found, np.minimum(k, total).astype(np.uint32))
        if not which:
            full = edges.count > 0
            np.testing.assert_array_equal(got.dur_us[full, 0], edges.max_us[full])
        check_unused(got)
        assert got.start_us[got.position != U64].min() > 0
    # the placement the geometry asks for (E = 168: K <= 16 fits the LDS budget)
    capfd.readouterr()
    ctx.edge_exemplars(dev, 8)
    _logged(capfd, "rows", "global" if geom[1] == "0" else "lds")
    ctx.edge_exemplars(dev, 64)
    _logged(capfd, "rows", "global")
    # the device set with the row stream switched off: the keys form
    monkeypatch.setenv("ANOMOD_PARENT_ROWS", "0")
    for k, which, ref in sn_refs[2:4]:
        off = ctx.edge_exemplars(dev, k, errors_only=bool(which))
        _logged(capfd, "keys")
        assert_exemplars_equal(off, ref)
    monkeypatch.delenv("ANOMOD_PARENT_ROWS")
    dev.free()


# 2
@pytest.mark.parametrize("lds", [None, "0"])
def test_ties_across_workgroups(ctx, monkeypatch, capfd, lds):
    """6 000 spans of one duration on one edge, two durations on another, three
    workgroups: the exemplars are the smallest positions, whichever workgroup
    gets to the list first."""
    _geometry(monkeypatch, ("3", lds))
    sp = ties_set()
    ref = exemplars_ref(sp, 8)
    r0, r1 = ref.row("ROOT", "s0"), ref.row("ROOT", "s1")
    assert ref.position[r0].tolist() == [0, 1, 3, 4, 6, 7, 9, 10]
    assert ref.position[r1].tolist() == [5, 11, 17, 23, 29, 35, 41, 47]
    both_forms(ctx, sp, [(8, 0, ref), (1, 0, exemplars_ref(sp, 1))], capfd, monkeypatch)


# 3
@pytest.mark.parametrize("geom", [(None, None), ("3", None), ("3", "0")])
def test_order_extremes(ctx, monkeypatch, capfd, geom):
    _geometry(monkeypatch, geom)
    for name, sp in order_sets(8).items():
        ref = exemplars_brute(sp, 8)
        both_forms(ctx, sp, [(8, 0, ref)], capfd, monkeypatch)
        r = ref.row("ROOT", "s0")
        if name == "ascending":
            assert ref.position[r].tolist() == list(range(4999, 4991, -1))
        if name == "descending":
            assert ref.position[r].tolist() == list(range(8))
        if name == "extremes":
            assert (ref.dur_us[r] == U32).all() and ref.position[r, 0] == 3
            assert int((sp.dur_us == 0).sum()) > 0
        if name == "k_and_k_minus_1":
            assert ref.n_found[r] == 8 and ref.n_found[ref.row("ROOT", "s1")] == 7


# 4
def test_trainticket_width(ctx, monkeypatch, capfd):
    """E = 2208: at K = 16 the lists (282 KiB) stay in global memory behind the
    threshold cache, whatever the budget cap; at K = 2 they fit LDS."""
    sp = anomod.synth_generate_host(anomod.SynthSpec("TT", seed=11, p_orphan_ppm=5000), 300)
    assert edge_rows(sp.n_services) == 2208
    ref = exemplars_ref(sp, 16)
    err = exemplars_ref(sp, 16, 1)
    both_forms(ctx, sp, [(16, 0, ref), (16, 1, err)], capfd, monkeypatch, lists="global")
    monkeypatch.setenv("ANOMOD_EXEMPLARS_LDS", str(1 << 20))  # a cap: cannot force lds
    both_forms(ctx, sp, [(16, 0, ref)], capfd, monkeypatch)
    monkeypatch.setenv("ANOMOD_EXEMPLARS_LDS", "0")            # no threshold cache
    monkeypatch.setenv("ANOMOD_EXEMPLARS_WGS", "2")
    both_forms(ctx, sp, [(16, 0, ref), (16, 1, err)], capfd, monkeypatch, lists="global")
    monkeypatch.delenv("ANOMOD_EXEMPLARS_LDS")
    both_forms(ctx, sp, [(2, 0, exemplars_ref(sp, 2))], capfd, monkeypatch, lists="lds")
    monkeypatch.delenv("ANOMOD_EXEMPLARS_WGS")
    # rows written at one service count, read at another
    wide = anomod.SpanSet(sp.services + ["extra-1", "extra-2"], sp.trace_ptr, sp.trace_hash,
                          sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us,
                          unique_ids=sp.unique_ids)
    wref = exemplars_ref(wide, 16)
    dev = resident(ctx, sp)
    got = EdgeExemplars.empty(wide.services, 16)
    cs = got.c_struct()
    capfd.readouterr()
    assert L.lib().anomod_edge_exemplars_spans(ctx.handle, dev.handle, C.byref(cs)) == L.OK
    _logged(capfd, "rows", "global")
    assert_exemplars_equal(got, wref)
    dev.free()


# 5
@pytest.mark.parametrize("unique", [True, False])
def test_long_traces(ctx, unique, monkeypatch, capfd):
    """Traces of 16..600 spans: the keys form goes through the long-trace key pass."""
    sp = anomod.synth_generate_host(anomod.SynthSpec("LONG", seed=4, p_orphan_ppm=10000), 40)
    lens = np.diff(sp.trace_ptr)
    assert lens.max() > 256 and lens.min() >= 16
    sp.unique_ids = unique
    both_forms(ctx, sp, [(8, 0, exemplars_brute(sp, 8)), (3, 1, exemplars_ref(sp, 3, 1))],
               capfd, monkeypatch)


# 6
@pytest.mark.parametrize("geom", [(None, None), ("3", "0")])
def test_spans_outside_every_trace_are_never_exemplars(ctx, monkeypatch, capfd, geom):
    _geometry(monkeypatch, geom)
    sp = cut_set()
    ref = exemplars_brute(sp, 8)
    dev = resident(ctx, sp)
    both_forms(ctx, sp, [(8, 0, ref), (8, 1, exemplars_brute(sp, 8, 1))], capfd, monkeypatch,
               dev=dev)
    got = ctx.edge_exemplars(dev, 8)
    dev.free()
    used = got.position != U64
    pos, t = got.position[used], got.trace[used].astype(np.int64)
    assert pos.min() >= 3 and pos.max() < 4098 and got.dur_us.max() <= 1000
    assert (sp.trace_ptr[t] <= pos).all() and (pos < sp.trace_ptr[t + 1]).all()
    assert 1 not in t.tolist()  # the empty trace holds nothing


# 7
def _raw_call(ctx, dev, S, k, which):
    cs = L.EdgeExemplarsC(S, k, which, None, None, None, None, None, None, None)
    return L.lib().anomod_edge_exemplars_spans(ctx.handle, dev.handle, C.byref(cs))


def test_errors_and_empty_input(ctx, sn_set):
    S = sn_set.n_services
    small = sn_set.select_traces(np.arange(sn_set.n_traces) < 50)
    dev = ctx.upload(small)
    assert _raw_call(ctx, dev, S, 8, 0) == L.OK      # every output pointer NULL
    assert _raw_call(ctx, dev, S, 64, 1) == L.OK
    for k, which in ((0, 0), (65, 0), (8, 2)):
        assert _raw_call(ctx, dev, S, k, which) == L.EINVAL, (k, which)
    # E * K <= 2^24: S = 600 has 361 200 rows
    assert _raw_call(ctx, dev, 600, 46, 0) == L.OK
    assert _raw_call(ctx, dev, 600, 47, 0) == L.EINVAL
    assert b"2^24" in L.lib().anomod_last_error(ctx.handle)
    assert _raw_call(ctx, dev, int(small.svc.max()), 8, 0) == L.EINVAL
    assert b"service index" in L.lib().anomod_last_error(ctx.handle)
    assert _raw_call(ctx, dev, 0, 8, 0) == L.EINVAL and _raw_call(ctx, dev, 4097, 1, 0) == L.EINVAL
    for k in (0, 65):
        with pytest.raises(anomod.AnomodError) as e:
            ctx.edge_exemplars(dev, k)
        assert e.value.status == L.EINVAL
    ung = ctx.upload_ungrouped(small)
    assert _raw_call(ctx, ung, S, 8, 0) == L.EINVAL
    assert b"not grouped" in L.lib().anomod_last_error(ctx.handle)
    ung.free()
    # without a start column: start_us stays 0
    bare = small.select_traces(np.ones(small.n_traces, bool))
    bare.start_us = None
    got = ctx.edge_exemplars(bare, 4)
    assert not got.start_us.any()
    assert_exemplars_equal(got, exemplars_ref(bare, 4))
    dev.free()
    # an empty set: nothing found, every slot unused
    empty = small.select_traces(np.zeros(small.n_traces, bool))
    got = ctx.edge_exemplars(empty, 8, errors_only=True)
    assert_exemplars_equal(got, EdgeExemplars.empty(small.services, 8, 1))


def test_two_calls_and_the_shared_scratch(ctx, sn_set, sn_refs):
    dev = resident(ctx, sn_set)
    a = ctx.edge_exemplars(dev, 8)
    ctx.edge_exemplars(sn_set.select_traces(np.arange(sn_set.n_traces) % 7 == 0), 64)
    ctx.edge_windows(sn_set, 1_762_000_000_000_000, 1_000_000, 4)  # shares the scratch slot
    b = ctx.edge_exemplars(dev, 8)
    assert_exemplars_equal(a, b)
    assert_exemplars_equal(a, sn_refs[2][2])
    whole, kern = ctx.stage_ms(L.STAGE_EDGE_EXEMPLARS), ctx.stage_ms(L.STAGE_EDGE_EXEMPLARS_KERNEL)
    assert 0 < kern <= whole
    # rows and hints are left alone
    rows = np.zeros(dev.n_spans, np.uint16)
    hints = dev.hints
    fresh = ctx.upload(sn_set)
    ctx.edge_exemplars(fresh, 8)
    assert L.lib().anomod_spans_parent_rows(ctx.handle, fresh.handle, L.ptr(rows, C.c_uint16),
                                            len(fresh.services)) != L.OK
    assert dev.hints == hints
    fresh.free()
    dev.free()


def _golden_experiment(golden, tmp_path):
    exp_name = "Svc_Kill_Media_20251103_230000"
    d = tmp_path / "trace_data" / f"{exp_name}_traces_2025-11-03_23-10-00"
    d.mkdir(parents=True)
    shutil.copy(golden / "jaeger_small.json", d / "all_traces.json")
    return anomod.load_experiment(d, name=exp_name), d


def test_features_fill_both_tables_and_change_nothing_else(ctx, golden, tmp_path):
    exp, _ = _golden_experiment(golden, tmp_path)
    f0 = anomod.features(exp, ctx)
    f = anomod.features(exp, ctx, exemplars=4)
    assert f0.exemplars is None and f0.error_exemplars is None
    np.testing.assert_array_equal(f.service_scores, f0.service_scores)
    assert f.params["components"].keys() == f0.params["components"].keys()
    for name, v in f0.params["components"].items():
        np.testing.assert_array_equal(f.params["components"][name], v)
    for name in ("count", "errors", "sum_us", "max_us", "p99_us"):
        np.testing.assert_array_equal(getattr(f.edges, name), getattr(f0.edges, name))
    assert_exemplars_equal(f.exemplars, exemplars_brute(exp.spans, 4))
    assert_exemplars_equal(f.error_exemplars, exemplars_brute(exp.spans, 4, 1))
    assert f.exemplars.n_found.sum() > 0


def test_cli_prints_trace_ids_of_the_file(ctx, golden, tmp_path):
    from anomod.__main__ import main

    exp, d = _golden_experiment(golden, tmp_path)
    out = tmp_path / "features.json"
    assert main(["features", str(d), "--exemplars", "3", "--out", str(out)]) == 0
    doc = json.loads(out.read_text())
    file_ids = {t["traceID"] for t in json.loads((d / "all_traces.json").read_text())["data"]}
    by_id = {t["traceID"]: {s["spanID"].lower().zfill(16) for s in t["spans"]}
             for t in json.loads((d / "all_traces.json").read_text())["data"]}
    ex = doc["exemplars"]
    assert ex["k"] == 3 and list(ex["services"]) == [s for s, _ in doc["ranking"][:5]]
    f = anomod.features(exp, ctx, exemplars=3)
    n_calls = 0
    for name, entry in ex["services"].items():
        slow = entry["slow"]
        if slow is None:
            continue
        assert slow["child"] == name
        r = f.exemplars.row(slow["parent"], name)
        assert [c["dur_us"] for c in slow["calls"]] == f.exemplars.dur_us[r, : f.exemplars.n_found[r]].tolist()
        assert 1 <= len(slow["calls"]) <= 3
        for c in slow["calls"] + (entry["errors"]["calls"] if entry["errors"] else []):
            assert c["trace_id"] in file_ids, c
            assert c["span_id"] in by_id[c["trace_id"]], c
            n_calls += 1
        if entry["errors"]:
            assert all(c["error"] for c in entry["errors"]["calls"])
    assert n_calls > 0

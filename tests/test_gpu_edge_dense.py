"""Dense edge stream of a resident span set: the set learns from its own first
table which edges carry spans (codes) and which histogram bins each of them
touches (a cell range), streams its parent rows three more times as before,
writes a u16 code column on the aggregation after those (its fifth), and from
the next on reads codes and durations only
(edge_row_kernel<dense_hist,code_stats>).

Every table of every call — walk, rows x 3, transition, dense, dense — equals the CPU
oracle bit for bit, the E x 896 histogram included, the log says which kernel
ran, and the layout the library reports (codes, cells, LDS tier) equals a numpy
model built from the oracle's per-span edges."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import anomod
from anomod import _lib as L
from oracle import native, spec

from conftest import PKG_DIR, ROOT
from edge_exemplars_ref import assert_exemplars_equal, exemplars_ref
from edge_load_ref import assert_load_equal, edge_load_ref
from test_gpu_parent_rows import (_aggregate_abi, _offset_set, _random_spanset, assert_table_equal,
                                  get_rows, model_rows)

pytestmark = pytest.mark.gpu

WALK, STREAM = "edge_agg_kernel<", "edge_row_kernel<"
FILLS, CODES = "+ parent rows", "+ edge codes"
DENSE = "edge_row_kernel<dense_hist,code_stats>"
# the library's two LDS carves (codes, cells) and the spans of one workgroup round
SMALL, LARGE = (64, 8192), (512, 32768)
ROUND = {"small": 8192, "large": 16384}
NBINS = L.HIST_BINS
U32MAX = 2**32 - 1
WAIT = 3  # plain row streams between the call that learns a layout and the one that writes codes
_LAYOUT = re.compile(r"edge dense layout S=(\d+) codes=(\d+) cells=(\d+): (\w+)")


def _log(capfd):
    """(kernel lines, layout lines as (S, codes, cells, word)) since the last read."""
    err = capfd.readouterr().err.splitlines()
    lay = [(int(m[1]), int(m[2]), int(m[3]), m[4]) for m in map(_LAYOUT.search, err) if m]
    return [ln for ln in err if "edge aggregation kernel" in ln], lay


def with_dur(sp, dur):
    return anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id, sp.parent_span_id,
                          sp.svc, sp.flags, np.asarray(dur, np.uint32))


def _narrow(rng, S, n_traces, max_len, dmax, **kw):
    """(a random span set, durations below dmax for it): arguments of with_dur."""
    sp = _random_spanset(rng, S, n_traces, max_len, **kw)
    return sp, rng.integers(0, dmax, sp.n_spans)


def model_layout(sp, S=None, shrink=False):
    """(codes, cells, tier word) of the layout rule, from the oracle's per-span
    edges: a code per edge with spans, hist_bin(max) - hist_bin(min) + 1 cells
    each (two fewer, at least none, under ANOMOD_DENSE_SHRINK=1)."""
    S = len(sp.services) if S is None else S
    edges = np.asarray(native.span_edges(sp, S), np.int64)
    bins = spec.hist_bins_np(sp.dur_us).astype(np.int64)
    E = (S + 2) * S
    lo = np.full(E, NBINS, np.int64)
    hi = np.full(E, -1, np.int64)
    np.minimum.at(lo, edges, bins)
    np.maximum.at(hi, edges, bins)
    used = hi >= 0
    width = hi[used] - lo[used] + 1
    if shrink:
        width = np.maximum(width - 2, 0)
    codes, cells = int(used.sum()), int(width.sum())
    word = ("small" if codes <= SMALL[0] and cells <= SMALL[1] else
            "large" if codes <= LARGE[0] and cells <= LARGE[1] else "does")
    return codes, cells, word


def run_calls(ctx, dev, ref, capfd, calls=4 + WAIT, layout=None, S=None):
    """`calls` aggregations of a fresh resident set: every table == ref; the
    log names walk, WAIT row streams, transition, dense, dense for a set whose
    layout fits, and walk, rows, rows, ... for one whose layout does not."""
    capfd.readouterr()
    for _ in range(calls):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    names, lay = _log(capfd)
    assert len(names) == calls, names
    assert WALK in names[0] and FILLS in names[0], names
    assert len(lay) == 1, lay
    if layout is not None:
        assert lay[0] == (len(dev.services) if S is None else S,) + tuple(layout), (lay, layout)
    if lay[0][3] == "does":
        assert all(STREAM in n and CODES not in n and DENSE not in n for n in names[1:]), names
    else:
        assert all(STREAM in n and CODES not in n and DENSE not in n for n in names[1:1 + WAIT]), names
        t = names[1 + WAIT]
        assert STREAM in t and CODES in t and DENSE not in t, names
        assert all(DENSE in n for n in names[2 + WAIT:]) and len(names) >= 4 + WAIT, names
    return names, lay[0]


def _bin_dur(b):
    """A duration of histogram bin b."""
    return spec.hist_bounds(int(b))[0]


def star_set(S, groups, rng=None, fill=0, err=0.1):
    """One trace per group (a, root_dur, [(b, durs), ...]): a root span of
    service a and, for every (b, durs), one child of service b per duration,
    all referring to the root — edge (S, a) gets root_dur, edge (a, b) durs.
    `fill` > 0 adds that many more children per child edge with durations
    drawn between the edge's extremes (same bins range)."""
    rng = rng or np.random.default_rng(0)
    svc, dur, pid, sid, lens = [], [], [], [], []
    nid = 1
    for a, rd, kids in groups:
        root = nid
        nid += 1
        svc.append(a), dur.append(rd), pid.append(0), sid.append(root)
        n = 1
        for b, ds in kids:
            ds = list(ds)
            if fill:
                ds += rng.integers(min(ds), max(ds) + 1, fill).tolist()
            for d in ds:
                svc.append(b), dur.append(d), pid.append(root), sid.append(nid)
                nid += 1
                n += 1
        lens.append(n)
    ptr = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    sid = np.asarray(sid, np.uint64)
    flg = (rng.random(len(svc)) < err).astype(np.uint16)
    return anomod.SpanSet([f"svc{i:03d}" for i in range(S)], ptr, sid.copy(), sid,
                          np.asarray(pid, np.uint64), np.asarray(svc, np.uint16), flg,
                          np.asarray(dur, np.uint32))


def plan(S, codes, cells):
    """Groups for star_set with exactly `codes` edges with spans and `cells`
    dense cells: R root edges of one cell each, codes - R child edges whose
    bin ranges (from bin 0 up) add up to the rest."""
    R = -(-codes // (S + 1))
    kids = codes - R
    assert kids <= R * S and kids <= cells - R <= kids * NBINS
    left, groups, k = cells - R, [], 0
    for a in range(R):
        mine = []
        for b in range(S):
            if k == kids:
                break
            w = min(NBINS, left - (kids - k - 1))
            mine.append((b, [0, _bin_dur(w - 1)] if w > 1 else [0]))
            left -= w
            k += 1
        groups.append((a, 7, mine))
    assert left == 0 and k == kids
    return groups


def test_model_layout_on_a_hand_made_set():
    """The numpy layout model on three edges whose ranges are known by hand."""
    sp = star_set(3, [(0, 7, [(1, [0, 63, 64, 65]), (2, [U32MAX, U32MAX])])], err=0)
    # (3, 0): bin 7; (0, 1): bins 0..64 (64 and 65 share one) -> 65 cells; (0, 2): bin 895 alone
    assert spec.hist_bins_np(np.array([63, 64, 65, 66, U32MAX], np.uint32)).tolist() == [
        63, 64, 64, 65, 895]
    assert model_layout(sp) == (3, 67, "small")
    assert model_layout(sp, shrink=True) == (3, 63, "small")
    assert model_layout(star_set(12, plan(12, 11, 8193))) == (11, 8193, "large")


def test_bins(ctx, monkeypatch, capfd):
    """Durations 0, 63, 64, 65 and 2^32 - 1, an edge of one bin (min = max),
    an edge over all 896 bins, error bits, roots, orphans, self references,
    duplicated ids and empty traces."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(5)
    # services 4 and 5 for the hand-made edges, 0..3 for the random part
    a = star_set(6, [(4, 0, [(5, [0, 63, 64, 65, U32MAX]), (4, [1234] * 9)]),
                     (5, U32MAX, [(4, [63, 64]), (5, [65, 65, 64])]),
                     (4, 0, [])], rng, err=0.4)
    b = _random_spanset(rng, 4, 400, 12, orphan=0.1, dup=0.05, self_ref=0.05)
    b = anomod.SpanSet(a.services, b.trace_ptr, b.trace_hash, b.span_id, b.parent_span_id, b.svc,
                       b.flags, rng.choice(np.array([0, 63, 64, 65, 300, U32MAX], np.uint32), b.n_spans))
    assert (np.diff(b.trace_ptr.astype(np.int64)) == 0).any()
    sp = anomod.SpanSet.concat([a, b])
    assert sp.flags.any() and (sp.dur_us == U32MAX).any()
    ref = native.edge_aggregate(sp)
    assert (ref["count"] > 0).sum() > 8 and ((ref["min_us"] == ref["max_us"]) & (ref["count"] > 1)).any()
    assert ((ref["min_us"] == 0) & (ref["max_us"] == U32MAX)).any()
    dev = ctx.upload(sp)
    _, lay = run_calls(ctx, dev, ref, capfd, layout=model_layout(sp))
    assert lay[3] in ("small", "large")
    np.testing.assert_array_equal(get_rows(ctx, dev)[1], model_rows(sp, 6))
    dev.free()


@pytest.mark.parametrize("S,codes,cells,word", [
    (12, 11, SMALL[1], "small"), (12, 11, SMALL[1] + 1, "large"),
    (12, SMALL[0], 8000, "small"), (12, SMALL[0] + 1, 8000, "large"),
    (12, 50, LARGE[1], "large"), (12, 50, LARGE[1] + 1, "does"),
    (23, LARGE[0], 700, "large"), (23, LARGE[0] + 1, 700, "does")])
def test_capacity_borders(ctx, monkeypatch, capfd, S, codes, cells, word):
    """Cells exactly at a carve's capacity run in it and one more cell does
    not; 64 / 65 codes switch the carve; 512 edges with spans run dense and
    513 keep the hash form, which the log says."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = star_set(S, plan(S, codes, cells), np.random.default_rng(codes + cells), fill=3)
    assert model_layout(sp) == (codes, cells, word)
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    names, lay = run_calls(ctx, dev, ref, capfd, layout=(codes, cells, word))
    if word == "does":
        assert "lds_hist" in names[-1] or "lds_compact_hist" in names[-1], names
    dev.free()


@pytest.mark.parametrize("tier", ["small", "large"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("head", [0, 1, 2, 3])
def test_stream_borders(ctx, monkeypatch, capfd, tier, delta, head):
    """Ranges of one workgroup round - 1 / exact / + 1 spans starting at span
    position 0..3, with spans outside every trace before and after (they get
    no code): the 8-B and 16-B loads start at the first 4-aligned position."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    n_range = ROUND[tier] + delta
    S, dmax = (6, 500) if tier == "small" else (12, 1000)
    rng = np.random.default_rng(n_range * 4 + head)
    lens = []
    while sum(lens) < n_range:
        lens.append(int(min(rng.integers(0, 40), n_range - sum(lens))))
    core = _random_spanset(rng, S, 0, 0, lens=lens, dup=0.01)
    core = with_dur(core, rng.integers(0, dmax, core.n_spans))
    assert core.n_spans == n_range
    sp = _offset_set(core, head, 5, rng) if head else core
    ref = native.edge_aggregate(core)
    dev = ctx.upload(sp)
    _, lay = run_calls(ctx, dev, ref, capfd, layout=model_layout(core))
    assert lay[3] == tier
    np.testing.assert_array_equal(get_rows(ctx, dev)[1], model_rows(sp, S))
    dev.free()


@pytest.mark.parametrize("cap", [1000, 4096])
def test_launch_caps(ctx, monkeypatch, capfd, cap):
    """ANOMOD_MAX_LAUNCH_SPANS on a set with one 5000-span trace: the dense
    stream is cut by span count like the row stream; once more without."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(cap)
    sp = anomod.SpanSet.concat([_random_spanset(rng, 12, 1500, 12, dup=0.01),
                                _random_spanset(rng, 12, 0, 0, lens=[5000, 300]),
                                _random_spanset(rng, 12, 500, 3)])
    sp = with_dur(sp, rng.integers(0, 1000, sp.n_spans))
    assert int(np.diff(sp.trace_ptr.astype(np.int64)).max()) == 5000
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    monkeypatch.setenv("ANOMOD_MAX_LAUNCH_SPANS", str(cap))
    _, lay = run_calls(ctx, dev, ref, capfd, layout=model_layout(sp))
    assert lay[3] == "large"
    monkeypatch.delenv("ANOMOD_MAX_LAUNCH_SPANS")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert DENSE in _log(capfd)[0][0]
    dev.free()


@pytest.mark.parametrize("topo,traces,word", [("SN", 20000, "small"), ("LONG", 1 << 16, "large"),
                                              ("TT", 4096, "does")])
def test_generated_sets(ctx, monkeypatch, capfd, topo, traces, word):
    """Generated SN and LONG sets go dense after their transition call, in the small
    and the large carve; a generated TrainTicket set does not (whole-ms
    durations: sparse ranges).  Equal tables either way."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    dev = ctx.generate(anomod.SynthSpec(topo, seed=11, p_orphan_ppm=500), traces)
    host = dev.download()
    ref = native.edge_aggregate(host)
    _, lay = run_calls(ctx, dev, ref, capfd, layout=model_layout(host))
    assert lay[3] == word
    dev.free()


def test_shrunk_ranges_take_the_hbm_path(ctx, monkeypatch, capfd):
    """ANOMOD_DENSE_SHRINK=1 narrows every learned range by a bin at each end:
    the extremes of every edge count in HBM, edges of one or two bins keep no
    cell at all, and the tables still equal the oracle's."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_SHRINK", "1")
    rng = np.random.default_rng(8)
    sp = anomod.SpanSet.concat([
        star_set(6, [(0, 5, [(1, [9, 9, 9]), (2, [9, 10]), (3, [0, 63, 64, U32MAX])])], rng),
        with_dur(*_narrow(rng, 6, 3000, 20, 500, dup=0.01))])
    ref = native.edge_aggregate(sp)
    want = model_layout(sp, shrink=True)
    assert want[1] < model_layout(sp)[1]
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=want)
    dev.free()


def test_switch_and_overrides(ctx, monkeypatch, capfd):
    """ANOMOD_EDGE_DENSE=0: equal tables and never a dense line.  Switching it
    off on a set that already holds codes goes back to the row stream, and
    ANOMOD_UNIQUE_SCAN=0 on such a set runs the walk."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(21)
    sp = with_dur(*_narrow(rng, 12, 3000, 30, 1000, dup=0.01))
    ref = native.edge_aggregate(sp)
    monkeypatch.setenv("ANOMOD_EDGE_DENSE", "0")
    dev = ctx.upload(sp)
    capfd.readouterr()
    for _ in range(4):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    names, lay = _log(capfd)
    assert WALK in names[0] and all(STREAM in n for n in names[1:]) and len(names) == 4, names
    assert not any(DENSE in n or CODES in n for n in names) and lay == [], (names, lay)
    monkeypatch.delenv("ANOMOD_EDGE_DENSE")
    for _ in range(3 + WAIT):  # learn from a row stream, WAIT row streams, transition, dense
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    names, lay = _log(capfd)
    assert not any(CODES in n or DENSE in n for n in names[:1 + WAIT]), names
    assert CODES in names[1 + WAIT] and DENSE in names[2 + WAIT], names
    assert [x[1:] for x in lay] == [model_layout(sp)], lay
    monkeypatch.setenv("ANOMOD_EDGE_DENSE", "0")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    names, _ = _log(capfd)
    assert len(names) == 1 and STREAM in names[0] and DENSE not in names[0], names
    monkeypatch.delenv("ANOMOD_EDGE_DENSE")
    monkeypatch.setenv("ANOMOD_UNIQUE_SCAN", "0")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    names, _ = _log(capfd)
    assert len(names) == 1 and WALK in names[0] and FILLS not in names[0], names
    monkeypatch.delenv("ANOMOD_UNIQUE_SCAN")
    monkeypatch.setenv("ANOMOD_PARENT_ROWS", "0")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert WALK in _log(capfd)[0][0]
    monkeypatch.delenv("ANOMOD_PARENT_ROWS")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert DENSE in _log(capfd)[0][0]
    dev.free()


def test_another_service_count(ctx, monkeypatch, capfd):
    """S alternates 12, 15, 12, 15, 12, 12 at the C ABI: a layout belongs to
    the S it was learned under, so every change of S goes back to the row
    stream and learns again.  Staying at 12, then at 15, then at 12 again long
    enough reaches the transition and a dense call at each S.  Every
    table equals its reference and the parent rows still equal the row model."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(12)
    sp = with_dur(*_narrow(rng, 12, 2000, 30, 1000, dup=0.01))
    refs = {}
    for S in (12, 15):
        wide = anomod.SpanSet([f"svc{i:03d}" for i in range(S)], sp.trace_ptr, sp.trace_hash,
                              sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us)
        refs[S] = native.edge_aggregate(wide)
        want = model_layout(wide, S)
    dev = ctx.upload(sp)
    capfd.readouterr()
    seq = [12, 15, 12, 15, 12, 12] + [12] * (1 + WAIT) + [15] * (3 + WAIT) + [12] * (3 + WAIT)
    for S in seq:
        assert_table_equal(_aggregate_abi(ctx, dev, S), refs[S])
    names, lay = _log(capfd)
    assert len(names) == len(seq)
    kind = ["dense" if DENSE in n else "codes" if CODES in n else "walk" if WALK in n else "rows"
            for n in names]
    stay = ["rows"] * (1 + WAIT) + ["codes", "dense"]  # learn, wait, transition, dense
    assert kind == ["walk", "rows", "rows", "rows"] + stay + stay + stay, kind
    # a layout per change of S, each with the codes and cells of the model
    assert [x[0] for x in lay] == [12, 15, 12, 15, 12, 15, 12], lay
    assert all(x[1:] == want for x in lay), (lay, want)
    for S in (12, 15):
        np.testing.assert_array_equal(get_rows(ctx, dev, S)[1], model_rows(sp, S))
    dev.free()


def test_other_readers_are_unchanged(ctx, monkeypatch, capfd):
    """edge_quantiles_exact, the exemplars and the edge load of a set in the
    dense state: the results of their references, and of the same set before
    it held codes — they read the parent rows, as before."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp = anomod.synth_generate_host(anomod.SynthSpec("SN", seed=7, p_orphan_ppm=20000), 2000)
    t0 = 1_762_000_000_000_000
    sp.start_us = np.uint64(t0) + np.arange(sp.n_spans, dtype=np.uint64) * np.uint64(37)
    q = (0, 50, 99)
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    before = (ctx.edge_quantiles_exact(dev, q), ctx.edge_exemplars(dev, 8),
              ctx.edge_load(dev, t0, 5000, 32))
    capfd.readouterr()
    for _ in range(3 + WAIT):
        assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert DENSE in _log(capfd)[0][-1]
    got, cnt = ctx.edge_quantiles_exact(dev, q)
    ex = ctx.edge_exemplars(dev, 8)
    ld = ctx.edge_load(dev, t0, 5000, 32)
    err = capfd.readouterr().err
    assert "edge_row_kernel<keys>" in err and "edge_exemplars_kernel<rows>" in err
    assert "edge_load_kernel<rows>" in err
    np.testing.assert_array_equal(got, native.exact_quantiles(sp, q))
    np.testing.assert_array_equal(got, before[0][0])
    np.testing.assert_array_equal(cnt, before[0][1])
    assert_exemplars_equal(ex, exemplars_ref(sp, 8, 0))
    assert_exemplars_equal(before[1], exemplars_ref(sp, 8, 0))
    want = edge_load_ref(sp, t0, 5000, 32)
    assert_load_equal(ld, want)
    assert_load_equal(before[2], want)
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert DENSE in _log(capfd)[0][0]
    dev.free()


_WORKER = textwrap.dedent("""
    import os, sys
    sys.path[:0] = [{pkg!r}, {root!r}]
    import numpy as np
    import anomod
    from anomod import dist
    info = dist.rank_from_env()
    grp = dist.HostGroup(info.rank, info.world)
    d = np.load(os.path.join({out!r}, f"part{{info.rank}}.npz"))
    part = anomod.SpanSet([f"svc{{i:03d}}" for i in range(int(d["S"]))], d["ptr"], d["sid"].copy(),
                          d["sid"], d["pid"], d["svc"], d["flg"], d["dur"])
    out = {{}}
    with anomod.Context(0) as c:
        dist.attach_host(c, grp)
        dev = c.upload(part)
        for k in range({calls}):
            t = c.edge_aggregate(dev)
            for f in ("count", "errors", "sum_us", "min_us", "max_us", "hist"):
                out[f"{{f}}{{k}}"] = getattr(t, f)
        dev.free()
    np.savez(os.path.join({out!r}, f"rank{{info.rank}}.npz"), **out)
    grp.barrier()
    grp.close()
""")


def test_two_ranks(tmp_path):
    """Two ranks on one device over the host transport, with different
    duration ranges per edge on each rank: a rank's layout comes from the
    reduced table, whose ranges cover both ranks' spans, and the tables of all
    calls of both ranks equal the oracle's table of the whole set."""
    rng = np.random.default_rng(77)
    parts = []
    for r in range(2):
        sp = _random_spanset(rng, 6, 1500, 20, dup=0.01)
        parts.append(with_dur(sp, rng.integers(0, 300, sp.n_spans) + (0 if r == 0 else 5000)))
        p = parts[-1]
        np.savez(tmp_path / f"part{r}.npz", S=6, ptr=p.trace_ptr, sid=p.span_id,
                 pid=p.parent_span_id, svc=p.svc, flg=p.flags, dur=p.dur_us)
    whole = anomod.SpanSet.concat(parts)
    ref = native.edge_aggregate(whole)
    # the reduced table's ranges span both ranks' durations and need the large carve; a
    # rank's own spans alone would fit the small one
    want = model_layout(whole)
    assert want[2] == "large" and all(model_layout(p)[2] == "small" for p in parts)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker.py"
    calls = 4 + WAIT
    script.write_text(_WORKER.format(pkg=str(PKG_DIR), root=str(ROOT), out=str(tmp_path),
                                     calls=calls))
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r),
                   WORLD_SIZE="2", LOCAL_RANK=str(r), ANOMOD_LOG_KERNEL="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      start_new_session=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100)[0].decode(errors="replace"))
        except subprocess.TimeoutExpired:
            for q in procs:
                if q.poll() is None:
                    os.killpg(q.pid, 9)
            pytest.fail("two-rank dense run timed out")
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    for r, text in enumerate(outs):
        names = [ln for ln in text.splitlines() if "edge aggregation kernel" in ln]
        lay = [m for m in map(_LAYOUT.search, text.splitlines()) if m]
        assert [(int(m[2]), int(m[3]), m[4]) for m in lay] == [want], text[-2000:]
        assert len(names) == calls and CODES in names[1 + WAIT], names
        assert all(DENSE in n for n in names[2 + WAIT:]), names
        got = np.load(tmp_path / f"rank{r}.npz")
        for k in range(calls):
            for f in ("count", "errors", "sum_us", "min_us", "max_us", "hist"):
                np.testing.assert_array_equal(got[f"{f}{k}"], ref[f], err_msg=f"rank {r} call {k} {f}")

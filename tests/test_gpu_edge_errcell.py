"""Error cells of the dense edge stream: a packed layout of the small carve
whose cells fit the cell array twice (2^cell_bits + cells <= 16384 entries) is
read by edge_dense_kernel<0, 3>, which counts the error spans of a cell in an
entry of their own, 2^cell_bits above the cell's, and reads the error count of
an edge off those entries when it flushes: the span path branches for a
possible extreme only.

Every case runs a resident set through walk, row streams, the transition call
and two dense calls, every table of every call equals the CPU oracle's bit
for bit (test_gpu_edge_packword.run: tables, kernel names, layout, format and
pack lines), and the `edge dense errcells` line equals a numpy model of the
rule, or is absent."""
import re

import numpy as np
import pytest

import anomod
from oracle import native

from test_gpu_edge_cellword import _bounds, _first_bin, _last_bin, with_flags
from test_gpu_edge_dense import model_layout, star_set
from test_gpu_edge_packword import border_core, model_pack, model_wide, plan_capped, run as pack_run
from test_gpu_parent_rows import _offset_set

pytestmark = pytest.mark.gpu

ENTRIES = 16384
_ERRC = re.compile(r"edge dense errcells S=(\d+) entries=(\d+)")


def model_errcells(sp, S=None):
    """None, or the entries the layout takes: packed, small carve, and the
    error entries 2^cell_bits above the cells' own still inside the array."""
    codes, cells, tier = model_layout(sp, S)
    pack = model_pack(sp, S)
    if pack is None or tier != "small" or 2**pack[0] + cells > ENTRIES:
        return None
    return 2**pack[0] + cells


def run(ctx, dev, ref, capfd, sp_model, want="model"):
    """pack_run, and the errcells lines: one with the entries of model_errcells
    (or `want`), or none."""
    want = model_errcells(sp_model) if want == "model" else want
    seen = pack_run(ctx, dev, ref, capfd, sp_model)
    got = [(int(m[1]), int(m[2])) for m in map(_ERRC.search, seen) if m]
    assert got == ([(len(sp_model.services), want)] if want else []), (got, want)
    return seen


def flagged_set(S, traces):
    """star_set with the flag of every span given: traces of (a, (root_dur,
    flag), [(b, [(dur, flag), ...]), ...])."""
    groups = [(a, rd, [(b, [d for d, _ in kids]) for b, kids in edges]) for a, (rd, _), edges in traces]
    flags = [f for _, (_, rf), edges in traces for f in [rf] + [f for _, kids in edges for _, f in kids]]
    return with_flags(star_set(S, groups, np.random.default_rng(0), err=0.0), flags)


# ---- 1. errors everywhere they matter ---------------------------------------------
def errors_core(share, seed=1):
    """Edges from service 0: to 1, the minimum is an error span; to 2, the
    maximum; to 3, both; to 4, only error spans; to 5, the errors all fall in
    one bin (duration 300 .. 303) that also holds plain spans.  Edges from
    service 1 carry errors at `share`."""
    rng = np.random.default_rng(seed)
    mid = [(int(d), 0) for d in rng.integers(20, 3000, 30)]
    special = (0, (9, 0), [
        (1, [(10, 1), (4000, 0)] + mid),
        (2, [(10, 0), (4000, 1)] + mid),
        (3, [(10, 1), (4000, 1)] + mid),
        (4, [(int(d), 1) for d in rng.integers(5, 5000, 25)]),
        (5, [(40, 0), (2500, 0)] + [(300 + k % 4, k % 2) for k in range(24)] + mid)])
    fill = [(1, (7, int(rng.random() < share)),
             [(b, [(int(d), int(rng.random() < share)) for d in rng.integers(0, 5000, 12)])
              for b in range(6)]) for _ in range(3)]
    return flagged_set(6, [special] + fill)


@pytest.mark.parametrize("share", [0.0, 0.5, 1.0])
def test_errors_where_they_matter(ctx, monkeypatch, capfd, share):
    """errors_core, a few hundred spans, 5 span positions before the first
    trace: error spans as the extremes of their edges, alone on an edge, and
    sharing one bin with plain spans."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    core = errors_core(share)
    assert 300 <= core.n_spans <= 600
    ref = native.edge_aggregate(core)
    S = 6
    cnt, err, mn, mx = ref["count"], ref["errors"], ref["min_us"], ref["max_us"]
    assert (mn[1], mx[1], mn[3], mx[3]) == (10, 4000, 10, 4000)
    assert cnt[4] == err[4] == 25 and err[5] == 12 and cnt[5] == 56
    fill_edges = np.arange(S, 2 * S)
    assert err[fill_edges].sum() == round(share * cnt[fill_edges].sum()) or 0 < share < 1
    assert model_errcells(core) is not None
    dev = ctx.upload(_offset_set(core, 5, 2, np.random.default_rng(2)))
    run(ctx, dev, ref, capfd, core)
    dev.free()


# ---- 2. the eligibility border ----------------------------------------------------
@pytest.mark.parametrize("cells,entries", [(8190, 16382), (8191, None), (8192, None)])
def test_rule_cells(ctx, monkeypatch, capfd, cells, entries):
    """64 codes in the small carve, bins up to exponent 4: 8 190 cells take 13
    cell bits and 16 382 entries; 8 191 and 8 192 cells take 14 cell bits, whose
    error entries would start at 16 384: they pack and keep the kernel without
    error cells."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(cells)
    sp = star_set(8, plan_capped(8, 64, cells, _last_bin(4) + 1), rng, fill=2, err=0.3)
    assert model_layout(sp) == (64, cells, "small")
    pack = model_pack(sp)
    assert pack is not None and pack[0] == (13 if cells == 8190 else 14), pack
    assert model_errcells(sp) == entries
    ref = native.edge_aggregate(sp)
    assert ref["errors"].sum() > 20
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp)
    dev.free()


def test_rule_five_cell_bits(ctx, monkeypatch, capfd):
    """4 codes, 20 cells: 5 cell bits, the entry index is error << 5 | cell."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(5)
    sp = star_set(6, plan_capped(6, 4, 20, 10), rng, fill=40, err=0.3)
    assert model_layout(sp) == (4, 20, "small") and model_pack(sp)[0] == 5
    assert model_errcells(sp) == 32 + 20
    ref = native.edge_aggregate(sp)
    assert 0 < ref["errors"].sum() < ref["count"].sum()
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp)
    dev.free()


# ---- 3. an escape word at every position of a load group ------------------------
def wide_core():
    """Traces of 8 spans, a root of service 0 and 7 children: 5 cell bits leave
    18 residual bits, the children of service 1 lie in the last bin of exponent
    18 and, one per marked trace, in the first bin of exponent 19 — a wide span,
    an escape word — at child position 1 .. 7, with and without the error flag;
    a trace of one span half way moves the later traces on by one position.
    Filler traces keep the wide spans under 1/256 of the set."""
    rng = np.random.default_rng(3)
    lo18, hi18 = _bounds(_last_bin(18))
    wide_d = _bounds(_first_bin(19))[0] + 12345

    def near():  # an ordinary child: three durations share a cell and a residual, some are errors
        return (int(rng.choice([lo18, lo18, hi18, lo18 + int(rng.integers(1, 2**18 - 1))])),
                int(rng.random() < 0.3))

    def marked(pos, err):
        kids = [near() for _ in range(7)]
        kids[pos - 1] = (wide_d, err)
        return (0, (7, 0), [(1, kids)])

    def filler():
        if rng.random() < 0.5:
            return (0, (7, int(rng.random() < 0.1)), [(1, [near() for _ in range(7)])])
        return (0, (7, 0), [(2, [(int(d), int(rng.random() < 0.2)) for d in rng.integers(0, 15, 7)])])

    traces = []
    for shift in (0, 1):
        for pos in range(1, 8):
            for err in (0, 1):
                traces += [marked(pos, err), filler()]
        if shift == 0:
            traces.append((0, (7, 1), []))
    traces.append((0, (7, 0), [(2, [(0, 0), (14, 1)])]))  # (the whole range of the filler edge)
    traces += [filler() for _ in range(900)]
    return flagged_set(4, traces), 28


@pytest.mark.parametrize("head", range(8))
def test_escape_at_every_group_position(ctx, monkeypatch, capfd, head):
    """wide_core behind 0 .. 7 span positions outside every trace: the 28 wide
    spans fall on every position of a group of 8, between neighbours that are
    ordinary spans."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    core, n_wide = wide_core()
    assert model_layout(core) == (3, 18, "small") and model_pack(core) == (5, 18)
    wide = model_wide(core, 18)
    assert wide == n_wide and wide * 256 <= core.n_spans, (wide, core.n_spans)
    at = np.flatnonzero(core.dur_us > _bounds(_last_bin(18))[1])
    assert len(at) == n_wide and set((at % 8).tolist()) == set(range(8))
    assert set(core.flags[at].tolist()) == {0, 1}
    ref = native.edge_aggregate(core)
    sp = _offset_set(core, head, 3, np.random.default_rng(head)) if head else core
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, core, want=32 + 18)
    dev.free()


# ---- 4. one cell, every lane ------------------------------------------------------
def test_one_cell_every_lane(ctx, monkeypatch, capfd):
    """One workgroup, one edge of 20 000 root spans of one duration, a quarter
    of them errors: every add of every lane goes to the two entries of one cell."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_WGS", "1")
    n = 20_000
    sid = np.random.default_rng(4).permutation(n).astype(np.uint64) + np.uint64(1)
    sp = anomod.SpanSet(["svc000", "svc001"], np.arange(n + 1, dtype=np.uint64), sid.copy(), sid,
                        np.zeros(n, np.uint64), np.ones(n, np.uint16),
                        (np.arange(n) % 4 == 0).astype(np.uint16), np.full(n, 1234, np.uint32))
    ref = native.edge_aggregate(sp)
    assert ref["count"][2 * 2 + 1] == n and ref["errors"][2 * 2 + 1] == n // 4
    assert model_layout(sp) == (1, 1, "small") and model_errcells(sp) == 4 + 1
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp)
    dev.free()


# ---- 5. the switch ---------------------------------------------------------------
def test_switch(ctx, monkeypatch, capfd):
    """ANOMOD_DENSE_ERRCELLS=0: the same lines but the errcells line, the same tables."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    core = errors_core(0.5)
    ref = native.edge_aggregate(core)
    monkeypatch.setenv("ANOMOD_DENSE_ERRCELLS", "0")
    dev = ctx.upload(core)
    run(ctx, dev, ref, capfd, core, want=None)
    dev.free()
    monkeypatch.delenv("ANOMOD_DENSE_ERRCELLS")
    dev = ctx.upload(core)
    run(ctx, dev, ref, capfd, core)
    dev.free()


# ---- 6. the large carve keeps its kernel -----------------------------------------
def test_large_carve_is_untouched(ctx, monkeypatch, capfd):
    """border_core("large"), 15 cell bits: packed, no error cells, equal tables."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    core, pr, _ = border_core("large")
    assert model_layout(core)[2] == "large" and model_pack(core) == (15, 8)
    assert model_errcells(core) is None
    ref = native.edge_aggregate(core)
    dev = ctx.upload(core)
    run(ctx, dev, ref, capfd, core)
    dev.free()

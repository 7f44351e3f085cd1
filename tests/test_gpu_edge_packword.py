"""Packed words of the dense edge stream: a layout that qualifies for cell
words and has at most 256 codes and 15 cell bits keeps its span-word column in
3 bytes per position — error |
cell | residual in 24 bits, the code implied by the cell, in a u16 and a u8
plane.  A span whose bin exponent exceeds the residual field (a wide span)
escapes like one outside its code's range; an escape word carries its code in
the residual field.

Every case runs a resident set through walk, row streams, the transition call
and at least two dense calls, every table of every call equals the CPU
oracle's bit for bit, the old format line equals test_gpu_edge_cellword's
model, and the `edge dense pack` lines equal a numpy model of the pack rule."""
import re

import numpy as np
import pytest

import anomod
from oracle import native, spec

import test_gpu_edge_dense as ted
from test_gpu_edge_cellword import (ROUND, _bounds, _edges, _exp, _first_bin, _last_bin, model_fmt,
                                    run as cell_run, sum_rounds, with_flags, without_svc0)
from test_gpu_edge_dense import WAIT, model_layout, star_set, with_dur
from test_gpu_parent_rows import _offset_set, _random_spanset, assert_table_equal

pytestmark = pytest.mark.gpu

U32MAX = 2**32 - 1
_PACK = re.compile(r"edge dense pack S=(\d+) bytes=3 cell_bits=(\d+) res_bits=(\d+)")
_DROP = re.compile(r"edge dense pack S=(\d+) dropped: (\d+) wide of (\d+) spans")
_BOUND = re.compile(r"edge dense sum bound: (\d+) spans per launch on (\d+) workgroups")


def model_pack(sp, S=None, shrink=False):
    """None, or (cell_bits, pr) of the layout's packed word: the pack rule from
    the layout and format models.  pr = min(max(res_bits, code_bits), 23 -
    cell_bits): the residual field also has to hold the code of an escape word."""
    codes, cells, tier = model_layout(sp, S, shrink)
    kind, code_bits, cell_bits, res_bits = model_fmt(sp, S, shrink)
    if kind != "cell" or codes > 256 or cell_bits > 15:
        return None
    return cell_bits, min(max(res_bits, code_bits), 23 - cell_bits)


def model_wide(sp, pr, S=None):
    """Wide spans of a set whose learned ranges are not cut: the spans of a bin
    exponent above pr (every span with an edge lies inside its edge's range)."""
    S = len(sp.services) if S is None else S
    ed = np.asarray(native.span_edges(sp, S), np.int64)
    return int(((_exp(spec.hist_bins_np(sp.dur_us)) > pr) & (ed >= 0)).sum())


def run(ctx, dev, ref, capfd, sp_model, shrink=False, calls=4 + WAIT, want_pack="model", want_drop=None):
    """test_gpu_edge_cellword.run (tables, kernel names, layout and format
    lines), and the pack lines: one `bytes=3` line equal to model_pack of
    sp_model, or none; a `dropped` line with want_drop = (wide, spans), or
    none.  Returns the stderr lines."""
    fmt, lay = model_fmt(sp_model, shrink=shrink), model_layout(sp_model, shrink=shrink)
    want = model_pack(sp_model, shrink=shrink) if want_pack == "model" else want_pack
    seen = cell_run(ctx, dev, ref, capfd, fmt, layout=lay, calls=calls)
    packs = [tuple(int(m[k]) for k in (2, 3)) for m in map(_PACK.search, seen) if m]
    assert packs == ([tuple(want)] if want else []), (packs, want)
    drops = [tuple(int(m[k]) for k in (2, 3)) for m in map(_DROP.search, seen) if m]
    assert drops == ([tuple(want_drop)] if want_drop else []), (drops, want_drop)
    return seen


def plan_capped(S, codes, cells, wmax):
    """ted.plan with ranges of at most wmax bins (from bin 0 up): groups for
    star_set with exactly `codes` edges with spans and `cells` cells, the
    widest bin at hist_bin wmax - 1."""
    R = -(-codes // (S + 1))
    kids = codes - R
    assert kids <= R * S and kids <= cells - R <= kids * wmax, (codes, cells, wmax)
    left, groups, k = cells - R, [], 0
    for a in range(R):
        mine = []
        for b in range(S):
            if k == kids:
                break
            w = min(wmax, left - (kids - k - 1))
            mine.append((b, [0, ted._bin_dur(w - 1)] if w > 1 else [0]))
            left -= w
            k += 1
        groups.append((a, 7, mine))
    assert left == 0 and k == kids
    return groups


# ---- 1. residual borders at pr ---------------------------------------------------
def border_core(tier, n_wide_extra=0, n_total=None):
    """A set whose layout packs with pr one below its largest exponent (small:
    13 cell bits, pr 10; large: 15 cell bits, pr 8).  32 border edges: for a
    bin of exponent pr and one of exponent pr + 1, the durations lo, lo + 2^pr
    - 1, lo + 2^pr and hi, each as the minimum of one edge and the maximum of
    another, with and without the error flag.  Filler edges over the bins up to
    exponent pr bring the cells to the width wanted and the wide spans under
    1/256 of the set; n_wide_extra more wide spans and padding to n_total spans
    for the share tests."""
    S, pr, fillers, fill = (7, 10, 9, 740) if tier == "small" else (12, 8, 62, 110)
    rng = np.random.default_rng(pr)
    top = _bounds(_last_bin(pr))[1]            # the largest duration that is not wide
    cases = []
    for e in (pr, pr + 1):
        lo, hi = _bounds(_first_bin(e) + 9)
        for d in (lo, lo + 2**pr - 1, lo + 2**pr, hi):
            for err in (0, 1):
                near_lo = _bounds(_first_bin(pr - 1))[0]
                near_hi = max(_bounds(_first_bin(pr) + 20)[1], d)
                cases.append(([d, near_hi if near_hi > d else d + 1], [err, 0]))   # d is the minimum
                cases.append(([near_lo, d], [0, err]))                             # d is the maximum
    assert len(cases) == 32
    pairs = [(a, b) for a in range(S) for b in range(S)]
    groups, flags = [], []
    by_a = {}
    for (a, b), (ds, fl) in zip(pairs, cases):
        by_a.setdefault(a, []).append((b, ds, fl))
    extra = [_bounds(_first_bin(pr + 1) + 3)[0] + 17] * n_wide_extra
    rest = pairs[len(cases):len(cases) + fillers]
    assert len(rest) == fillers
    for k, (a, b) in enumerate(rest):
        ds = [0, top] + rng.integers(0, top + 1, fill).tolist()
        if k == 0:
            ds += extra
        by_a.setdefault(a, []).append((b, ds, (rng.random(len(ds)) < 0.2).astype(int).tolist()))
    for a in sorted(by_a):
        groups.append((a, 50 + a, [(b, ds) for b, ds, _ in by_a[a]]))
        flags += [0] + [f for _, _, fl in by_a[a] for f in fl]
    core = with_flags(star_set(S, groups, rng, err=0.0), flags)
    if n_total is not None:  # pad with root spans of one trace each, not wide
        pad = n_total - core.n_spans
        assert pad >= 0, (core.n_spans, n_total)
        more = star_set(S, [(0, 50, [])] * pad, rng, err=0.0)
        core = anomod.SpanSet.concat([core, more]) if pad else core
    return core, pr, cases


@pytest.mark.parametrize("tier", ["small", "large"])
def test_residual_borders_at_pr(ctx, monkeypatch, capfd, tier):
    """border_core in both carves, 3 span positions before the first trace:
    wide spans inside their ranges at both extremes of their edges, and the
    largest residuals that still fit."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    core, pr, cases = border_core(tier)
    lay, fmt, pack = model_layout(core), model_fmt(core), model_pack(core)
    assert lay[2] == tier and fmt[0] == "cell" and fmt[3] == pr + 1, (lay, fmt)
    assert pack == ((13, 10) if tier == "small" else (15, 8)) and pack[1] == pr, pack
    wide = model_wide(core, pr)
    assert 24 <= wide and wide * 256 <= core.n_spans, (wide, core.n_spans)
    ref = native.edge_aggregate(core)
    # every border duration is an extreme of an edge, half of them with the error flag
    mins, maxs = set(ref["min_us"][ref["count"] > 0].tolist()), set(ref["max_us"][ref["count"] > 0].tolist())
    for ds, _ in cases:
        assert ds[0] in mins and ds[1] in maxs, ds
    sp = _offset_set(core, 3, 5, np.random.default_rng(1))
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, core)
    dev.free()


# ---- 2. alignment ------------------------------------------------------------------
def narrow_core(rng, n_traces=150):
    sp = without_svc0(_random_spanset(rng, 6, n_traces, 40, dup=0.01), 5)
    return with_dur(sp, rng.integers(0, 5000, sp.n_spans))


@pytest.mark.parametrize("head", range(10))
def test_alignment(ctx, monkeypatch, capfd, head):
    """0 .. 9 span positions before the first trace and 0 .. 9 after the last
    (every count once over the cases): the groups of 8 start at the first
    8-aligned position, up to 7 positions before and after are read singly."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    tail = (7 * head + 3) % 10
    rng = np.random.default_rng(20 + head)
    core = narrow_core(rng)
    assert model_pack(core) is not None
    ref = native.edge_aggregate(core)
    sp = _offset_set(core, head, tail, rng) if head + tail else core
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, core)
    dev.free()


@pytest.mark.parametrize("n", [1, 7, 8, 9])
@pytest.mark.parametrize("head", [0, 3])
def test_tiny_sets(ctx, monkeypatch, capfd, n, head):
    """Sets of 1, 7, 8 and 9 spans, at position 0 and at position 3: no group
    of 8, exactly one, one and a single position."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(100 * n + head)
    core = star_set(6, [(1, 900, [(2, rng.integers(70, 3000, n - 1).tolist())] if n > 1 else [])], rng,
                    err=0.4)
    assert core.n_spans == n and model_pack(core) is not None
    ref = native.edge_aggregate(core)
    sp = _offset_set(core, head, 2, rng) if head else core
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, core)
    dev.free()


# ---- 3. launch cuts ----------------------------------------------------------------
@pytest.mark.parametrize("cap", [1000, 1001, 4099])
def test_launch_cuts(ctx, monkeypatch, capfd, cap):
    """ANOMOD_MAX_LAUNCH_SPANS = 1000, 1001 and 4099 over about 6 000 spans, as
    in test_gpu_edge_cellword.test_launch_cuts: launches that start and end at
    any position of a group of 8, an edge whose spans all lie in the first
    launch, and one with its minimum before the first cut and its maximum after
    the last."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(cap)
    first = star_set(6, [(0, 40, [(1, [5, 77, 300, 4000] * 5), (2, [3, 500])])], rng, err=0.3)
    last = star_set(6, [(0, 41, [(2, [400, 4999])])], rng, err=0.3)
    mid = without_svc0(_random_spanset(rng, 6, 600, 20, dup=0.01), 3)
    mid = with_dur(mid, rng.integers(0, 5000, mid.n_spans))
    sp = anomod.SpanSet.concat([first, mid, last])
    assert sp.n_spans > 4099 + 1001
    ed = _edges(sp)
    assert np.flatnonzero(ed == 1).max() < 100
    ref = native.edge_aggregate(sp)
    assert ref["min_us"][2] == 3 and ref["max_us"][2] == 4999
    assert model_pack(sp) is not None
    dev = ctx.upload(sp)
    monkeypatch.setenv("ANOMOD_MAX_LAUNCH_SPANS", str(cap))
    run(ctx, dev, ref, capfd, sp)
    monkeypatch.delenv("ANOMOD_MAX_LAUNCH_SPANS")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    dev.free()


# ---- 4. out-of-range escapes carry their code -------------------------------------
def test_escapes_carry_their_code(ctx, monkeypatch, capfd):
    """ANOMOD_DENSE_SHRINK=1 over 256 codes: the extremes of every edge lie
    outside its cut range and escape with the code in the residual field —
    code 0 (edge (0, 0)), codes in between, and code 255, a root edge whose
    one-bin range keeps no cell at all.  Some carry the error flag."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_SHRINK", "1")
    rng = np.random.default_rng(44)
    S = 16
    groups = [(a, 7 + a, [(b, [100 + b, 130 + a, 200 + b]) for b in range(S)]) for a in range(15)]
    groups.append((15, 22, []))
    sp = star_set(S, groups, rng, fill=3, err=0.3)
    lay = model_layout(sp, shrink=True)
    assert lay[0] == 256 and lay[2] == "large", lay
    ref = native.edge_aggregate(sp)
    used = np.flatnonzero(ref["count"])
    assert used[0] == 0 and used[255] == S * S + 15 and ref["count"][used[255]] == 1
    assert ref["errors"][used[[0, 100, 200]]].sum() > 0
    pack = model_pack(sp, shrink=True)
    assert pack is not None and pack[1] >= 8, pack
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp, shrink=True)
    dev.free()


# ---- 5. rule borders ---------------------------------------------------------------
@pytest.mark.parametrize("codes,packs", [(256, True), (257, False)])
def test_rule_codes(ctx, monkeypatch, capfd, codes, packs):
    """256 codes pack, 257 keep 4-byte cell words; the format line is the cell
    format's either way."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(codes)
    S = 16
    groups = [(a, 7 + a, [(b, [100 + b, 130 + a, 200 + b]) for b in range(S)]) for a in range(15)]
    groups.append((15, 22, [(0, [150, 151])] if codes == 257 else []))
    sp = star_set(S, groups, rng, fill=3, err=0.3)
    assert model_layout(sp)[0] == codes and model_fmt(sp)[0] == "cell"
    assert (model_pack(sp) is not None) == packs
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp)
    dev.free()


@pytest.mark.parametrize("cells,packs", [(16382, True), (16383, True), (32766, True), (32767, False)])
def test_rule_cells(ctx, monkeypatch, capfd, cells, packs):
    """Cells at the borders of the cell field, 120 codes, bins up to exponent
    8: 16 382 cells take 14 cell bits, 16 383 and 32 766 take 15 and pack with
    the 8 residual bits that leaves; 32 767 take 16 and keep 4-byte cell words."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(cells)
    wmax = _last_bin(8) + 1
    sp = star_set(12, plan_capped(12, 120, cells, wmax), rng, fill=2)
    lay, fmt = model_layout(sp), model_fmt(sp)
    assert lay == (120, cells, "large") and fmt[0] == "cell" and fmt[3] == 8, (lay, fmt)
    assert fmt[2] == (14 if cells == 16382 else 16 if cells == 32767 else 15), fmt
    assert fmt[1] == 7 and fmt[1] + 1 + fmt[2] + fmt[3] <= 32  # (cell words at every width here)
    pack = model_pack(sp)
    assert (pack is not None) == packs and (not packs or pack == (fmt[2], 8)), pack
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp)
    dev.free()


def test_duration_word_layouts_are_untouched(ctx, monkeypatch, capfd):
    """An edge over all 896 bins: duration words, no pack line."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(7)
    sp = _random_spanset(rng, 6, 250, 20, dup=0.01)
    sp = with_dur(sp, rng.integers(0, 3000, sp.n_spans))
    sp = anomod.SpanSet.concat([sp, star_set(6, [(1, 9, [(2, [0, U32MAX, 77])])], rng), sp])
    assert model_fmt(sp) == ("dur", 10, 0, 21) and model_pack(sp) is None
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, sp)
    dev.free()


# ---- 6. wide share -------------------------------------------------------------------
@pytest.mark.parametrize("over", [False, True])
def test_wide_share(ctx, monkeypatch, capfd, over):
    """border_core padded to 7 680 spans = 30 x 256.  With 30 wide spans the set
    stays packed; with 31 the transition call logs that it dropped the packed
    form and writes the column again as 4-byte cell words, which the dense
    calls after it read.  Every table is exact, and the kernel names of the
    calls are the same in both."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    n = 7680
    base, pr, _ = border_core("small")
    w0 = model_wide(base, pr)
    core, pr, _ = border_core("small", n_wide_extra=30 + int(over) - w0, n_total=n)
    wide = model_wide(core, pr)
    assert core.n_spans == n and wide == 30 + int(over) and (wide * 256 > n) == over
    pack = model_pack(core)
    assert pack == (13, 10)
    ref = native.edge_aggregate(core)
    dev = ctx.upload(core)
    run(ctx, dev, ref, capfd, core, want_drop=(wide, n) if over else None)
    dev.free()


# ---- 7. sum bound --------------------------------------------------------------------
def test_sum_bound_runs_packed(ctx, monkeypatch, capfd):
    """test_gpu_edge_cellword.test_sum_bound_cuts_the_launch, packed: 1 + 2 +
    15 bits.  The same cut of 256 rounds is logged and the sum is exact."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_WGS", "1")
    n = 4_500_000
    d = _bounds(_first_bin(15) + 1)[1]
    assert n > 32 * (2**32 // (2**15 - 1)) and sum_rounds("small", 15) == 256
    rng = np.random.default_rng(6)
    sid = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    sp = anomod.SpanSet(["svc000", "svc001"], np.arange(n + 1, dtype=np.uint64), sid.copy(), sid,
                        np.zeros(n, np.uint64), np.ones(n, np.uint16),
                        (np.arange(n) % 5 == 0).astype(np.uint16), np.full(n, d, np.uint32))
    ref = native.edge_aggregate(sp)
    assert ref["sum_us"][2 * 2 + 1] == n * d > 2**42
    assert model_fmt(sp) == ("cell", 0, 2, 15) and model_pack(sp) == (2, 15)
    dev = ctx.upload(sp)
    seen = run(ctx, dev, ref, capfd, sp)
    cuts = [(int(m[1]), int(m[2])) for m in map(_BOUND.search, seen) if m]
    assert cuts == [(256 * ROUND["small"], 1)] * 2, cuts
    dev.free()


def test_count_bound_cuts_the_launch(ctx, monkeypatch, capfd):
    """One workgroup (ANOMOD_DENSE_WGS=1), one edge of 9 M root spans of duration
    5: one cell takes every span.  A cell of the packed kernel counts in 23
    bits below its flag and code, 8 388 607 at most, so the host gives a launch
    at most 511 rounds of 16 384 spans; count, histogram and errors are exact
    (residuals of exponent 0: no sum bound here)."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_WGS", "1")
    n = 9_000_000
    assert n > 2**23 > 511 * ROUND["small"]
    rng = np.random.default_rng(9)
    sid = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    sp = anomod.SpanSet(["svc000", "svc001"], np.arange(n + 1, dtype=np.uint64), sid.copy(), sid,
                        np.zeros(n, np.uint64), np.ones(n, np.uint16),
                        (np.arange(n) % 5 == 0).astype(np.uint16), np.full(n, 5, np.uint32))
    ref = native.edge_aggregate(sp)
    assert ref["count"][2 * 2 + 1] == n and ref["hist"][2 * 2 + 1, 5] == n
    assert model_fmt(sp) == ("cell", 0, 2, 0) and model_pack(sp) == (2, 0)
    dev = ctx.upload(sp)
    seen = run(ctx, dev, ref, capfd, sp)
    assert not any(_BOUND.search(ln) for ln in seen), seen
    dev.free()


# ---- 8. the switch -------------------------------------------------------------------
def test_switch(ctx, monkeypatch, capfd):
    """ANOMOD_DENSE_PACK=0: the layout keeps 4-byte cell words — the same
    kernel names, layout and format lines, no pack line, the same tables."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    core, pr, _ = border_core("small")
    assert model_pack(core) is not None
    ref = native.edge_aggregate(core)
    monkeypatch.setenv("ANOMOD_DENSE_PACK", "0")
    dev = ctx.upload(core)
    run(ctx, dev, ref, capfd, core, want_pack=None)
    dev.free()
    monkeypatch.delenv("ANOMOD_DENSE_PACK")
    dev = ctx.upload(core)
    run(ctx, dev, ref, capfd, core)
    dev.free()

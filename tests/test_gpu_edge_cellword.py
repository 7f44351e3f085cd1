"""Cell words of the dense edge stream: for a layout whose fields fit 32 bits
the set's span-word column holds code | error | cell | residual, bin and range
check resolved when the column is written, and the dense kernel adds to the
cell, adds the residual to a u32 sum replica and keeps min and max as keys.
Spans that do not fit their code's range (or the residual width) carry the
escape value and are read from dur_us; layouts that do not fit keep duration
words.

Every case runs a resident set through walk, row streams, the transition call
and at least two dense calls (run_calls checks the log), every table of every
call equals the CPU oracle's bit for bit, and the format line of the log
(`edge dense words ... format=cell|dur`) equals a numpy model of the rule."""
import re

import numpy as np
import pytest

import anomod
from oracle import native, spec

import test_gpu_edge_dense as ted
from test_gpu_edge_dense import (CODES, DENSE, LARGE, SMALL, WAIT, WALK, model_layout, run_calls,
                                 star_set, with_dur)
from test_gpu_parent_rows import _aggregate_abi, _offset_set, _random_spanset, assert_table_equal

pytestmark = pytest.mark.gpu

U32MAX = 2**32 - 1
NBINS = ted.NBINS
_WORDS = re.compile(r"edge dense words S=(\d+) format=(\w+) code_bits=(\d+) cell_bits=(\d+) res_bits=(\d+)")
_BOUND = re.compile(r"edge dense sum bound: (\d+) spans per launch on (\d+) workgroups")
# spans of one workgroup round (1024 threads x 4 spans x kLoad groups) and sum replicas
ROUND = {"small": 1024 * 4 * 4, "large": 1024 * 4 * 8}
REPS = {"small": 32, "large": 8}


def _exp(b):
    """Exponent of histogram bin b: the bin spans 2^e durations."""
    b = np.asarray(b, np.int64)
    return np.where(b < 64, 0, (b >> 5) - 1)


def _bounds(b):
    return spec.hist_bounds(int(b))


def _first_bin(e):
    return 0 if e == 0 else (e + 1) << 5


def _last_bin(e):
    return 63 if e == 0 else ((e + 1) << 5) + 31


def _bits(n):
    return max(0, int(n - 1).bit_length())


def sum_rounds(tier, res_bits):
    """Rounds a workgroup may run in one launch: a replica takes ROUND / REPS
    residuals below 2^res_bits per round and one head or tail span."""
    top = 2**res_bits - 1
    return 2**40 if top == 0 else (U32MAX // top - 1) // (ROUND[tier] // REPS[tier])


def model_fmt(sp, S=None, shrink=False):
    """('cell', code_bits, cell_bits, res_bits) or ('dur', 10, 0, 21): the rule
    of dense_learn from the oracle's per-span edges."""
    S = len(sp.services) if S is None else S
    edges = np.asarray(native.span_edges(sp, S), np.int64)
    bins = spec.hist_bins_np(sp.dur_us).astype(np.int64)
    E = (S + 2) * S
    lo = np.full(E, NBINS, np.int64)
    hi = np.full(E, -1, np.int64)
    np.minimum.at(lo, edges, bins)
    np.maximum.at(hi, edges, bins)
    used = hi >= 0
    b0, width = lo[used], hi[used] - lo[used] + 1
    if shrink:
        b0, width = b0 + 1, np.maximum(width - 2, 0)
    codes, cells = int(used.sum()), int(width.sum())
    last = (b0 + width - 1)[width > 0]
    res_bits = int(_exp(last).max()) if last.size else 0
    code_bits, cell_bits = _bits(codes), _bits(cells + 2)
    tier = "small" if codes <= SMALL[0] and cells <= SMALL[1] else "large"
    fits = (code_bits + 1 + cell_bits + res_bits <= 32 and cell_bits + res_bits < 31
            and sum_rounds(tier, res_bits) >= 1)
    return ("cell", code_bits, cell_bits, res_bits) if fits else ("dur", 10, 0, 21)


def run(ctx, dev, ref, capfd, want, layout=None, S=None, calls=4 + WAIT):
    """run_calls, and the format lines the calls logged: one, equal to `want`
    (a model_fmt tuple).  Returns every stderr line of the calls."""
    seen = []

    def log(capfd):
        err = capfd.readouterr().err.splitlines()
        seen.extend(err)
        lay = [(int(m[1]), int(m[2]), int(m[3]), m[4]) for m in map(ted._LAYOUT.search, err) if m]
        return [ln for ln in err if "edge aggregation kernel" in ln], lay

    orig, ted._log = ted._log, log  # (run_calls reads the log through its module's _log)
    try:
        _, lay = run_calls(ctx, dev, ref, capfd, calls=calls, layout=layout, S=S)
    finally:
        ted._log = orig
    assert lay[3] in ("small", "large"), lay
    words = [(m[2],) + tuple(int(m[k]) for k in (3, 4, 5)) for m in map(_WORDS.search, seen) if m]
    assert words == [tuple(want)], (words, want)
    return seen


def with_flags(sp, flags):
    return anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id, sp.parent_span_id,
                          sp.svc, np.asarray(flags, np.uint16), sp.dur_us)


def without_svc0(sp, to):
    """sp with service 0 renamed to `to`: no span of it lies on an edge from or to service 0."""
    svc = sp.svc.copy()
    svc[svc == 0] = to
    return anomod.SpanSet(sp.services, sp.trace_ptr, sp.trace_hash, sp.span_id, sp.parent_span_id,
                          svc, sp.flags, sp.dur_us)


def _edges(sp, S=None):
    return np.asarray(native.span_edges(sp, len(sp.services) if S is None else S), np.int64)


# ---- 1. residual borders ------------------------------------------------------
def border_set(tier, head, R=11):
    """(set with `head` spans before its first trace and 5 after, the core it
    wraps): a random part whose durations all lie inside one bin of exponent R,
    so that the min and max of its edges differ in the residual only, with the
    bin's lo and hi, lo + 1 and hi - 1 at the first position, the last singly
    read head position, the first tail position and the last position; and one
    star edge per exponent e in {0, 1, R - 1, R} with lo and hi of the
    exponent's first and last bin."""
    S = 6 if tier == "small" else 12
    rng = np.random.default_rng(1000 * head + S)
    b = _first_bin(R) + 9
    lo, hi = _bounds(b)
    kids = []
    for k, e in enumerate((0, 1, R - 1, R)):
        ds = [x for bb in (_first_bin(e), _last_bin(e)) for x in _bounds(bb)]
        kids.append((k + 1, ds + ds[:2]))
    star = star_set(S, [(0, hi, kids)], rng, err=0.2)
    n = 2500 if tier == "small" else 5000
    # (the parts around the star, on edges of their own: the first and last positions are theirs)
    rnd = without_svc0(_random_spanset(rng, S, n // 20, 20, dup=0.01), S - 1)
    a = with_dur(rnd, rng.integers(lo + 100, hi - 100, rnd.n_spans))
    rnd2 = without_svc0(_random_spanset(rng, S, n // 20, 20, dup=0.01), S - 1)
    c = with_dur(rnd2, rng.integers(lo + 100, hi - 100, rnd2.n_spans))
    core = anomod.SpanSet.concat([a, star, c])
    n = core.n_spans
    p0, p1 = head, head + n
    a0, a1 = (p0 + 3) & ~3, p1 & ~3
    dur = core.dur_us.copy()
    at = {0: lo, n - 1: hi}
    if a0 - p0 - 1 > 0:
        at[a0 - p0 - 1] = lo + 1
    if a1 < p1 and a1 - p0 < n - 1:
        at[a1 - p0] = hi - 1
    for i, d in at.items():
        dur[i] = d
    core = with_dur(core, dur)
    return _offset_set(core, head, 5, rng), core, at


@pytest.mark.parametrize("tier", ["small", "large"])
@pytest.mark.parametrize("head", [1, 2, 3, 5])
def test_residual_borders(ctx, monkeypatch, capfd, tier, head):
    """border_set in both carves, its traces starting at span position 1, 2, 3
    and 5: extremes that differ only in the residual, at the positions the
    kernel reads singly and at both ends of the 16-B groups."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    sp, core, at = border_set(tier, head)
    lay, fmt = model_layout(core), model_fmt(core)
    assert lay[2] == tier and fmt[0] == "cell" and fmt[3] == 11, (lay, fmt)
    ref = native.edge_aggregate(core)
    ed = _edges(core)
    n = core.n_spans
    assert ref["min_us"][ed[0]] == core.dur_us[0] and ref["max_us"][ed[n - 1]] == core.dur_us[n - 1]
    # edges of the random part: min and max in one bin, apart in the residual
    one_bin = (ref["count"] > 1) & (spec.hist_bins_np(ref["min_us"]) == spec.hist_bins_np(ref["max_us"]))
    assert (one_bin & (ref["min_us"] < ref["max_us"])).sum() > 10
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, fmt, layout=lay)
    dev.free()


# ---- 2. escapes ---------------------------------------------------------------
def test_escapes_by_exponent_and_range(ctx, monkeypatch, capfd):
    """ANOMOD_DENSE_SHRINK=1 cuts the first and the last bin of every learned
    range.  Three edges have their maximum alone in bins of exponent 8 while
    everything else stays at exponent <= 7: the cut ranges end at exponent 7,
    res_bits is 7, and those maxima escape by range and by exponent alike.  The
    extremes of every edge escape (HBM min / max) while the spans between them
    stay in LDS (keys), edges of one or two bins keep no cell, and both merge
    into the oracle's tables.  (The switch cuts both ends, so an edge with only
    one escaping extreme cannot be made through it.)"""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_SHRINK", "1")
    rng = np.random.default_rng(2)
    top7 = _bounds(_last_bin(7))[1]
    e8 = _bounds(_first_bin(8))[0]
    bg = _random_spanset(rng, 6, 250, 20, dup=0.01)
    bg = with_dur(bg, rng.integers(40, top7 + 1, bg.n_spans))
    star = star_set(6, [(0, 5, [(1, [9, 9, 9]), (2, [9, 10]), (3, [70, 3000, e8 + 5]),
                                (4, [100, 200, 300, e8, e8 + 77]), (5, [top7, top7 - 1, 64, e8 + 255])])],
                    rng, err=0.3)
    sp = anomod.SpanSet.concat([bg, star, bg])
    lay, fmt = model_layout(sp, shrink=True), model_fmt(sp, shrink=True)
    assert fmt[0] == "cell" and fmt[3] == 7 and model_fmt(sp)[3] == 8, fmt
    ref = native.edge_aggregate(sp)
    assert ref["max_us"][0 * 6 + 3] == e8 + 5 and ref["max_us"][0 * 6 + 5] == e8 + 255
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, fmt, layout=lay)
    dev.free()


# ---- 3. error bit in the key --------------------------------------------------
@pytest.mark.parametrize("rate", [0.0, 0.3, 1.0])
def test_error_bit_in_the_key(ctx, monkeypatch, capfd, rate):
    """Error rates 0, 0.3 and 1.0 over a random set; on top, an edge whose
    minimum carries the error flag, one whose maximum does, one whose every
    extreme does and one whose only span carries it."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(int(rate * 10) + 3)
    bg = without_svc0(_random_spanset(rng, 6, 250, 20, dup=0.01), 5)
    bg = with_dur(bg, rng.integers(0, 5000, bg.n_spans))
    bg = with_flags(bg, rng.random(bg.n_spans) < rate)
    star = star_set(6, [(0, 7, [(1, [10, 500, 900, 4000]), (2, [20, 600, 4100]),
                                (3, [30, 700, 4200, 30, 4200]), (4, [1234])])], rng, err=0.0)
    # span order of the star: root, then the children edge by edge
    flags = np.zeros(star.n_spans, np.uint16)
    flags[[1, 7, 8, 10, 11, 12, 13]] = 1  # min of (0,1); max of (0,2); 30, 4200, 30, 4200; the lone span
    star = with_flags(star, flags)
    sp = anomod.SpanSet.concat([bg, star, bg])
    ref = native.edge_aggregate(sp)
    if rate == 0.0:
        assert ref["errors"][[1, 2, 3, 4]].tolist() == [1, 1, 4, 1] and ref["count"][4] == 1
    fmt = model_fmt(sp)
    assert fmt[0] == "cell"
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, fmt, layout=model_layout(sp))
    dev.free()


# ---- 4. field extremes --------------------------------------------------------
def test_field_extremes(ctx, monkeypatch, capfd):
    """The last code's one span sits in the last cell with the largest residual
    and the error flag: the last code, the error bit, the last cell and every
    bit of the residual field at once.  The first code's minimum is cell 0 with
    residual 0 and no error.  Spans outside every trace take the skip word."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    S, R = 6, 9
    rng = np.random.default_rng(4)
    top = _bounds(_last_bin(R))[1]
    low = _bounds(70)[0]
    groups = [(0, 50, [(0, [low, low + 1, 999, 2000])])]
    groups += [(a, 50 + a, [(b, [10 * b + 3, 800 + a]) for b in range(S)]) for a in range(1, S - 1)]
    groups += [(S - 1, top, [])]
    core = star_set(S, groups, rng, fill=20, err=0.0)
    flags = np.zeros(core.n_spans, np.uint16)
    flags[-1] = 1
    flags[25:-1] = rng.random(core.n_spans - 26) < 0.2  # (past the 1 + 24 spans of the first group)
    core = with_flags(core, flags)
    ed = _edges(core)
    ref = native.edge_aggregate(core)
    used = np.flatnonzero(ref["count"])
    assert used[-1] == ed[-1] == S * S + S - 1 and ref["count"][used[-1]] == 1
    assert used[0] == 0 and ref["min_us"][0] == low and ref["errors"][0] == 0
    lay, fmt = model_layout(core), model_fmt(core)
    assert fmt[0] == "cell" and fmt[3] == R and top - _bounds(_last_bin(R))[0] == 2**R - 1
    sp = _offset_set(core, 3, 5, rng)
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, fmt, layout=lay)
    dev.free()


# ---- 5. launch cuts -----------------------------------------------------------
@pytest.mark.parametrize("cap", [1000, 4096])
def test_launch_cuts(ctx, monkeypatch, capfd, cap):
    """ANOMOD_MAX_LAUNCH_SPANS = 1000 and 4096 over about 6 000 spans.  Edge
    (0, 1) has spans in the first 100 positions only: in every later launch its
    entry keeps its initial value and must not be flushed.  Edge (0, 2) has its
    minimum before the first cut and its maximum after the last."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(cap)
    first = star_set(6, [(0, 40, [(1, [5, 77, 300, 4000] * 5), (2, [3, 500])])], rng, err=0.3)
    last = star_set(6, [(0, 41, [(2, [400, 4999])])], rng, err=0.3)
    mid = without_svc0(_random_spanset(rng, 6, 600, 20, dup=0.01), 3)  # service 0's edges: the stars' alone
    mid = with_dur(mid, rng.integers(0, 5000, mid.n_spans))
    sp = anomod.SpanSet.concat([first, mid, last])
    assert sp.n_spans > 4096 + 1000
    ed = _edges(sp)
    assert np.flatnonzero(ed == 1).max() < 100
    at2 = np.flatnonzero(ed == 2)
    assert at2.min() < 100 and at2.max() > sp.n_spans - 10
    ref = native.edge_aggregate(sp)
    assert ref["min_us"][2] == 3 and ref["max_us"][2] == 4999
    fmt = model_fmt(sp)
    assert fmt[0] == "cell"
    dev = ctx.upload(sp)
    monkeypatch.setenv("ANOMOD_MAX_LAUNCH_SPANS", str(cap))
    run(ctx, dev, ref, capfd, fmt, layout=model_layout(sp))
    monkeypatch.delenv("ANOMOD_MAX_LAUNCH_SPANS")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    dev.free()


# ---- 6. sum bound -------------------------------------------------------------
def test_sum_bound_cuts_the_launch(ctx, monkeypatch, capfd):
    """One workgroup (ANOMOD_DENSE_WGS=1), one edge of 4.5 M root spans, every
    duration at the largest residual of exponent 15.  A sum replica holds
    2^32 / 32767 = 131 076 such residuals, the 32 replicas of the one workgroup
    4 194 432: fewer than the set has.  The host gives a launch at most 256
    rounds (131 075 / 512 residuals per replica and round) of 16 384 spans, says
    so in the log, and sum_us is exact."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_WGS", "1")
    n = 4_500_000
    d = _bounds(_first_bin(15) + 1)[1]
    assert d - _bounds(_first_bin(15) + 1)[0] == 2**15 - 1
    assert n > 32 * (2**32 // (2**15 - 1)) and sum_rounds("small", 15) == 256
    rng = np.random.default_rng(6)
    sid = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    sp = anomod.SpanSet(["svc000", "svc001"], np.arange(n + 1, dtype=np.uint64), sid.copy(), sid,
                        np.zeros(n, np.uint64), np.ones(n, np.uint16),
                        (np.arange(n) % 5 == 0).astype(np.uint16), np.full(n, d, np.uint32))
    ref = native.edge_aggregate(sp)
    e = 2 * 2 + 1
    assert ref["count"][e] == n and ref["sum_us"][e] == n * d > 2**42
    fmt = model_fmt(sp)
    assert fmt == ("cell", 0, 2, 15), fmt
    dev = ctx.upload(sp)
    seen = run(ctx, dev, ref, capfd, fmt, layout=model_layout(sp))
    cuts = [(int(m[1]), int(m[2])) for m in map(_BOUND.search, seen) if m]
    assert cuts == [(256 * ROUND["small"], 1)] * 2, cuts  # the two dense calls
    dev.free()


# ---- 7. fallback to duration words -------------------------------------------
@pytest.mark.parametrize("kind", ["wide_edge", "long_durations"])
def test_fallback_to_duration_words(ctx, monkeypatch, capfd, kind):
    """An edge over all 896 bins (durations 0 and 2^32 - 1), and a set whose
    every duration lies far above 2^21 (exponent 26): the residual would take
    26 bits, the layout keeps duration words and the dense path as it was."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(7)
    sp = _random_spanset(rng, 6, 250, 20, dup=0.01)
    if kind == "wide_edge":
        sp = with_dur(sp, rng.integers(0, 3000, sp.n_spans))
        sp = anomod.SpanSet.concat([sp, star_set(6, [(1, 9, [(2, [0, U32MAX, 77])])], rng), sp])
    else:
        sp = with_dur(sp, rng.integers(U32MAX - 200_000, U32MAX, sp.n_spans, dtype=np.uint64))
        assert int(sp.dur_us.min()) > 2**21
    fmt = model_fmt(sp)
    assert fmt == ("dur", 10, 0, 21)
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run(ctx, dev, ref, capfd, fmt, layout=model_layout(sp))
    dev.free()


# ---- 8. another S, then back --------------------------------------------------
def test_another_service_count_changes_the_format(ctx, monkeypatch, capfd):
    """S alternates between 12 and 15 at the C ABI as in
    test_gpu_edge_dense.test_another_service_count.  One edge has all its spans
    at 2^32 - 1: at S = 12 its one bin of exponent 26 is part of the layout,
    which therefore keeps duration words; the calls at S = 15 run under
    ANOMOD_DENSE_SHRINK=1, which leaves that edge no cell, so that layout takes
    cell words (and that edge escapes).  The one word column is rewritten at
    every change and never read under the other format: every table is exact."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(8)
    bg = without_svc0(_random_spanset(rng, 12, 250, 20, dup=0.01), 11)  # edge (0, 1): the star's alone
    bg = with_dur(bg, rng.integers(0, 1000, bg.n_spans))
    sp = anomod.SpanSet.concat([bg, star_set(12, [(0, 8, [(1, [U32MAX] * 6)])], rng, err=0.5), bg])
    refs, want = {}, {}
    for S in (12, 15):
        wide = anomod.SpanSet([f"svc{i:03d}" for i in range(S)], sp.trace_ptr, sp.trace_hash,
                              sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us)
        refs[S] = native.edge_aggregate(wide)
        want[S] = model_fmt(wide, S, shrink=S == 15)
    assert want[12][0] == "dur" and want[15][0] == "cell", want
    dev = ctx.upload(sp)
    capfd.readouterr()
    seq = [12, 15, 12] + [12] * (2 + WAIT) + [15] * (3 + WAIT) + [12] * (3 + WAIT)
    for S in seq:
        if S == 15:
            monkeypatch.setenv("ANOMOD_DENSE_SHRINK", "1")
        else:
            monkeypatch.delenv("ANOMOD_DENSE_SHRINK", raising=False)
        assert_table_equal(_aggregate_abi(ctx, dev, S), refs[S])
    err = capfd.readouterr().err.splitlines()
    names = [ln for ln in err if "edge aggregation kernel" in ln]
    kind = ["dense" if DENSE in n else "codes" if CODES in n else "walk" if WALK in n else "rows"
            for n in names]
    stay = ["rows"] * (1 + WAIT) + ["codes", "dense"]
    assert kind == ["walk", "rows"] + stay + stay + stay, kind
    words = [(int(m[1]), m[2]) + tuple(int(m[k]) for k in (3, 4, 5)) for m in map(_WORDS.search, err) if m]
    assert words == [(S,) + want[S] for S in (12, 15, 12, 15, 12)], words
    dev.free()

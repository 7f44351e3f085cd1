"""Span-word column of the dense edge stream: from a set's fifth aggregation on
its dense calls read one u32 per span position — edge code, error bit and a
21-bit duration field — and nothing else; a duration above M, the largest the
field holds, is marked by the field's all-ones value and read from dur_us by
that span alone.

Every case runs a resident set through walk, row streams, the transition call
and at least two dense calls (run_calls checks the log), and every table of
every call, the E x 896 histogram included, equals the CPU oracle's bit for
bit.  Every constructed set is first held to the numpy layout model, so that
none silently stays on the row stream."""
import numpy as np
import pytest

import anomod
from oracle import native, spec

from test_gpu_edge_dense import (CODES, DENSE, LARGE, STREAM, WAIT, WALK, _log, _narrow, model_layout,
                                 plan, run_calls, star_set, with_dur)
from test_gpu_parent_rows import (_aggregate_abi, _offset_set, _random_spanset, assert_table_equal)

pytestmark = pytest.mark.gpu

# the word's duration field (csrc/common.h): M is the largest duration it holds, M + 1 its
# all-ones escape value, which a span of that very duration takes as well
DUR_BITS = 21
M = 2**DUR_BITS - 2
U32MAX = 2**32 - 1
# spans of one workgroup round of the dense kernel: 1024 threads x 4 spans x kLoad groups
# (DenseCfg<0>::kLoad = 4, DenseCfg<1>::kLoad = 8)
ROUND = {"small": 1024 * 4 * 4, "large": 1024 * 4 * 8}


def _bin(v):
    return int(spec.hist_bins_np(np.array([v], np.uint32))[0])


def _fits(sp, word=None, S=None, shrink=False):
    """The layout model of sp: it has to fit (and be the tier asked for)."""
    lay = model_layout(sp, S, shrink)
    assert lay[0] <= LARGE[0] and lay[1] <= LARGE[1] and lay[2] != "does", lay
    assert word is None or lay[2] == word, lay
    return lay


def _sprinkle(rng, dur, k):
    """dur with k random positions set to durations just above M."""
    dur = np.array(dur, np.uint32)
    at = rng.choice(dur.shape[0], k, replace=False)
    dur[at] = rng.integers(M + 1, M + 1 + 100_000, k)
    return dur


def test_escape_border(ctx, monkeypatch, capfd):
    """One edge with durations 0, M - 1, M, M + 1 and 2^32 - 1 in a narrow
    random background: M is the last duration the word holds, M + 1 (the
    field's all-ones value) and 2^32 - 1 come from dur_us."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(41)
    durs = [0, M - 1, M, M + 1, U32MAX]
    a = star_set(6, [(4, 3, [(5, durs * 3)])], rng, err=0.3)
    b, bd = _narrow(rng, 4, 800, 12, 500, dup=0.02)
    b = anomod.SpanSet(a.services, b.trace_ptr, b.trace_hash, b.span_id, b.parent_span_id, b.svc,
                       b.flags, bd.astype(np.uint32))
    sp = anomod.SpanSet.concat([b, a, b])
    lay = _fits(sp)
    ref = native.edge_aggregate(sp)
    e = 4 * 6 + 5
    assert ref["count"][e] == 15 and ref["min_us"][e] == 0 and ref["max_us"][e] == U32MAX
    assert ref["sum_us"][e] == 3 * sum(durs)
    for d in (M, M + 1):  # (one bin holds M - 1, M and M + 1)
        assert ref["hist"][e, _bin(d)] == 3 * sum(_bin(x) == _bin(d) for x in durs) >= 3
    assert ref["hist"][e, 895] == 3 and ref["hist"][e, 0] == 3
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=lay)
    dev.free()


@pytest.mark.parametrize("base", [M + 1, U32MAX - 200_000])
def test_every_span_escapes(ctx, monkeypatch, capfd, base):
    """About 5 000 spans, every duration above M, within a few bins: every
    lane of the full groups takes the escape load."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(base % 1000)
    sp = _random_spanset(rng, 6, 500, 20, dup=0.01)
    sp = with_dur(sp, rng.integers(base, base + 200_000, sp.n_spans, dtype=np.uint64))
    assert 4000 < sp.n_spans < 6500 and int(sp.dur_us.min()) > M
    lay = _fits(sp, "small")
    assert lay[1] <= 16 * lay[0]  # a few bins per edge
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=lay)
    dev.free()


@pytest.mark.parametrize("tier", ["small", "large"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("head", [1, 2, 3, 5])
def test_escapes_in_head_groups_and_tail(ctx, monkeypatch, capfd, tier, delta, head):
    """Ranges of one workgroup round - 1 / exact / + 1 spans that start at
    span position 1, 2, 3 or 5, with an escaping span at the first and the last
    position, the last singly read head position, the first tail position
    (where there is a tail) and a few inside the 16-B groups."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    n = ROUND[tier] + delta
    S, dmax = (4, 200) if tier == "small" else (12, 500)
    rng = np.random.default_rng(n * 8 + head)
    lens = []
    while sum(lens) < n:
        lens.append(int(min(rng.integers(0, 40), n - sum(lens))))
    core = _random_spanset(rng, S, 0, 0, lens=lens, dup=0.01)
    assert core.n_spans == n
    lo, hi = head, head + n
    a0, a1 = (lo + 3) & ~3, hi & ~3  # groups [a0, a1), head before, tail after
    at = {0, n - 1, a0 - lo - 1}
    if a1 < hi:
        at.add(a1 - lo)
    assert any((head + ROUND[tier] + d) & 3 for d in (-1, 0, 1))  # some delta has a tail
    at |= set(int(x) for x in rng.integers(a0 - lo, a1 - lo, 4))
    dur = rng.integers(0, dmax, n)
    for k, i in enumerate(sorted(at)):
        dur[i] = M + 1 + 1000 * k
    core = with_dur(core, dur)
    lay = _fits(core, tier)
    sp = _offset_set(core, head, 5, rng)
    ref = native.edge_aggregate(core)
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=lay)
    dev.free()


def test_field_separation(ctx, monkeypatch, capfd):
    """Exactly 512 codes.  The one span of code 511 carries the error flag and
    duration M - 1 (all bits of the code and error fields set, and all but one
    of the duration field), the spans of code 0 durations from 0 up and no error, and
    spans outside every trace take the skip word."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    S = 23
    groups = plan(S, LARGE[0], 700)
    assert len(groups) == 22 and groups[21][0] == 21
    groups[21] = (21, M - 1, groups[21][2])
    rng = np.random.default_rng(512)
    core = star_set(S, groups, rng, err=0.3)
    edges = np.asarray(native.span_edges(core, S), np.int64)
    used = np.unique(edges)
    assert used.shape[0] == LARGE[0]
    hi_span = np.flatnonzero((core.svc == 21) & (core.parent_span_id == 0))
    lo_span = np.flatnonzero(edges == used[0])
    assert hi_span.shape[0] == 1 and edges[hi_span[0]] == used[-1] == S * S + 21
    assert used[0] == 0 and lo_span.shape[0] == 2 and int(core.dur_us[lo_span].min()) == 0
    flags = core.flags.copy()
    flags[hi_span] = 1
    flags[lo_span] = 0
    core = anomod.SpanSet(core.services, core.trace_ptr, core.trace_hash, core.span_id,
                          core.parent_span_id, core.svc, flags, core.dur_us)
    lay = _fits(core, "large")
    assert lay[:2] == (LARGE[0], 700)
    ref = native.edge_aggregate(core)
    assert ref["errors"][used[-1]] == 1 and ref["sum_us"][used[-1]] == M - 1
    assert ref["errors"][0] == 0 and ref["count"][0] == 2 and 0 < ref["errors"].sum() < core.n_spans
    sp = _offset_set(core, 2, 5, rng)
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=lay)
    dev.free()


@pytest.mark.parametrize("cap", [1000, 4096])
def test_launch_caps(ctx, monkeypatch, capfd, cap):
    """ANOMOD_MAX_LAUNCH_SPANS: the dense stream is cut every `cap` spans;
    escaping spans sit on both sides of the first three cuts."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(cap + 1)
    sp = anomod.SpanSet.concat([_random_spanset(rng, 12, 1500, 12, dup=0.01),
                                _random_spanset(rng, 12, 0, 0, lens=[5000, 300]),
                                _random_spanset(rng, 12, 500, 3)])
    dur = rng.integers(0, 300, sp.n_spans)
    assert sp.n_spans > 3 * cap + 1
    for k in (1, 2, 3):
        dur[k * cap - 1], dur[k * cap] = M + 1 + k, M + 50_000 + k
    sp = with_dur(sp, dur)
    lay = _fits(sp)
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    monkeypatch.setenv("ANOMOD_MAX_LAUNCH_SPANS", str(cap))
    run_calls(ctx, dev, ref, capfd, layout=lay)
    monkeypatch.delenv("ANOMOD_MAX_LAUNCH_SPANS")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert DENSE in _log(capfd)[0][0]
    dev.free()


def test_shrunk_ranges_with_escapes(ctx, monkeypatch, capfd):
    """ANOMOD_DENSE_SHRINK=1 with escaping maxima: the largest span of such an
    edge takes the escape load and the histogram's HBM path at once."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    monkeypatch.setenv("ANOMOD_DENSE_SHRINK", "1")
    rng = np.random.default_rng(9)
    bg, bd = _narrow(rng, 6, 2500, 20, 500, dup=0.01)
    sp = anomod.SpanSet.concat([
        star_set(6, [(0, 5, [(1, [9, 10, 500, M + 5, M + 70_001]), (2, [M + 1, M + 1]),
                             (3, [0, M, U32MAX])])], rng),
        with_dur(bg, _sprinkle(rng, bd, 6))])
    want = _fits(sp, shrink=True)
    assert want[1] < model_layout(sp)[1]
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=want)
    dev.free()


def test_another_service_count(ctx, monkeypatch, capfd):
    """Dense at S = 12, then at S = 15 through that S's own transition (the
    column is rewritten for it), then at 12 again: the words of one S are
    never read under the other, and every table equals its reference."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(15)
    sp, dur = _narrow(rng, 12, 2000, 30, 300, dup=0.01)
    sp = with_dur(sp, _sprinkle(rng, dur, 10))
    refs = {}
    for S in (12, 15):
        wide = anomod.SpanSet([f"svc{i:03d}" for i in range(S)], sp.trace_ptr, sp.trace_hash,
                              sp.span_id, sp.parent_span_id, sp.svc, sp.flags, sp.dur_us)
        refs[S] = native.edge_aggregate(wide)
        _fits(wide, S=S)
    dev = ctx.upload(sp)
    capfd.readouterr()
    seq = [12] * (4 + WAIT) + [15] * (4 + WAIT) + [12] * (4 + WAIT)
    for S in seq:
        assert_table_equal(_aggregate_abi(ctx, dev, S), refs[S])
    names, lay = _log(capfd)
    kind = ["dense" if DENSE in n else "codes" if CODES in n else "walk" if WALK in n else "rows"
            for n in names]
    stay = ["rows"] * WAIT + ["codes", "dense", "dense"]
    assert kind == ["walk"] + stay + ["rows"] + stay + ["rows"] + stay, kind
    assert [x[0] for x in lay] == [12, 15, 12], lay
    dev.free()


def test_other_readers(ctx, monkeypatch, capfd):
    """A set in the dense state: download() returns the durations that were
    uploaded, and ANOMOD_EDGE_DENSE=0 then streams the rows and dur_us again
    into the same table."""
    monkeypatch.setenv("ANOMOD_LOG_KERNEL", "1")
    rng = np.random.default_rng(77)
    sp, dur = _narrow(rng, 12, 1500, 30, 300, dup=0.01)
    sp = with_dur(sp, _sprinkle(rng, dur, 10))
    lay = _fits(sp)
    ref = native.edge_aggregate(sp)
    dev = ctx.upload(sp)
    run_calls(ctx, dev, ref, capfd, layout=lay)
    back = dev.download()
    np.testing.assert_array_equal(back.dur_us, sp.dur_us)
    np.testing.assert_array_equal(back.flags, sp.flags)
    monkeypatch.setenv("ANOMOD_EDGE_DENSE", "0")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    names, _ = _log(capfd)
    assert len(names) == 1 and STREAM in names[0] and DENSE not in names[0], names
    monkeypatch.delenv("ANOMOD_EDGE_DENSE")
    assert_table_equal(ctx.edge_aggregate(dev), ref)
    assert DENSE in _log(capfd)[0][0]
    dev.free()

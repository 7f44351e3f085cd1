"""Host checks of tests/walk_ref.py (no GPU): its constants against the text of
csrc/walk.h and csrc/chunk.h, its arithmetic against hand-derived tables and
against a literal emulation of the three parent scans, and for every case that
the border the case names is reached according to the model and that every
pass's own reference has something to say about it.  test_gpu_walk_borders.py
runs the same cases on the device."""
import re
from pathlib import Path

import numpy as np
import pytest

import walk_ref as W
from walk_ref import NO_PARENT

CASES = W.case_names()


def _csrc():
    import anomod
    return Path(anomod.__file__).resolve().parents[1] / "csrc"


# ------------------------------------------------------------------ constants
def test_constants_restate_the_kernel_source():
    """A retune of the walk fails here until the borders follow."""
    walk, chunk = (_csrc() / "walk.h").read_text(), (_csrc() / "chunk.h").read_text()
    for text, line in (
            (chunk, f"constexpr int kWave = {W.CHUNK_TRACES};"),
            (chunk, f"constexpr int kStage = {W.STAGE};"),
            (chunk, f"constexpr uint32_t kFwd = {W.BIDIR[0]}, kBwd = {W.BIDIR[1]};"),
            (chunk, f"constexpr uint32_t kScanSlack = {W.SCAN_SLACK};"),
            (chunk, "const bool fits = valid && (hi - c.base) <= (uint64_t)kStage;"),
            (walk, f"constexpr uint32_t kNarrowRows = {W.NARROW_ROWS};"),
            (walk, f"constexpr uint32_t kSplitFwd = {W.SPLIT[0]}, kSplitBwd = {W.SPLIT[1]};"),
            (walk, f"constexpr uint32_t kFwdScan = {W.FWD};"),
            (walk, f"constexpr uint64_t kDynSeg = {W.DYN_SEG};"),
            (walk, "constexpr int kBigThreads = 512;"), (walk, "constexpr int kBigPer = 8;"),
            (walk, f"constexpr uint32_t kBigWin = {W.BIG_WIN};"),
            (walk, "constexpr uint32_t kBigSlots = 2 * kBigWin;"),
            (walk, "return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & (kBigSlots - 1u);"),
            (walk, "return find_parent_split<kSplitFwd, kSplitBwd>(llo, lhi, a, b, i, pid);"),
            (walk, "return find_parent_bidir<kFwd, kBwd>(lsid, a, b, i, pid);"),
            (walk, "const uint64_t n_static = n_traces - n_traces / DYN;"),
            (walk, "for (uint32_t w0 = 0; w0 < L; w0 += kBigWin) {")):
        assert line in text, line
    assert W.BIG_BLOCK == 512 * 8 and W.BIG_SLOTS == 2 * W.BIG_WIN
    assert max(W.FWD, W.BIDIR[0], W.SPLIT[0]) <= W.SCAN_SLACK
    span_walk = (_csrc() / "span_walk.hip").read_text()
    assert ("*scan = !uni ? kScanFwd : (E > kNarrowRows || long_set) ? kScanSplit : kScanBidir;"
            in span_walk)
    for f in ("self_time", "critical_path", "trace_shapes", "spectrum", "error_origins"):
        m = re.findall(r"walk_traces<\w+, (\d+), Regs>\(", (_csrc() / f"{f}.hip").read_text())
        assert m == [str(W.DYN)], (f, m)


def test_big_slot_restates_the_multiply_shift():
    for x in (1, 2, 0x9E3779B97F4A7C15, 2**64 - 1, 0x0123456789ABCDEF, 1 << 63):
        want = (((x * 0x9E3779B97F4A7C15) % 2**64) >> 32) & 4095
        assert int(W.big_slot([x])[0]) == want
    assert int(W.big_slot([1])[0]) == 0x9E3779B9 & 4095 == 0x9B9
    assert int(W.big_slot([0])[0]) == 0      # (id 0 is the table's empty key: never inserted)
    assert [W.big_windows(L) for L in (257, 2048, 2049, 4096, 4097, 6145)] == [1, 1, 2, 2, 3, 4]
    assert [W.big_blocks(L) for L in (257, 4096, 4097, 8193)] == [1, 1, 2, 3]


def test_tail_chunks_by_hand():
    """Three length lists walked by hand.  (1) 8 traces: the tail is the last
    two, one run.  (2) 16 traces, tail [12, 16): 200 + 56 fill a chunk, 1 does
    not fit any more, 300 is long.  (3) 280 traces of one span: the tail is
    the last 70, a chunk of 64 and one of 6."""
    assert W.tail_start(8) == 6 and W.tail_start(7) == 6 and W.tail_start(3) == 3
    assert W.tail_chunks([9] * 6 + [3, 4]) == [(6, 2, 7)]
    assert W.tail_chunks([1] * 12 + [200, 56, 1, 300]) == [(12, 2, 256), (14, 1, 1), (15, 0, 300)]
    assert W.tail_chunks([1] * 280) == [(210, 64, 64), (274, 6, 6)]
    # a segment border: 4 * 520 traces, the tail's 520 in segments of 512 and 8
    ch = W.tail_chunks([1] * 2080)
    assert ch[0] == (1560, 64, 64) and ch[7] == (2008, 64, 64) and ch[8:] == [(2072, 8, 8)]
    assert W.tail_chunks([1, 1, 1]) == []        # n // 4 == 0: no dynamic tail


def test_scan_of():
    assert W.scan_of(False, 30, True) == "fwd"
    assert W.scan_of(True, 9, False) == "bidir" and W.scan_of(True, 9, True) == "split"
    assert W.scan_of(True, 21, False) == "bidir" and W.scan_of(True, 22, False) == "split"
    assert (21 + 2) * 21 <= W.NARROW_ROWS < (22 + 2) * 22


# ------------------------------------------------------------------ the scans, literally
def _emulate(ids, a, b, i, pid, kind):
    """find_first / find_parent_bidir / find_parent_split as loops over the
    staged ids (the split scan on unique low words is the bidirectional scan
    with its own widths) -> (position or -1, Hit fields)."""
    clamps = []
    if kind == "fwd":
        q0, step = a, 0
        while q0 < b:
            m = [j for j in range(W.FWD) if ids[q0 + j] == pid]
            hi = min(b - q0, W.FWD)
            m = [j for j in m if j < hi]
            if m:
                return q0 + m[0], (step, "f", m[0], hi, False, ())
            q0, step = q0 + W.FWD, step + 1
        return -1, (step, "", -1, min(b - (q0 - W.FWD), W.FWD), False, ())
    FW, BW = W.BIDIR if kind == "bidir" else W.SPLIT
    f, g, step = a, i - 1, 0
    while True:
        gb0 = g - BW + 1
        gb = a if gb0 < a else gb0
        v = [ids[f + j] for j in range(FW)]
        w = [ids[gb + j] for j in range(BW)]
        hi = min(b - f, FW)
        nb = g - gb + 1
        if gb0 < a:
            clamps.append(max(nb, 0))
        mf = [j for j in range(FW) if v[j] == pid and j < hi]
        mb = [j for j in range(BW) if w[j] == pid and j < nb]
        if mf:
            return f + mf[0], (step, "f", mf[0], hi, gb0 < a, tuple(clamps))
        if mb:
            return gb + mb[-1], (step, "b", mb[-1], hi, gb0 < a, tuple(clamps))
        f, g, step = f + FW, g - BW, step + 1
        if f >= b:
            return -1, (step, "", -1, hi, gb0 < a, tuple(clamps))


@pytest.mark.parametrize("kind", ["fwd", "bidir", "split"])
def test_scan_hit_matches_the_loops(kind):
    """All (a, b, i, q) with b - a <= 40, q = None included; the ids around
    the trace are other ids (the scans read up to the slack past b)."""
    n = 0
    for a in (0, 7):
        for L in range(1, 41):
            b = a + L
            ids = list(range(1000, 1000 + b + W.SCAN_SLACK + 1))
            for i in range(a, b):
                for q in [None] + list(range(a, b)):
                    pid = 5 if q is None else ids[q]
                    pos, want = _emulate(ids, a, b, i, pid, kind)
                    assert pos == (-1 if q is None else q)
                    h = W.scan_hit(a, b, i, q, kind)
                    got = (h.step, h.side, h.slot, h.valid, h.clamped, h.clamps)
                    assert got == want, (a, b, i, q, got, want)
                    if q is not None:
                        st = W.scan_steps(a, b, i, kind)[h.step]
                        assert (st.valid, st.clamped) == (h.valid, h.clamped)
                        assert not (h.side == "b" and h.clamped)   # ladder_required's premise
                    n += 1
    assert n == 2 * sum(L * (L + 1) for L in range(1, 41))


# ------------------------------------------------------------------ the cases
def test_case_list():
    """Every shape in every regime the rules allow, and nothing dropped: 112
    cases, 560 (shape, regime, pass) combinations."""
    assert len(CASES) == len(set(CASES)) and len(W.SHAPES) == len(set(W.SHAPES)) == 45
    by = {s: W.regimes(s) for s in W.SHAPES}
    for s, r in by.items():
        sh = W.shape(s)
        assert r == (("F",) if sh.dup else ("F", "P") if W.has_long(sh) else ("F", "B", "P")), s
    assert [s for s, r in by.items() if r == ("F",)] == ["big_window_borders"]
    assert sum(r == ("F", "P") for r in by.values()) == 21
    assert sum(r == ("F", "B", "P") for r in by.values()) == 23
    assert len(CASES) == 1 + 2 * 21 + 3 * 23 == 112
    assert len(CASES) * len(W.PASSES) == 560
    for kind in ("fwd", "rev", "shuf"):
        for L in (255, 256, 257, 4095, 4096, 4097, 8193):
            assert f"chain_{kind}_{L}-F" in CASES and f"chain_{kind}_{L}-P" in CASES
    for s in ("scan_ladder_fwd", "scan_ladder_bidir", "scan_ladder_split", "word_border_starts"):
        assert by[s] == ("F", "B", "P")


def _chunk_of(chunks, t):
    mine = [ch for ch in chunks if ch[0] <= t < ch[0] + max(ch[1], 1)]
    assert len(mine) == 1
    return mine[0]


def _check_ladder(c, chunks):
    kind = c.facts["ladder"]
    FW, BW = W._widths(kind)
    sp, par = c.sp, c.par
    sid, pid = sp.span_id, sp.parent_span_id
    combos, clamps, decoys, reread, tail_read = set(), set(), set(), set(), set()
    for t, info in c.facts["targets"].items():
        a, b = c.bounds(t)
        ch = _chunk_of(chunks, c.first + t)          # mid-chunk, between its neighbours
        assert ch[0] < c.first + t and c.first + t + 1 < ch[0] + ch[1], (t, ch)
        pa, pb = c.bounds(t - 1)
        na, nb_ = c.bounds(t + 1)
        for i, q in info["par"].items():
            assert par[a + i] == (NO_PARENT if q == i else a + q)
            h = W.scan_hit(a, b, a + i, a + q, kind)
            combos.add(W.hit_combo(h, kind))
            clamps |= set(h.clamps)
        for i in info["orphans"]:
            assert par[a + i] == NO_PARENT and pid[a + i] != 0
            clamps |= set(W.scan_hit(a, b, a + i, None, kind).clamps)
        for i, side, d in info["decoys"]:
            at = b - 1 + d if side == "next" else a - d
            assert (na <= at < nb_) if side == "next" else (pa <= at < pb)
            # an orphan here, not an orphan if the neighbouring trace were searched
            assert pid[a + i] == sid[at] and par[a + i] == NO_PARENT
            assert sid[at] not in sid[a:b]
            decoys.add((side, d))
            steps = W.scan_steps(a, b, a + i, kind)
            if side == "next" and at < steps[-1].f + FW:
                tail_read.add(d)                     # read by the last forward block, masked by hi
            st = steps[0]
            if side == "next" and BW and st.gb <= at < st.gb + BW:
                reread.add(max(st.nb, 0))            # read by a clamped backward block, cut by nb
        al = info["alias"]
        if al:
            lo = lambda x: int(x) & 0xFFFFFFFF       # noqa: E731
            i, r, q = al["false_candidate"]
            assert lo(sid[a + r]) == lo(sid[a + q]) and sid[a + r] != sid[a + q]
            hr, hq = W.scan_hit(a, b, a + i, a + r, kind), W.scan_hit(a, b, a + i, a + q, kind)
            assert (hr.step, hr.side == "b") < (hq.step, hq.side == "b") and par[a + i] == a + q
            i, r = al["no_parent"]
            assert lo(pid[a + i]) == lo(sid[a + r]) and par[a + i] == NO_PARENT
            assert pid[a + i] not in sid[a:b]
            i, r = al["neighbour"]
            assert lo(pid[a + i]) == lo(sid[na + r]) and pid[a + i] != sid[na + r]
            assert par[a + i] == NO_PARENT
        if b - a > 2 * FW:                           # a main target: several parent services
            kids = [i for i in range(a, b) if par[i] != NO_PARENT]
            assert len({int(sp.svc[par[i]]) for i in kids}) >= 2
            assert sid[a] == pid[a] and sid[b - 1] == pid[b - 1]     # the self-references
    missing = W.ladder_required(kind) - combos
    print(c.name, "combinations:", len(combos), "missing:", sorted(missing))
    assert not missing
    assert decoys >= ({("next", d) for d in range(1, FW + 1)} |
                      {("prev", d) for d in range(1, (BW or 4) + 1)})
    assert tail_read >= set(range(1, FW))
    if BW:
        assert clamps >= set(range(BW)), clamps
        assert reread >= {0, 1, 2}, reread
    if kind == "split":
        assert any(info["alias"] for info in c.facts["targets"].values())


def _rel_starts(c, ch):
    t0, k, _ = ch
    lens = c.lens
    return [(int(lens[t0:t].sum()), int(lens[t])) for t in range(t0, t0 + k)]


@pytest.mark.parametrize("name", CASES)
def test_case_reaches_its_border(name):
    c = W.case(name)
    sp, f, sh = c.sp, c.facts, W.shape(c.shape_name)
    lens = c.lens
    nt = sp.n_traces
    # the regime is what it says
    declared = sp.unique_ids
    assert declared == (c.regime != "F")
    try:   # check_unique_ids() sets the flag of the cached set
        assert sp.check_unique_ids() == (not sh.dup)
    finally:
        sp.unique_ids = declared
    assert c.scan == {"F": "fwd", "B": "bidir", "P": "split"}[c.regime]
    assert c.scan == W.scan_of(declared, c.S, bool((lens > W.STAGE).any()))
    assert c.n_long == int((lens > W.STAGE).sum()) and (c.regime != "B" or c.n_long == 0)
    assert (c.S + 2) * c.S > W.NARROW_ROWS if c.regime == "P" and not c.n_long else c.S == 9
    # where the device runs the shape: all of it in the dynamic tail
    chunks = W.tail_chunks(lens.tolist())
    if c.shape_name in W.NO_FILLERS:
        assert c.first == 0
    else:
        assert c.first == W.tail_start(nt) == 3 * len(sh.traces) and (lens[:c.first] == 1).all()
        assert not chunks or chunks[0][0] == c.first
        assert (nt - c.first <= W.DYN_SEG) == (c.shape_name != "segment_border")
    for t in np.flatnonzero(lens > W.STAGE):
        if t >= W.tail_start(nt):
            assert _chunk_of(chunks, t) == (t, 0, lens[t])
    if "chunks" in f:
        assert [(k, n) for _, k, n in chunks] == f["chunks"]
    if "ladder" in f:
        _check_ladder(c, chunks)
    if "starts" in f:
        rel = [_rel_starts(c, ch) for ch in chunks]
        starts = {s for r in rel for s, L in r if L}
        assert f["starts"] <= starts and all(ch[2] == W.STAGE for ch in chunks)
        assert [x for x in rel[0] if x[1]][-1] == (255, 1)
        for ci, w in f["bare_words"]:
            assert not any(64 * w <= s < 64 * w + 64 for s, L in rel[ci] if L)
        assert rel[0][0][1] == 0 and rel[0][-1][1] == 0 and rel[1][-1][1] == 0   # front, end
        assert any(L == 0 and 0 < s < 256 for s, L in rel[1])                    # between
        shp = c.refs["trace_shapes"][2][c.first:][lens[c.first:] > 0]
        assert np.unique(shp).shape[0] == shp.shape[0]        # a distinct answer per trace
        assert len(set(c.refs["spectrum"][1]["trace_abnormal"][c.first:].tolist())) == 2
    if "segments" in f:
        for s in f["segments"]:
            assert any(t0 + max(k, 1) == c.first + s for t0, k, _ in chunks)
        t0, k, n = next(ch for ch in chunks if ch[0] + ch[1] == c.first + 1024)
        assert 0 < k < W.CHUNK_TRACES and n + lens[t0 + k] <= W.STAGE    # more would fit
        for t, L in f["long_at"].items():
            assert (c.first + t, 0, L) in chunks
    if "cluster" in f and c.shape_name == "big_cluster_4095":
        a, b = c.bounds(0)
        ids = sp.span_id[a:b]
        slot = W.big_slot(ids[ids != 0])
        assert 600 <= b - a <= W.BIG_WIN and W.big_windows(b - a) == 1
        assert f["cluster"][0] == W.BIG_SLOTS - 1 and f["cluster"][1] >= 40
        assert int((slot == W.BIG_SLOTS - 1).sum()) >= 40 and int((slot < 40).sum()) >= 40
        z = a + f["zero_at"]
        assert sp.span_id[z] == 0 and c.par[z] != NO_PARENT and not (c.par == z).any()
        order = f["chain"]
        np.testing.assert_array_equal(c.par[a + order[1:]], a + order[:-1])
        assert np.isin(np.flatnonzero(W.big_slot(ids) == W.BIG_SLOTS - 1), order).all()
    if "planted" in f:
        rel = set()
        for t, want in f["planted"].items():
            a, b = c.bounds(t)
            L = b - a
            for child, parent in want.items():
                assert c.par[a + child] == a + parent, (t, child)
                rel.add((child // W.BIG_BLOCK, parent // W.BIG_WIN))
            for w in range(W.big_windows(L) - 1):
                e = W.BIG_WIN * (w + 1)
                assert {e - 1, e} <= set(want.values())
            if L % W.BIG_WIN == 1:               # the last window holds one span, a parent
                assert L - 1 in want.values()
        assert (1, 0) in rel and any(cb == 0 and pw >= 2 for cb, pw in rel)
        assert set(f["dups"]) == {2, 3, 4}
        for t, (p, q) in f["dups"].items():
            a, _ = c.bounds(t)
            assert sp.span_id[a + p] == sp.span_id[a + q] and p // W.BIG_WIN != q // W.BIG_WIN
            kids = np.flatnonzero(c.par == a + p) - a
            assert {q + 1, q + 2} <= set(kids.tolist()) and not (c.par == a + q).any()
    if "low_twins" in f:
        a, _ = c.bounds(sh.target)
        i, j = f["low_twins"]
        assert (int(sp.span_id[a + i]) ^ int(sp.span_id[a + j])) == 1 << 40
    if "long_traces" in f:
        assert c.n_long == f["long_traces"] == 2 * W.MI355X_CUS + 88
        assert 150_000 < sp.n_spans < 190_000 and lens[-1] > W.STAGE
    if "set_spans" in f:
        assert sp.n_spans == 0 and not c.refs
        return
    # every pass's reference alone has something to say about the set
    r = c.refs
    lo = int(sp.trace_ptr[c.first])
    linked = int((c.par[lo:] != NO_PARENT).sum())
    su, tab = r["self_time"]
    assert int(tab["count"].sum()) == sp.n_spans
    cp, on, nsel, cptab = r["critical_path"]
    # (a trace that is one reference cycle has no head: nothing of it is on a path)
    assert on[lo:].any() != c.shape_name.startswith("cycle_whole")
    assert int(cptab["count"].sum()) == int(on.sum())
    assert np.unique(r["trace_shapes"][2]).shape[0] >= 2
    assert int(r["spectrum"][1]["n_traces"].sum()) == nt
    if linked >= 3:
        assert (su[lo:] != sp.dur_us[lo:]).any() and nsel[lo:].any()
        assert len(set(r["spectrum"][0][lo:].tolist())) >= 2      # several edge rows
    if sp.n_spans - lo >= 60:
        o = r["error_origins"]
        assert o.error_spans > 0 and (nt < 40 or r["spectrum"][1]["n_traces"].min() > 0)
        assert int(o.origin.sum()) > 0 and (linked < 30 or int(o.propagated.sum()) > 0)
        d = sp.dur_us[lo:]
        assert (d == 0).any() and (d == W.U32_MAX).any()
        # not sorted by position (starts are laid down from the heads: a whole cycle has none)
        assert (np.diff(sp.start_us[lo:].astype(np.int64)) < 0).any() == on[lo:].any()
    if "ladder" in f or "starts" in f:
        err = (sp.flags & W.ERR) != 0
        kid = np.flatnonzero(c.par != NO_PARENT)
        heads = c.par[c.par[kid]] == NO_PARENT
        leaf = ~np.isin(kid, c.par)
        assert (err[kid] & ~err[c.par[kid]] & heads & leaf).any()     # flagged leaf, clean root
        assert (~err[kid] & err[c.par[kid]] & heads & leaf).any()     # and the reverse

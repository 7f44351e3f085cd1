"""CPU: the model of the shared edge stream (tests/stream_ref.py) against
itself and against the passes' reference helpers — every case reaches the
geometry and the ring events it names (a case that missed its border would
test nothing on the GPU), the ring simulation's table (flushed slots plus
global adds) is the plain per-span table and the pass's reference, grid_of is
stream_grid, lane_positions covers a batch.  Run with -s to read, per case and
pass, the events reached."""
import numpy as np
import pytest

import stream_ref as S
from edge_load_ref import assert_load_equal

CASES = S.case_names()
STRUCTURAL = {"anchor", "advance", "wrap", "jump", "backward", "no_window_batch", "finish_cut",
              "never_anchored"}


def test_grid_of_is_stream_grid():
    for B in (S.B_WIDE, S.B_CELL):
        for cap in (1, 2, 3, 4):
            ns = sorted({1, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B, 3 * B + 1, 4 * B + 1, 5 * B,
                         6 * B, 7 * B - 1, 12 * B + 5} | set(range(cap * B - 2, cap * B + 3)))
            for n in ns:
                if cap > -(-n // B):
                    continue
                for num_cus, per_cu in ((256, 1), (256, S.CELL_PER_CU), (64, 2), (4, 1)):
                    max_range = 1 << 31 if B == S.B_WIDE else 2**64 - 1
                    want = S.stream_grid_literal(num_cus, n, B, per_cu, cap, max_range)
                    assert S.grid_of(n, B, cap) == want, (n, B, cap, num_cus, per_cu)
                grid, per_wg = S.grid_of(n, B, cap)
                ranges = S.wg_ranges(n, B, cap)
                assert per_wg % B == 0 and len(ranges) == grid <= cap
                assert ranges[0][0] == 0 and ranges[-1][1] == n
                assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
                assert all(lo < hi for lo, hi in ranges)


@pytest.mark.parametrize("B,run", [(S.B_WIDE, 2), (S.B_WIDE, 4), (S.B_CELL, 2)])
def test_lane_positions_cover_the_batch(B, run):
    threads, b = S.THREADS[B], 3 * B
    pos = [p for tid in range(threads) for p in S.lane_positions(b, tid, threads, run)]
    assert sorted(pos) == list(range(b, b + B))
    for tid in (0, 1, threads - 1):
        p = S.lane_positions(b, tid, threads, run)
        # runs of `run` consecutive positions, threads * run apart
        assert all(p[j + 1] == p[j] + 1 for j in range(3) if (j + 1) % run)
        if run == 2:
            assert p[2] == p[0] + threads * 2


def test_min_holders_of_c7():
    """The span that alone holds the batch minimum sits where the case says."""
    for label, (tid, jk, jr) in S.MIN_HOLDER.items():
        c = S.case(f"{label}@{S.B_WIDE}")
        w = S.window_of(c.sp.start_us, c.t0, c.step, c.T)
        batch = w[S.B_WIDE:2 * S.B_WIDE]
        x = int(np.argmin(batch))
        assert (batch == batch.min()).sum() == 1
        keys = [t for t in range(512) if S.B_WIDE + x in S.lane_positions(S.B_WIDE, t, 512, 2)]
        rows = [t for t in range(512) if S.B_WIDE + x in S.lane_positions(S.B_WIDE, t, 512, 4)]
        pk = S.lane_positions(S.B_WIDE, keys[0], 512, 2).index(S.B_WIDE + x)
        pr = S.lane_positions(S.B_WIDE, rows[0], 512, 4).index(S.B_WIDE + x)
        if jk is not None:
            assert pk == jk and (tid is None or keys[0] == tid), (label, keys, pk)
        if jr is not None:
            assert pr == jr, (label, rows, pr)
        if label == "c7-last":
            assert keys[0] == rows[0] == 511 and keys[0] % S.WAVE == 63


def _matches(events, want):
    return all(e[:len(x)] == tuple(x) for e, x in zip(events, want)) and len(events) >= len(want)


@pytest.mark.parametrize("name", CASES)
def test_case_reaches_its_borders(name):
    c = S.case(name)
    refs = c.refs()
    sp = c.sp
    assert sp.n_spans <= 8 * S.B_WIDE   # c1 at Wt = 3: 2 Wt + 2 batches
    ptr = sp.trace_ptr.astype(np.int64)
    assert (np.diff(ptr) >= 0).all() and 0 <= ptr[0] and ptr[-1] <= sp.n_spans
    lens = np.diff(ptr)
    assert lens.min() >= 1 and lens.max() <= 3
    for p in c.passes:
        exp = c.expect[p]
        geo = S.geometry(c, p)
        if "grid" in exp:
            assert geo[0][2:] == (exp["grid"], exp["per_wg"]), (p, geo)
        if "bounds" in exp:
            assert geo[1][2:] == (exp["bounds"]["grid"], exp["bounds"]["per_wg"]), (p, geo)
        print(f"{name} {p}: " + "; ".join(f"{k} n={n} grid={g} per_wg={pw}" for k, n, g, pw in geo))
        if p in S.RING_PASSES:
            _ring(c, p, exp, refs)
    if "quantiles" in c.passes:
        _cells(c, c.expect["quantiles"])
    if "exemplars" in c.passes:
        _exemplars(c, c.expect["exemplars"], refs["exemplars"])
    if not name.startswith("d") and sp.n_spans > 8:
        rows = c.rows()[c.begin:c.end]
        S_ = len(sp.services)   # real parents, ROOT rows and ORPHAN rows all occur
        assert (rows // S_ == S_).any() and (rows // S_ == S_ + 1).any() and (rows // S_ < S_).any()


def _ring(c, p, exp, refs):
    ref = refs[p]
    Wt, events, table, hits = S.simulate(c, p)
    assert Wt == exp["Wt"], (p, Wt)
    wg0 = [e[1:] for e in events if e[0] == 0]
    names = {e[1] for e in events}
    print(f"  {p}: Wt={Wt} hits={hits} events={events}")
    first = exp.get("first")
    if first:
        keep = STRUCTURAL | {x[0] for x in first}
        walk = [e for e in wg0 if e[0] in keep]
        assert _matches(walk, first), (p, walk, first)
        if c.ring_extra:
            assert len(walk) == len(first), (p, walk, first)
    assert exp.get("names", set()) <= names, (p, names)
    for ev in exp.get("events", ()):
        assert any(e[:len(ev)] == ev for e in events), (p, ev, events)
    if c.ring_extra:
        assert hits > 0
    # the ring's table is the plain table and the pass's reference
    np.testing.assert_array_equal(table, S.plain_table(c, p))
    ones = S.simulate(c, p, ones=True)[2]
    if p == "windows":
        np.testing.assert_array_equal(table, ref.sum_us)
        np.testing.assert_array_equal(ones, ref.count)
        w = S.window_of(c.sp.start_us, c.t0, c.step, c.T)
        assert ref.outside == int(((w < 0) & c.live()).sum())
    else:
        w, _ = S.pass_windows(c, p)
        assert ref.outside == int(((w < 0) & c.live()).sum())
        end = c.sp.start_us.astype(np.int64) + c.sp.dur_us.astype(np.int64)
        inside = (c.sp.start_us.astype(np.int64) - c.t0) % c.step + c.sp.dur_us <= c.step
        if (inside | ~c.live() | (w < 0)).all():   # no span leaves its window: heads only
            np.testing.assert_array_equal(table, ref.busy_us)
            assert not ref.carried.any()
        else:
            assert c.name.startswith("c9") and (ref.busy_us >= table).all() and ref.carried.any()
            assert int((ref.busy_us - table).sum()) > 0
            if c.name.startswith("c9-c2"):   # some spans are clipped at the end of the range
                assert end.max() > c.t0 + c.T * c.step
        brute = S.load_brute(c)
        if brute is not None:
            assert_load_equal(ref, brute)
    if c.ring_extra:   # c8: the same case with every span to global atomics
        Wt0, ev0, table0, hits0 = S.simulate(c, p, tile=0)
        assert (Wt0, ev0, hits0) == (0, [], 0)
        np.testing.assert_array_equal(table0, table)


def _cells(c, exp):
    borders = S.cell_borders(c)
    m = c.end - c.begin
    print(f"  quantiles: m={m} cell borders={borders if len(borders) < 40 else len(borders)} "
          f"sentinel at {S.sentinel_start(c)}")
    if "borders" not in exp:
        return
    want = list(exp["borders"])
    sent = exp["sentinel"]
    assert borders == want + ([sent] if sent is not None else []), (borders, want, sent)
    assert S.sentinel_start(c) == sent
    if c.name.startswith(("d1", "d4")):
        ranges = S.wg_ranges(m, S.B_CELL, c.cap)
        reach = set(borders)
        if sent is None:
            assert {1, 128, 512, 640, S.B_CELL, m - 1, 5 * S.B_CELL} <= reach
            assert {lo for lo, _ in ranges[1:]} <= reach and len(ranges) == c.cap
            assert m % S.B_CELL and (m // S.B_CELL) * S.B_CELL in reach   # the partial batch
    if c.name.startswith("d2"):
        assert borders == []
    if c.name.startswith("d3"):
        assert borders == list(range(1, m))


def _exemplars(c, exp, refs):
    E = c.E
    for k in c.ks:
        ref = refs[k]
        places = {pl: S.exemplars_place(E, k, cap) for pl, cap in
                  (("lds", S.NO_CAP), ("global", 0), ("cached", E * 8))}
        assert places["lds"] == "lds" and places["global"] == "global"
        assert places["cached"] == ("cached" if k > 1 else "lds")   # K = 1: E * 8 holds the lists
        found = ref.n_found
        print(f"  exemplars k={k}: n_found={found.tolist()}")
        if c.name.startswith("e4") and k == 64:
            assert ((found > 0) & (found < k)).any() and (found == k).any()
        if exp.get("marks") and c.name.startswith("e2"):
            assert set(exp["marks"]) <= set(ref.position[ref.position != 2**64 - 1].tolist())
        if exp.get("marks") and c.name.startswith("e3") and k >= 3:
            row = int(c.rows()[exp["marks"][0]])
            top = ref.position[row, :min(k, len(exp["marks"]))].tolist()
            assert set(top) <= set(exp["marks"])
            ranges = S.wg_ranges(c.end, S.B_WIDE, c.cap)
            assert {sum(p >= lo for lo, _ in ranges) for p in top} == {1, 2, 3}
        if c.name.startswith("e1"):
            rows = c.rows()
            for r in np.nonzero(found)[0].tolist():
                lowest = np.nonzero((rows == r) & c.live())[0][:k]
                np.testing.assert_array_equal(ref.position[r, :len(lowest)], lowest.astype(np.uint64))
        if c.name.startswith("e5"):
            assert c.begin > 0
    if c.name.startswith("e"):
        ranges = S.wg_ranges(c.end, S.B_WIDE, c.cap)
        assert len(ranges) == 3 and (ranges[-1][1] - ranges[-1][0]) < S.B_WIDE

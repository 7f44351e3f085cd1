"""Trace-grouping model, host side (no GPU): tests/group_ref.py against the
kernel sources' constants and hand-derived geometry, and THE CAP: every case
the GPU file (tests/test_gpu_group_borders.py) runs is built here and
layout(), which counts straight from mix64(trace_hash), must show that it
hits the border it is named after.  No plan may miss, or the GPU cases would
pass vacuously."""
import re
from pathlib import Path

import numpy as np
import pytest

import group_ref as G
from oracle import spec


def test_unmix64_inverts_mix64():
    rng = np.random.default_rng(0)
    k = np.r_[rng.integers(0, 2**64, 1000, dtype=np.uint64),
              np.array([0, 1, G.ONES, G.ONES - 1, 1 << 63, (1 << 63) - 1], np.uint64)]
    h = G.unmix64(k)
    np.testing.assert_array_equal(spec.mix64(h), k)
    np.testing.assert_array_equal(G.unmix64(spec.mix64(k)), k)
    assert int(G.unmix64(np.uint64(0))[0]) == 0  # mix64(0) = 0
    assert np.unique(h).shape[0] == k.shape[0]


@pytest.mark.parametrize("avg,n,want", [
    (64, 2049, (5, 5, 0)), (64, 100000, (11, 11, 0)), (64, 140000, (12, 6, 6)),
    (64, 300000, (13, 7, 6)), (64, 524288, (13, 7, 6)), (1400, 524289, (9, 9, 0)),
    # the clamps and the caps of the rule
    (1, 2049, (5, 5, 0)), (5000, 1 << 22, (11, 11, 0)), (None, 1, (1, 1, 0)), (None, 0, (1, 1, 0)),
    (None, 1150000000, (20, 9, 11)), (None, 1 << 25, (15, 8, 7)), (64, (1 << 32) - 4097, (22, 11, 11)),
    (None, 16 * 524288 + 1, (13, 7, 6)),
])
def test_geometry_table(avg, n, want):
    g = G.bucket_geom(n, avg)
    assert (g.T, g.DA, g.DB) == want
    assert g.tilesA == max(1, -(-n // 2048))
    r = G.resplit(g)
    assert (r.T, r.DA, r.DB) == (g.DA + 11, g.DA, 11)


def test_constants_restate_the_kernel_source():
    """A retune of the kernels fails here until the borders follow."""
    import anomod
    csrc = Path(anomod.__file__).resolve().parents[1] / "csrc"
    text = {f: (csrc / f).read_text() for f in ("bucket.hip", "group.hip")}
    for f, name, value in G.KERNEL_CONSTANTS:
        m = re.search(r"constexpr\s+(?:int|uint32_t)\s+(?:\w+\s*=\s*\w+\s*,\s*)?" + name +
                      r"\s*=\s*(\d+)\s*[;,]", text[f])
        assert m, (f, name)
        assert int(m.group(1)) == value, (f, name, m.group(1))
    b, g = text["bucket.hip"], text["group.hip"]
    for line in ("constexpr int kBTile = kBThreads * kBPer;", "constexpr int kPTile = kBThreads * kPPer;",
                 "constexpr uint64_t kEmptyKey = ~0ull;",
                 "constexpr int join_big_per(bool pack) { return pack ? 8 : 4; }",
                 "const bool pack = g.T >= 12 && ", 'env_int("ANOMOD_BUCKET_AVG", 1400)',
                 "avg = std::min(std::max(avg, 64), 2048);", "while (g.T < 2 * kDMax && ",
                 "g.DA = std::max(g.T - kDMax, std::min((g.T + 1) / 2, 9));"):
        assert line in b, line
    for line in ("constexpr int kSTile = kSThreads * kSPer;", "constexpr int kTTile = kTThreads * kTPer;",
                 "if (m > (uint64_t)kFixCap) {"):
        assert line in g, line
    assert G.kBTile == 1024 * 2 and G.kPTile == 1024 * 16
    assert G.SMALL_CAP == 512 * 4 == G.JOIN_CAP and G.BIG_CAP == 1024 * 8 == G.JOIN_BIG_PACKED
    assert G.JOIN_BIG_UNPACKED == 1024 * 4 and G.kSTile == 1024 * 4 and G.kTTile == 1024 * 16
    assert G.T_MAX == 2 * G.kDMax


def test_lsd_pass_model():
    """By hand: 300 keys -> two passes; three keys sharing 16 bits with 1024
    records stay there, 1025 take a third pass, and a fourth when they share
    24 bits as well; one key of 5000 records is no mixed bucket."""
    rng = np.random.default_rng(1)
    base = rng.integers(0, 2**64, 300, dtype=np.uint64)
    assert G.lsd_passes(base[:256]) == 1 and G.lsd_passes(base) == 2
    assert G.lsd_passes(np.zeros(0, np.uint64)) == 1

    def three(shared_bits, counts):
        top = np.uint64(0xABCDEF0123456789) & ~np.uint64((1 << (64 - shared_bits)) - 1)
        keys = [top | (np.uint64(i + 1) << np.uint64(64 - shared_bits - 3)) for i in range(3)]
        return np.r_[base, np.repeat(np.array(keys, np.uint64), counts)]

    assert G.lsd_passes(three(16, [1000, 20, 4])) == 2
    assert G.lsd_passes(three(16, [1000, 20, 5])) == 3
    assert G.lsd_passes(three(24, [1000, 20, 5])) == 4
    assert G.lsd_passes(np.r_[base, np.full(5000, base[0])]) == 2


def test_model_paths_by_hand():
    """predict_group / predict_join on sets whose answer is plain: one trace
    of 9000 spans escalates one level to two and takes the huge walk; 2049
    four-span traces sharing 40 key bits leave for the LSD path."""
    rng = np.random.default_rng(2)
    one = G.plan_set(rng, 12, 6, [(5, [9000], "random")], n=20000,
                     filler=[{"buckets": None, "n": None, "max_len": 8}])
    assert G.bucket_geom(20000).T == 4
    p = G.predict_group(one)
    assert (p["path"], p["levels"], p["bits"]) == ("bucket", 2, 15) and p["debug"][3:] == (9000, 1, 0)
    assert G.predict_join(one)["path"] == "bucket"
    many = G.plan_set(rng, 12, 6, [(5, [4] * 2049, ("share", 40, "rand"))], n=20000,
                      filler=[{"buckets": None, "n": None, "max_len": 8}])
    p = G.predict_group(many)
    assert p["path"] == "lsd" and p["debug"][5] == 1
    assert G.predict_group(many, force_lsd=True)["debug"] is None


@pytest.mark.parametrize("name", list(G.CASES))
def test_every_case_hits_its_border(name):
    """THE CAP.  The case's facts hold for the set it builds, its traces have
    distinct keys, and the path, levels and bits written beside it by hand
    are the model's."""
    case = G.CASES[name]
    flat, grouped = G.built(name)
    assert case.facts and case.facts[0][0] == "n"
    for fact in case.facts:
        G.check_fact(flat, fact)
    pg = G.predict_group(flat, case.avg, case.lsd)
    pj = G.predict_join(flat, case.avg, True, case.lsd)
    for want, got in ((case.group, pg), (case.join, pj)):
        if want is None:
            continue
        assert (got["path"], got["levels"]) == want[:2], got
        if want[2] is None:
            assert got["resplit"]  # the two-level re-split: bits follow the workspace
        else:
            assert got["bits"] == want[2] and not got["resplit"], got
    if name.startswith("A-"):  # one level, whatever n
        assert (pg["path"], pg["levels"], pj["path"], pj["levels"]) == ("bucket", 1, "join", 1)
    # the oracle grouping the GPU cases compare with is a grouping of this set
    assert grouped.n_spans == flat.n_spans
    assert grouped.n_traces == np.unique(flat.trace_hash).shape[0]


def test_cases_cover_the_issue_list():
    names = set(G.CASES)
    for n in G.A_SIZES:
        for avg in (None, 64):
            for mode in ("time", "reverse"):
                assert f"A-{n}-{avg}-{mode}" in names
    assert {7 * 2048 + 1, 8 * 2048, 9 * 2048 - 1, 17 * 2048 + 5} <= set(G.A_SIZES)
    for n in (524287, 524288, 524289):
        assert {f"B-{n}-None", f"B-{n}-64"} <= names
    for n in (4095, 4096, 4097, 16383, 16384, 16385):
        assert f"G-{n}" in names

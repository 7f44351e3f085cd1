"""GPU parity at the borders of the trace-grouping kernels (csrc/bucket.hip,
the grouping part of csrc/group.hip): span sets PLANNED onto a tile, scan or
bucket border (tests/group_ref.py: mix64 is a bijection, so a test chooses
every trace's bucket; tests/test_group_ref_host.py proves on the host that
every case hits its border).  Every case asserts

 (a) Context.group, downloaded, equals the oracle's stable grouping on all
     six columns and trace_ptr;
 (b) Context.edge_aggregate of the ungrouped set equals the C oracle's table
     on the oracle-grouped spans;
 (c) Context.group_info's path, levels and bits are the model's — a set that
     silently falls back to the LSD or the unfused path fails here;
 (d) the ANOMOD_BUCKET_DEBUG line's largest bucket, buckets over 2048 and
     buckets too big are the ones counted from the keys.

Every comparison is exact.  Where the two-level re-split (level B to 11 bits)
is what a case triggers, its bits follow the workspace's capacity, which the
model cannot know: those cases assert output, path and levels only."""
import functools
import re

import pytest

import group_ref as G
from oracle import native

from test_gpu_edge import assert_table_equal
from test_gpu_group import _assert_grouped_equal

pytestmark = pytest.mark.gpu

FULL = re.compile(r"bucket path: T=(\d+) DA=(\d+) DB=(\d+) max bucket (\d+), (\d+) over 2048, "
                  r"(\d+) too big")
ANY_MAX = re.compile(r"bucket path: .*max bucket (\d+)")


@functools.lru_cache(maxsize=3)
def _oracle_table(name):
    return native.edge_aggregate(G.built(name)[1])


def _names(prefix):
    return [n for n in G.CASES if n.startswith(prefix)]


def _check_info(info, pred, case_want):
    assert info["path"] == pred["path"] and info["levels"] == pred["levels"], (info, pred)
    if not pred["resplit"]:
        assert info["bits"] == pred["bits"], (info, pred)
    if case_want is not None:  # the literal written beside the case
        assert (info["path"], info["levels"]) == case_want[:2], (info, case_want)
        assert case_want[2] is None or info["bits"] == case_want[2], (info, case_want)


def _check_debug(err, pred, forced_lsd):
    if forced_lsd:
        assert "bucket path" not in err, err
        return
    assert ANY_MAX.search(err), err
    if pred["resplit"]:
        return
    if pred["path"] == "join":
        assert not FULL.search(err), err
        assert int(ANY_MAX.findall(err)[-1]) == pred["max_bucket"], (err, pred)
    else:
        assert tuple(int(x) for x in FULL.findall(err)[-1]) == pred["debug"], (err, pred)


def _run(ctx, capfd, monkeypatch, name, join_envs=({},)):
    """(a)-(d) for one case; the join once per environment of join_envs.
    Returns group_info after the grouping and after every join."""
    case = G.CASES[name]
    flat, want = G.built(name)
    for k, v in case.env().items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ANOMOD_BUCKET_DEBUG", "1")
    dev = ctx.upload_ungrouped(flat)
    assert not dev.grouped
    capfd.readouterr()
    g = ctx.group(dev)
    ginfo = ctx.group_info()
    err = capfd.readouterr().err
    assert g.grouped
    _assert_grouped_equal(g.download(), want)                       # (a)
    g.free()
    pred = G.predict_group(flat, case.avg, case.lsd)
    _check_info(ginfo, pred, case.group)                            # (c)
    _check_debug(err, pred, case.lsd)                               # (d)
    ref = _oracle_table(name)
    infos = []
    for env in join_envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        table = ctx.edge_aggregate(dev)
        info = ctx.group_info()
        err = capfd.readouterr().err
        assert_table_equal(table, ref)                              # (b)
        pack = env.get("ANOMOD_JOIN_PACK", "1") != "0"
        pred = G.predict_join(flat, case.avg, pack, case.lsd)
        _check_info(info, pred, case.join if pack else None)        # (c)
        _check_debug(err, pred, case.lsd)                           # (d)
        infos.append(info)
    dev.free()
    return [ginfo] + infos


@pytest.mark.parametrize("name", _names("A-"))
def test_level_a_tiles(ctx, capfd, monkeypatch, name):
    """A. One level; n on the wave rows (63..129), a partial first tile,
    exact tiles, fewer than 8 tiles and a remainder of xcd_tile's eighths;
    default mean and 64; arrival orders 'time' and 'reverse'."""
    _, info = _run(ctx, capfd, monkeypatch, name)
    assert info["path"] == "join" and info["levels"] == 1


@pytest.mark.parametrize("name", _names("B-5"))
def test_scan_blocks(ctx, capfd, monkeypatch, name):
    """B. 256 / 257 level-A tiles (one scan block / two); at a mean of 64 two
    levels with 8192 buckets, two partial sums of the trace-count scan."""
    _, info = _run(ctx, capfd, monkeypatch, name)
    assert info["path"] == "join"


def test_scan_17_blocks(ctx, capfd, monkeypatch):
    """B. n = 16 * 524288 + 1 short traces: 4097 level-A tiles, 17 scan
    blocks, the second batch of 16 loads in bk_scan_top_kernel."""
    _, info = _run(ctx, capfd, monkeypatch, "B-17-blocks")
    assert info == {"path": "join", "levels": 2, "bits": 13}
    G.built.cache_clear()
    _oracle_table.cache_clear()


@pytest.mark.parametrize("name", _names("C-"))
def test_two_digits_per_thread(ctx, capfd, monkeypatch, name):
    """C. T = DA = 11, nd = 2048: every thread of the digit scans holds two
    digits.  Traces in the first and last buckets and either side of the
    1023 | 1024 pair border, long runs of empty buckets; the second set's
    empty run crosses that border (the two cannot hold in one set)."""
    _, info = _run(ctx, capfd, monkeypatch, name)
    assert info == {"path": "join", "levels": 1, "bits": 11}


JOIN_ENVS = [{"ANOMOD_BK_STABLE_B": s, "ANOMOD_JOIN_RECB": r, "ANOMOD_JOIN_PACK": p}
             for s in "01" for r in "01" for p in "10"]


@pytest.mark.parametrize("name", _names("D-"))
def test_level_b_tiles(ctx, capfd, monkeypatch, name):
    """D. Level-A buckets of exactly 0, 1, 16383, 16384, 16385 spans (the
    first or the last one empty), and one of 16 * 16384 + 1 spans: 17 level-B
    tiles, the second batch of bk_scan_seg_kernel — once with repeated
    (trace, id) pairs whose copies lie in different level-B tiles and carry
    different services.  The join under every ANOMOD_BK_STABLE_B x
    ANOMOD_JOIN_RECB x ANOMOD_JOIN_PACK; unpacked, the 17-tile bucket's final
    buckets of 4097 spans exceed the join's 4096 and the model says so."""
    infos = _run(ctx, capfd, monkeypatch, name, JOIN_ENVS)
    assert infos[0]["path"] == "bucket" and infos[0]["levels"] == 2
    for env, info in zip(JOIN_ENVS, infos[1:]):
        if env["ANOMOD_JOIN_PACK"] == "1":
            assert info["path"] == "join" and info["levels"] == 2, (env, info)


@pytest.mark.parametrize("name", _names("E-"))
def test_bucket_caps(ctx, capfd, monkeypatch, name):
    """E. Buckets of exactly 2047 / 2048 / 2049 and 8191 / 8192 spans; 8193
    spans (several traces sharing 40 key bits, one trace, 2048 and 2049
    distinct keys): the one-level escalation and the huge walk, or the LSD
    path; k = 2^64 - 1 (the huge table's empty mark) inside a huge bucket and
    an ordinary one; k = 0; mixed sub-buckets (T + 9 shared bits) and equal
    pair keys (T + 32) in buckets of 2048 and 6000 spans."""
    ginfo, _ = _run(ctx, capfd, monkeypatch, name)
    assert ginfo["path"] == ("lsd" if name in ("E-huge-2049-keys", "E-ones-in-huge") else "bucket")


@pytest.mark.parametrize("name", _names("F-"))
def test_join_caps(ctx, capfd, monkeypatch, name):
    """F. The join's 2048 / 2049 spans (small kernel -> big list) and its big
    kernel's 4096 (unpacked, T < 12) and 8192 (packed, S = 12 and 46) spans:
    the join; 4097 and 8193: the unfused path, the oracle's table all the
    same."""
    _, info = _run(ctx, capfd, monkeypatch, name)
    if name in ("F-unpacked-4097", "F-packed-8193"):
        assert info["path"] != "join"
    else:
        assert info["path"] == "join"


@pytest.mark.parametrize("name", _names("G-"))
def test_lsd_tiles_and_mixed_buckets(ctx, capfd, monkeypatch, name):
    """G. ANOMOD_GROUP_PATH=lsd at its 4096-record radix tiles and 16384-span
    scan tiles; at two passes, traces sharing their top 16 key bits with 1024
    records in all are sorted by one wave, 1025 force a third pass (the rule
    group.hip documents: 'a mixed bucket larger than the wave's LDS reruns
    the sort with P + 1', m > kFixCap)."""
    _, info = _run(ctx, capfd, monkeypatch, name)
    assert info["path"] == "lsd"
    assert info["levels"] == (3 if name == "G-mixed-1025" else 2)

"""The conditions under which test_frame_edges_gpu.py's frames mean something,
asserted with the oracle alone (no GPU), the depth goldens of the unmodified
reference (tests/golden/depths.json), and mirt_frame_desc's limits through
mirt_shard_rows.

Shares of pixels, measured when the tests were written (asserted bounds in
brackets). S1 160x90, seed 3, pixels differing between depth d - 1 and d for
d = 1..8: 14400, 9277, 2983, 1480, 899, 634, 480, 366 [>= 144, 1 %]. S2
96x54: at least 99 % at every d [>= 99 %]. Seed 5 against 5 + 2^32 and sample
0 against 0xFFFFFFFF on S1 at depth 5: 64 % each [>= 25 %].
"""
import json
import os

import numpy as np
import pytest

import frame_edge_cases as E
from conftest import GOLDEN, sha

mirt = E.mirt


def _differ(a, b):
    return int((a != b).any(axis=-1).sum())


@pytest.mark.parametrize("name,share", [("S1", 0.01), ("S2", 0.99)])
def test_every_level_changes_the_frame(oracle, name, share):
    """A pixel that differs between the depth d - 1 and the depth d frame had a
    chain that hit something at level d - 1: enough of them at every d that a
    walk cut short at any level shows."""
    w, h = E.scene(name).size
    frames = [E.depth_ref(oracle, name, d) for d in E.DEPTHS]
    counts = [_differ(frames[d - 1], frames[d]) for d in E.DEPTHS[1:]]
    print(name, f"{w}x{h}", "pixels differing between depth d-1 and d, d = 1..8:", counts)
    assert len(counts) == 8
    for d, c in zip(E.DEPTHS[1:], counts):
        assert c >= share * w * h, (name, d, c)


def test_rng_words_change_the_frame(oracle):
    """The seed's high word and the sample's wrap-around are visible: seed s
    against s + 2^32, and sample 0 against 0xFFFFFFFF, each change at least a
    quarter of S1's depth-5 pixels."""
    w, h = E.scene("S1").size
    lo, hi = E.depth_ref(oracle, "S1", 5, seed=5), E.depth_ref(oracle, "S1", 5, seed=5 + 2**32)
    first, last = E.depth_ref(oracle, "S1", 5), E.depth_ref(oracle, "S1", 5, sample=0xFFFFFFFF)
    print("seed 5 vs 5 + 2^32:", _differ(lo, hi), "sample 0 vs 0xFFFFFFFF:", _differ(first, last), "of", w * h)
    assert _differ(lo, hi) >= 0.25 * w * h
    assert _differ(first, last) >= 0.25 * w * h


def test_sample_wraps_modulo_2_32(oracle):
    """oracle_frame's rule for `samples` frames from sample 0xFFFFFFFE: frames
    2 and 3 are RNG samples 0 and 1."""
    tree, spheres = E.oracle_scene(oracle, "S1")
    cam = E.camera("default")
    acc = np.zeros(160 * 90 * 3, np.float32)
    want = None
    for j, smp in enumerate((0xFFFFFFFE, 0xFFFFFFFF, 0, 1)):
        col = E.depth_ref(oracle, "S1", 5, sample=smp)
        want = oracle.accumulate(col, acc, j == 0, j + 1).reshape(90, 160, 4)
    got = E.depth_ref(oracle, "S1", 5, sample=0xFFFFFFFE, samples=4)
    assert (got == want).all()
    # and a one-sample fresh descriptor is the oracle's frame itself
    one = oracle.render(cam, 160, 90, spheres, tree, depth=5, mode=1, seed=3, sample=0xFFFFFFFF)
    assert (one == E.depth_ref(oracle, "S1", 5, sample=0xFFFFFFFF)).all()


def test_tiny_frames_cover_the_hit_counts(oracle):
    """Among the tiny frames: one without a camera hit, one with fewer hits
    than the bounce queue has segments (1..7), one with fewer than a wave
    (8..63), and one in which every pixel is a hit."""
    tree, spheres = E.oracle_scene(oracle, "S1")
    hits = {}
    for cam in E.TINY_CAMERAS:
        for w, h in E.TINY_SIZES:
            rays = oracle.camera_rays(E.camera(cam), w, h).reshape(-1)
            hits[cam, w, h] = int(oracle.intersect(tree, spheres, rays)["hit"].sum())
    print("camera hits of the tiny frames:", hits)
    assert any(n == 0 for n in hits.values())
    assert any(1 <= n <= 7 for n in hits.values())
    assert any(8 <= n <= 63 for n in hits.values())
    assert any(n == w * h for (_, w, h), n in hits.items())
    assert hits["closeup", 1, 1] == 1 and hits["default", 1, 1] == 0


def test_ragged_frames_hit_at_their_edges(oracle):
    """From the origin of either scene every camera ray of the ragged sizes is
    a hit, those of the last tile column and row included; under the default
    camera the first and the last column of those sizes are sky."""
    cam, w, h = E.FULL_AFTER
    for name, sizes in (("S1", [(w, h)]), ("S2", E.RAGGED_SIZES)):
        tree, spheres = E.oracle_scene(oracle, name)
        for w, h in sizes:
            assert w % 8 and h % 8 and (w % 4 or h % 4), (w, h)   # ragged in both directions for the 8x8 tiles
            rays = oracle.camera_rays(E.camera(cam), w, h).reshape(-1)
            assert oracle.intersect(tree, spheres, rays)["hit"].all(), (name, w, h)
    tree, spheres = E.oracle_scene(oracle, "S1")
    for w, h in E.RAGGED_SIZES:
        rays = oracle.camera_rays(E.camera("default"), w, h)
        hit = oracle.intersect(tree, spheres, rays.reshape(-1))["hit"].reshape(h, w)
        assert hit.any() and not hit[:, 0].any() and not hit[:, -1].any(), (w, h)


def test_sky_camera_has_no_hits(oracle):
    """The all-sky camera: no camera ray of either size meets a sphere, and
    the depth-1 frame is the depth-5 and depth-8 frame."""
    tree, spheres = E.oracle_scene(oracle, "S1")
    for w, h in E.SKY_SIZES:
        rays = oracle.camera_rays(E.camera("sky"), w, h).reshape(-1)
        assert int(oracle.intersect(tree, spheres, rays)["hit"].sum()) == 0
        one = E.ref(oracle, "S1", "sky", w, h, depth=1)
        for d in E.SKY_DEPTHS:
            assert (E.ref(oracle, "S1", "sky", w, h, depth=d) == one).all()


def test_oracle_reproduces_the_reference_depths(oracle):
    """depths.json (the unmodified reference at depth 0..8, both seeds, S2 at
    6 and 8, brute force at 4 and 8): the oracle's frames have the same
    SHA-256, so the GPU tests' oracle frames stand for the reference's."""
    with open(os.path.join(GOLDEN, "depths.json")) as f:
        gold = json.load(f)
    assert sorted(gold["frames"]) == sorted(E.GOLDEN) and tuple(gold["size"]) == E.GOLDEN_SIZE
    for key, (name, kw) in E.GOLDEN.items():
        img = E.ref(oracle, name, E.scene(name).cam, *E.GOLDEN_SIZE, **kw)
        assert sha(img) == gold["frames"][key], key


def _rows(**kw):
    kw.setdefault("width", 40)
    kw.setdefault("height", 9)
    return mirt.shard_rows(mirt.frame_desc(**kw))


def test_descriptor_limits():
    """frame_desc_valid through mirt_shard_rows: the last accepted value of
    each axis, and the first rejected one."""
    assert len(_rows(depth=8)) == 9
    assert len(_rows(samples=64)) == 9
    assert list(_rows(width=1)) == list(range(9))
    assert list(_rows(width=1, height=1)) == [0]
    assert list(_rows(seed=2**64 - 1, sample=2**32 - 1)) == list(range(9))
    for bad in (dict(depth=9), dict(depth=-1), dict(samples=65), dict(width=0), dict(height=0),
                dict(lead_skip=1), dict(lead_skip=8, num_shards=2), dict(shard=3, num_shards=3)):
        with pytest.raises(mirt.MirtError):
            _rows(**bad)


def test_empty_shards_are_valid():
    """More shards than row blocks: the shards beyond them are valid and have
    0 rows, and the shards together still hold every row once."""
    for kw, nrows in E.EMPTY_SHARDS:
        assert len(mirt.shard_rows(E.desc(**kw))) == nrows, kw
    for n, d, w, h, rb, empty in E.EMPTY_MULTI:
        rows = [mirt.shard_rows(mirt.frame_desc(w, h, row_block=rb, shard=s, num_shards=n, lead_skip=d))
                for s in range(n)]
        assert [s for s in range(n) if len(rows[s]) == 0] == empty
        assert sorted(np.concatenate(rows).tolist()) == list(range(h))

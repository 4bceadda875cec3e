"""The bounce lane loop confirms a walk's closest hit once (MIRT_OPT_CONFIRM_ONCE,
trace.h wide_leaf_once): frames with the option on, off and under forced
confirmation failures (MIRT_OPT_DEBUG_FAIL_CONFIRM) equal the oracle's byte
for byte.

Every frame here runs with MIRT_OPT_BOUNCE_BLOCKS = 1: one workgroup takes
every bounce ray, so its four waves refill many times, cross the shading
threshold, and enter the quad drain and the solo chain holding tentative
state.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (67, 45)]          # a ragged one: neither a multiple of 8 nor of 4
DEPTHS = [2, 3, 5, 8]
SCENES = [("render", 200), ("render", 2000), ("bench", 200), ("bench", 2000)]

_scenes = {}   # key -> (spheres as built, Bvh, oracle spheres, oracle tree, cameras)
_refs = {}     # (key, W, H, depth, cam) -> the oracle's frame


def _cameras(mirt, spheres):
    """The default camera, and one inside the cloud (at the mean centre)."""
    inside = mirt.default_camera()
    c = spheres["center"].astype(np.float64).mean(axis=0)
    inside.position = mirt.abi.Vec3(float(c[0]), float(c[1]), float(c[2]))
    return [mirt.default_camera(), inside]


def _install(key, mirt, oracle, spheres):
    if key not in _scenes:
        s2 = spheres.copy()
        b = mirt.build_bvh(spheres)
        t = oracle.build(s2)
        _scenes[key] = (spheres, b, s2, t, _cameras(mirt, spheres))
    return _scenes[key]


def _generated(mirt, oracle, kind, n):
    s = mirt.create_random_spheres(n, 1) if kind == "render" else mirt.create_benchmark_spheres(n, 1)
    return _install((kind, n), mirt, oracle, s)


def _pairs(mirt, oracle, shift):
    """100 spheres, each twice with different colours; shift: the copy's
    centre moved that many floats along x."""
    key = ("pairs", shift)
    if key in _scenes:
        return _scenes[key]
    a = mirt.create_random_spheres(100, 3)
    b = a.copy()
    b["color"][:, :3] = 255 - a["color"][:, :3]
    x = b["center"][:, 0].copy()
    for _ in range(shift):
        x = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
    b["center"][:, 0] = x
    s = np.ascontiguousarray(np.concatenate([a, b]))
    return _install(key, mirt, oracle, s)


def _ref(oracle, key, W, H, depth, ci):
    k = (key, W, H, depth, ci)
    if k not in _refs:
        _, _, s2, t, cams = _scenes[key]
        _refs[k] = oracle.render(cams[ci], W, H, s2, t, depth=depth, mode=1, seed=1)
    return _refs[k]


def _check(gpu, mirt, oracle, key, settings, depths=DEPTHS):
    """Every size x depth x camera of scene `key` under each (confirm_once,
    fail_n) setting against the oracle's frame."""
    abi = mirt.abi
    s, b, _, _, cams = _scenes[key]
    gpu.upload(s, b)
    try:
        gpu.set_option(abi.OPT_BOUNCE_BLOCKS, 1)
        for once, fail in settings:
            gpu.set_option(abi.OPT_CONFIRM_ONCE, once)
            gpu.set_option(abi.OPT_DEBUG_FAIL_CONFIRM, fail)
            assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == once
            assert gpu.get_option(abi.OPT_DEBUG_FAIL_CONFIRM) == fail
            for W, H in SIZES:
                for depth in depths:
                    for ci, cam in enumerate(cams):
                        img = gpu.render_frame(cam, W, H, depth=depth, seed=1)
                        ref = _ref(oracle, key, W, H, depth, ci)
                        bad = int((img != ref).any(axis=-1).sum())
                        assert bad == 0, (key, once, fail, W, H, depth, ci, bad)
    finally:
        gpu.set_option(abi.OPT_BOUNCE_BLOCKS, 0)
        gpu.set_option(abi.OPT_CONFIRM_ONCE, 2)   # the library default: by tree size
        gpu.set_option(abi.OPT_DEBUG_FAIL_CONFIRM, 0)


@pytest.mark.parametrize("kind,n", SCENES)
def test_option_on_equals_off_equals_oracle(gpu, mirt, oracle, kind, n):
    _generated(mirt, oracle, kind, n)
    _check(gpu, mirt, oracle, (kind, n), [(1, 0), (0, 0)])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("fail", [1, 2, 7])
def test_forced_confirmation_failures(gpu, mirt, oracle, fail):
    """The confirmation of every chain whose pixel index is a multiple of
    `fail` reports failure although the box passed: those levels are walked
    again in exact mode, and the frames stay the oracle's. With 1 every hit
    of the lane loop walks its level twice -- and no more than twice: an
    exact-mode walk confirms nothing afterwards, so the frames take their
    ordinary time. The bound: a level walked at most twice is at most twice
    the device work, so the forced run of the same 64 frames (oracle frames
    cached by then) may take 3x the unforced run plus 2 s of slack for the
    host's share -- seconds, where an unbounded re-walk never ends."""
    unforced = forced = 0.0
    for kind, n in SCENES:
        _generated(mirt, oracle, kind, n)
        _check(gpu, mirt, oracle, (kind, n), [(1, 0)])      # fills the oracle cache, warms the scene
        t0 = time.perf_counter()
        _check(gpu, mirt, oracle, (kind, n), [(1, 0)])
        t1 = time.perf_counter()
        _check(gpu, mirt, oracle, (kind, n), [(1, fail)])
        t2 = time.perf_counter()
        unforced += t1 - t0
        forced += t2 - t1
    print(f"fail {fail}: unforced {unforced:.3f} s, forced {forced:.3f} s")
    assert forced <= 3.0 * unforced + 2.0


@pytest.mark.parametrize("shift", [0, 1])
def test_ties_and_near_ties(gpu, mirt, oracle, shift):
    """shift 0: every sphere twice, so every hit is an exact tie of t, which
    the larger sphere index wins at every level (the deferred gate reads the
    two leaves' sphere indices). shift 1: the copy one float along x, so the
    pair's t differ by about an ulp."""
    _pairs(mirt, oracle, shift)
    _check(gpu, mirt, oracle, ("pairs", shift), [(1, 0), (0, 0), (1, 2)])


def test_default_follows_the_tree_size(gpu, mirt, oracle):
    """MIRT_OPT_CONFIRM_ONCE 2 (the default) is 1 up to 32,768 leaves and 0
    above; on a tree above the line, 0, 1 and 2 give the oracle's frame."""
    abi = mirt.abi
    s, b, _, _, _ = _generated(mirt, oracle, "render", 2000)
    gpu.upload(s, b)
    assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == 1
    big = mirt.create_random_spheres(40000, 1)
    big2 = big.copy()
    bb = mirt.build_bvh(big)
    t = oracle.build(big2)
    cam = mirt.default_camera()
    ref = oracle.render(cam, 64, 48, big2, t, depth=5, mode=1, seed=1)
    oracle.free(t)
    gpu.upload(big, bb)
    try:
        assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == 0
        for mode, in_effect in ((2, 0), (1, 1), (0, 0)):
            gpu.set_option(abi.OPT_CONFIRM_ONCE, mode)
            assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == in_effect
            assert (gpu.render_frame(cam, 64, 48, depth=5, seed=1) == ref).all(), mode
        with pytest.raises(mirt.MirtError):
            gpu.set_option(abi.OPT_CONFIRM_ONCE, 3)
    finally:
        gpu.set_option(abi.OPT_CONFIRM_ONCE, 2)


# Seed 1 of create_random_spheres(2000): chosen on the CPU alone -- the
# oracle's BVH frame and its brute-force frame of this scene agree pixel for
# pixel (asserted below), so no closest hit's exact box fails hit.c's test and
# a correct deferred walk has nothing to walk again.
REWALK_SEED = 1


def test_unforced_rewalks_are_rare(gpu, mirt, oracle):
    """One 160x90, 2,000-sphere frame through the instrumented bounce kernel:
    at most 1 unforced re-walk in 1,000 confirmed hits (a condition, not a
    measurement: on this scene the reference has no winner whose box fails)."""
    abi = mirt.abi
    s = mirt.create_random_spheres(2000, REWALK_SEED)
    s2 = s.copy()
    b = mirt.build_bvh(s)
    t = oracle.build(s2)
    cam = mirt.default_camera()
    with_bvh = oracle.render(cam, 160, 90, s2, t, depth=5, mode=1, seed=1)
    brute = oracle.render(cam, 160, 90, s2, None, depth=5, use_bvh=False, mode=1, seed=1)
    oracle.free(t)
    assert (with_bvh == brute).all()
    gpu.upload(s, b)
    try:
        gpu.set_option(abi.OPT_BOUNCE_BLOCKS, 1)
        d = gpu.bounce_stats(cam, 160, 90, depth=5, seed=1)
        img = gpu.render_frame(cam, 160, 90, depth=5, seed=1)
        # the test hook does what the forced-failure tests rely on: every
        # confirmation fails, and each failure is walked again just once
        gpu.set_option(abi.OPT_DEBUG_FAIL_CONFIRM, 1)
        f = gpu.bounce_stats(cam, 160, 90, depth=5, seed=1)
    finally:
        gpu.set_option(abi.OPT_DEBUG_FAIL_CONFIRM, 0)
        gpu.set_option(abi.OPT_BOUNCE_BLOCKS, 0)
    assert int(f[:, 20].sum()) == int(f[:, 21].sum()) > 1000
    assert (img == with_bvh).all()
    confirmed, failed, restarted = int(d[:, 20].sum()), int(d[:, 21].sum()), int(d[:, 22].sum())
    print(f"confirmed {confirmed}, failed {failed}, fallback restarts {restarted}")
    assert confirmed > 1000
    assert 1000 * (failed + restarted) <= confirmed

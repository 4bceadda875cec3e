"""The four-wide walks' stack-overflow fallbacks (trace.h: wide_lane_step's DFS
segment, the deferred walk's restart, quad_step's segment in the bounce
kernel's drain and in intersect_quad_kernel) on trees that overflow the
20-entry lane stack: every frame and every hit record equals the oracle's
byte for byte, and mirt_bounce_stats shows that the fallbacks ran.

The trees are wide_stack_cases.py's (test_wide_stack_host.py shows on the CPU
that they overflow and that their frames are not vacuous); the oracle renders
them through Oracle.tree_from_flat. The lane-loop frames run with
MIRT_OPT_BOUNCE_BLOCKS = 1, so that one workgroup takes every chain.
"""
import contextlib

import numpy as np
import pytest
import torch

import wide_stack_cases as W

pytestmark = pytest.mark.gpu

NAMES = list(W.CASES)
abi = W.abi
DEFAULTS = {abi.OPT_TRAVERSAL: abi.TRAV_WAVEFRONT, abi.OPT_BOUNCE_THRESHOLD: 20, abi.OPT_PRUNE: 1,
            abi.OPT_BOUNCE_BLOCKS: 0, abi.OPT_QUAD_DRAIN: 1, abi.OPT_LEAF_BATCH: 2, abi.OPT_QUAD_BATCH: 1,
            abi.OPT_CONFIRM_ONCE: 2}
SEGMENT_STEPS, FALLBACKS, DRAIN_ITERATIONS, RESTARTS = 10, 11, 8, 22   # mirt_bounce_stats columns

_trees = {}   # name -> the oracle's pointer tree of the padded flat tree
_refs = {}    # (name, W, H, depth) -> the oracle's frame


@contextlib.contextmanager
def options(gpu, values):
    """The library's defaults with `values` on top; the defaults again afterwards."""
    try:
        for opt, v in {**DEFAULTS, **values}.items():
            gpu.set_option(opt, v)
        yield
    finally:
        for opt, v in DEFAULTS.items():
            gpu.set_option(opt, v)


def _tree(oracle, name):
    if name not in _trees:
        _trees[name] = oracle.tree_from_flat(W.case(name).nodes)
    return _trees[name]


def _ref(oracle, name, width, height, depth):
    key = (name, width, height, depth)
    if key not in _refs:
        c = W.case(name)
        _refs[key] = oracle.render(c.cam, width, height, c.spheres, _tree(oracle, name), depth=depth, mode=1, seed=1)
    return _refs[key]


def _upload(gpu, mirt, name):
    c = W.case(name)
    gpu.upload(c.spheres, mirt.Bvh(c.nodes))
    return c


def _frames(gpu, oracle, name, label, sizes=W.SIZES, depths=W.DEPTHS):
    """The frames of the uploaded case under the options in force, against the oracle's."""
    c = W.case(name)
    for width, height in sizes:
        for depth in depths:
            img = gpu.render_frame(c.cam, width, height, depth=depth, seed=1)
            bad = int((img != _ref(oracle, name, width, height, depth)).any(axis=-1).sum())
            assert bad == 0, (name, label, width, height, depth, bad)


def _stats(gpu, name, *columns, lane_loop_only=False):
    """Columns of mirt_bounce_stats for the 160x90 depth-5 frame, summed over
    the waves. lane_loop_only: with the drain off, so that every chain ends
    in the lane loop, whose fallbacks the columns count -- which chains a
    wave's last lanes hand to the drain depends on timing, and a tree that
    overflows a few times a frame could else show none."""
    c = W.case(name)
    if lane_loop_only:
        gpu.set_option(abi.OPT_QUAD_DRAIN, 0)   # (the caller's options() restores it)
    d = gpu.bounce_stats(c.cam, 160, 90, depth=5, seed=1)
    return [int(d[:, col].sum()) for col in columns]


@pytest.mark.parametrize("name", NAMES)
def test_lane_loop_exact_gates(gpu, mirt, oracle, name):
    """MIRT_OPT_CONFIRM_ONCE 0: an overflowing step walks the node's flat
    segment with lane_step and skips its own leaf slots."""
    c = _upload(gpu, mirt, name)
    with options(gpu, {abi.OPT_BOUNCE_BLOCKS: 1, abi.OPT_CONFIRM_ONCE: 0, abi.OPT_LEAF_BATCH: 0}):
        assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == 0 and gpu.get_option(abi.OPT_LEAF_BATCH) == 0
        _frames(gpu, oracle, name, "exact gates")
        entered, steps, restarts = _stats(gpu, name, FALLBACKS, SEGMENT_STEPS, RESTARTS, lane_loop_only=True)
        _frames(gpu, oracle, name, "exact gates, no drain", sizes=[(160, 90)], depths=[5])   # the frame just counted
    print(f"{name}: {entered} fallbacks entered, {steps} lane-steps in segments")
    assert restarts == 0
    if c.overflows:
        assert entered > 0 and steps > 0
    else:
        assert entered == 0 and steps == 0


@pytest.mark.parametrize("name", NAMES)
def test_lane_loop_deferred(gpu, mirt, oracle, name):
    """MIRT_OPT_CONFIRM_ONCE 1: a deferred walk that would overflow starts the
    level again in exact mode -- where it overflows again and takes the
    segment. 0, 1 and 2 (by tree size: 1 here) give one and the same frame."""
    c = _upload(gpu, mirt, name)
    with options(gpu, {abi.OPT_BOUNCE_BLOCKS: 1, abi.OPT_CONFIRM_ONCE: 1, abi.OPT_LEAF_BATCH: 0}):
        assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == 1
        _frames(gpu, oracle, name, "deferred")
        restarts, entered = _stats(gpu, name, RESTARTS, FALLBACKS, lane_loop_only=True)
        _frames(gpu, oracle, name, "deferred, no drain", sizes=[(160, 90)], depths=[5])   # the frame just counted
        gpu.set_option(abi.OPT_QUAD_DRAIN, 1)
        imgs = []
        for mode in (0, 1, 2):
            gpu.set_option(abi.OPT_CONFIRM_ONCE, mode)
            imgs.append(gpu.render_frame(c.cam, 160, 90, depth=5, seed=1))
        assert gpu.get_option(abi.OPT_CONFIRM_ONCE) == 1
    print(f"{name}: {restarts} restarts, {entered} fallbacks entered")
    assert (imgs[0] == imgs[1]).all() and (imgs[1] == imgs[2]).all()
    if c.overflows:
        assert restarts > 0 and entered > 0
    else:
        assert restarts == 0 and entered == 0


@pytest.mark.parametrize("name", NAMES)
def test_leaf_batch_walk(gpu, mirt, oracle, name):
    """MIRT_OPT_LEAF_BATCH 1 (bounce_kernel<true, 4>): the batched gates are
    skipped by an overflowing step like the others."""
    _upload(gpu, mirt, name)
    with options(gpu, {abi.OPT_BOUNCE_BLOCKS: 1, abi.OPT_LEAF_BATCH: 1}):
        assert gpu.get_option(abi.OPT_LEAF_BATCH) == 1
        _frames(gpu, oracle, name, "leaf batch")


@pytest.mark.parametrize("name", NAMES)
def test_quad_drain(gpu, mirt, oracle, name):
    """The drain on and off, entered early (threshold 56) and late (8), with
    one workgroup and with the default grid (many sparse waves: most chains
    end in the drain, the last ray of each wave in the solo walk). Every
    complete walk on these trees overflows (the model), so a level begun in
    the drain takes quad_step's segment."""
    _upload(gpu, mirt, name)
    for blocks in (1, 0):
        for drain in (1, 0):
            for threshold in (8, 56):
                with options(gpu, {abi.OPT_BOUNCE_BLOCKS: blocks, abi.OPT_QUAD_DRAIN: drain,
                                   abi.OPT_BOUNCE_THRESHOLD: threshold}):
                    _frames(gpu, oracle, name, ("drain", blocks, drain, threshold), depths=[5])
                    (iterations,) = _stats(gpu, name, DRAIN_ITERATIONS)
                if drain:
                    assert iterations > 0, (name, blocks, threshold)
                else:
                    assert iterations == 0, (name, blocks, threshold)


@pytest.mark.parametrize("name", NAMES)
def test_tile_schedule_and_trace_rays(gpu, mirt, oracle, name):
    """MIRT_TRAV_TILE and mirt_trace_rays: closest_hit's per-lane four-wide
    walk (exact gates, no deferral) for camera and bounce rays alike."""
    c = _upload(gpu, mirt, name)
    rays = W.inside_rays(name)
    want = oracle.trace_rays(rays, c.spheres, _tree(oracle, name), depth=5, mode=1, seed=3)
    with options(gpu, {abi.OPT_TRAVERSAL: abi.TRAV_TILE}):
        _frames(gpu, oracle, name, "tile", depths=[5])
        got = gpu.trace_ray(rays, depth=5, seed=3)
    assert (got == want).all(), (name, int((got != want).any(axis=-1).sum()))


_hits = {}   # (name, n) -> (rays, the oracle's hit records)


def _inside_hits(oracle, name, n):
    if (name, n) not in _hits:
        c = W.case(name)
        rays = W.inside_rays(name, n)
        _hits[name, n] = (rays, oracle.intersect_flat(c.nodes, c.spheres, rays))
    return _hits[name, n]


def _same_hits(got, want, label):
    g = got.view(np.uint8).reshape(len(got), -1)
    w = want.view(np.uint8).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, f"{label}: {len(bad)} of {len(got)} rays differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("name", NAMES)
def test_per_ray_entry_points(gpu, mirt, oracle, name):
    """mirt_intersect_rays / mirt_any_hit_rays from origins inside the box:
    a small batch one ray per quad (intersect_quad_kernel's quad_step), the
    same batch one ray per lane, and a batch past the quad kernel's limit of
    256 rays per CU -- hit, t, sphere, normal and point against hit.c over
    the flat tree, with pruning and without."""
    _upload(gpu, mirt, name)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    small = _inside_hits(oracle, name, 3000)
    large = _inside_hits(oracle, name, 256 * cus + 1500)
    assert len(small[0]) <= 256 * cus < len(large[0])
    for prune in (1, 0):
        for label, quad, (rays, want) in (("quad batch", 1, small), ("per lane", 0, small), ("large batch", 1, large)):
            with options(gpu, {abi.OPT_PRUNE: prune, abi.OPT_QUAD_BATCH: quad}):
                _same_hits(gpu.closest_hit(rays), want, (name, label, prune))
                assert (gpu.any_hit(rays, use_bvh=True) == want["hit"]).all(), (name, label, prune)


@pytest.mark.parametrize("name", ["graft6", "far14"])
def test_device_layout_of_an_overflowing_tree(gpu, mirt, oracle, name):
    """mirt_scene_upload_flat_device: the layouts derived on the device (HAux's
    flat and end among them) give the host upload's frame."""
    c = _upload(gpu, mirt, name)
    with options(gpu, {abi.OPT_BOUNCE_BLOCKS: 1, abi.OPT_CONFIRM_ONCE: 0}):
        host = gpu.render_frame(c.cam, 160, 90, depth=5, seed=1)
        gpu.upload_device(c.spheres, c.nodes)
        dev = gpu.render_frame(c.cam, 160, 90, depth=5, seed=1)
        (entered,) = _stats(gpu, name, FALLBACKS, lane_loop_only=True)
    assert (dev == host).all()
    assert (dev == _ref(oracle, name, 160, 90, 5)).all()
    assert entered > 0

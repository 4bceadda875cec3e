"""mirt_bvh_overlay against the oracle's restatement, byte for byte, on the
cases of tests/overlay_cases.py (tests/test_overlay_edges_host.py shows they
are not vacuous): cameras inside the tree, looking away, skewed and
non-finite, frames down to 1 x 1, every level value around a tree's depth,
trees of no builder and trees deeper than the one-byte resident depth, scenes
after refit, update and rebuild, the frame slab the overlay shares with frames,
and the arguments.

Why the raster loop ends and stays in bounds whatever the camera holds
(csrc/render.hip overlay_lines_kernel): both endpoints passed the integer
range test [-W, 2W] x [-H, 2H] with W, H <= 2^30, so Bresenham runs at most
3 max(W, H) + 2 steps, and a pixel is written only after the on-screen test.
A NaN or out-of-range coordinate converts to INT_MIN and fails the range
test. overlay_depth's descent moves a node index forward and stops at the
node it looks for."""
import ctypes as C

import numpy as np
import pytest

import overlay_cases as oc
from test_update_device import host_update, moved

pytestmark = pytest.mark.gpu

BIG = (160, 90)
E_INVALID, E_NOSCENE = -1, -3


def upload(r, mirt, name):
    s, _, nodes = oc.scene(name)
    r.upload(s, mirt.Bvh(nodes) if len(nodes) else None)


def same(got, want, what):
    assert got.shape == want.shape, what
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = " \
                          f"{tuple(int(v) for v in np.argwhere(bad)[0])}"


def overlay(r, case):
    name, cam, (w, h), levels = case
    return r.bvh_overlay(oc.camera(cam, name), w, h, levels)


# ---------------------------------------------------------------- parity

@pytest.mark.parametrize("name", oc.SCENES)
def test_every_case_equals_the_oracle(gpu, mirt, name):
    upload(gpu, mirt, name)
    for case in oc.cases_of(name):
        same(overlay(gpu, case), oc.expected(*case), str(case))


@pytest.mark.parametrize("levels", oc.CHAIN_LEVELS)
def test_hand_chain300_at_every_level(gpu, mirt, levels):
    """Depths past the resident byte's clamp at 255, in the level test and in the colour."""
    upload(gpu, mirt, "hand_chain300")
    case = ("hand_chain300", "chain", BIG, levels)
    same(overlay(gpu, case), oc.expected(*case), str(case))
    # MIRT_LAYOUT_NDEPTH stays the clamped byte
    d = oc.depths(oc.scene("hand_chain300")[2])
    assert (gpu.resident_layout()[1]["ndepth"] == np.minimum(d, 255)).all()


def test_the_device_layout_path_gives_the_same_overlays(gpu, mirt):
    """mirt_scene_upload_flat_device derives the depth bytes on the device."""
    for name in ("hand_chain300", "r1000"):
        s, _, nodes = oc.scene(name)
        gpu.upload_device(s, nodes)
        for case in oc.cases_of(name)[-6:]:
            same(overlay(gpu, case), oc.expected(*case), f"upload_device, {case}")


# ---------------------------------------------------------------- the frame slab

def test_buffer_reuse_across_sizes_and_frames(mirt):
    """One context: 160 x 90, 1 x 1, 257 x 3, 160 x 90 again, with a rendered
    frame of another size before each (the overlay writes the frame's device
    output slab), and the frames stay what they were."""
    cam = oc.camera("default")
    with mirt.Renderer(0) as r:
        upload(r, mirt, "r1000")
        frames = {}
        for k, size in enumerate((BIG, (1, 1), (257, 3), BIG)):
            fw, fh = ((44, 26), (77, 45), (8, 8), (320, 180))[k]
            frame = r.render_frame(cam, fw, fh, depth=2)
            frames.setdefault((fw, fh), frame)
            case = ("r1000", "default", size, -1)
            same(overlay(r, case), oc.expected(*case), f"step {k}: {size} after a {fw} x {fh} frame")
            same(r.render_frame(cam, fw, fh, depth=2), frame, f"step {k}: the frame again")
        inside = ("r1000", "inside", BIG, -1)
        same(overlay(r, inside), oc.expected(*inside), "another camera into the same slab")


def test_a_pending_fresh_frame_on_a_shared_accumulation_buffer(mirt, oracle):
    """Two contexts share one accumulation buffer: A's fresh frame leaves its
    display pending in A's slab (the lazy fold), A draws an overlay into that
    slab, B accumulates the next frame: the fold must have taken A's frame,
    not the overlay."""
    w, h = BIG
    cam = oc.camera("default")
    s, tree, nodes = oc.scene("r1000")
    frames = [oracle.render(cam, w, h, s, tree, depth=5, mode=1, seed=6, sample=k) for k in range(2)]
    acc = np.zeros(3 * w * h, np.float32)
    oracle.accumulate(frames[0], acc, True, 1)
    shown = oracle.accumulate(frames[1], acc, False, 2).reshape(h, w, 4)
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
        for r in (A, B):
            r.upload(s, mirt.Bvh(nodes))
            r.share_accum(A)
        same(A.render_frame(cam, w, h, depth=5, seed=6, sample=0), frames[0], "A's fresh frame")
        same(A.bvh_overlay(cam, w, h), oc.expected("r1000", "default", BIG, -1), "A's overlay")
        got = B.render_frame(cam, w, h, depth=5, seed=6, sample=1, accumulate=True, frames=2)
        same(got, shown, "B's accumulated frame")
        assert B.accum(3 * w * h).tobytes() == acc.tobytes()


def test_a_frame_in_flight(mirt, small):
    """A context of its own: a frame waits behind a bounded stall, and
    bvh_overlay and camera_rays_uv are called on the context at once. Both
    run on the context's stream, behind the frame and its copy out of the
    slab the overlay then writes (d_out; camera_rays_uv's d_in and d_res are
    shared with no frame), so the frame is the frame without the stall and
    both results are their references."""
    abi = mirt.abi
    w, h = BIG
    cam = oc.camera("default")
    fd = mirt.frame_desc(w, h, depth=5, seed=3)
    uv = oc.pixel_uv(77, 45).reshape(-1, 2)
    want_uv = oc.cases._oracle().camera_rays(cam, 77, 45).reshape(-1)
    case = ("r1000", "inside", BIG, -1)
    buf = mirt.HostBuffer((h, w, 4))
    try:
        with mirt.Renderer(0) as r:
            upload(r, mirt, "r1000")
            want = r.render_frame(cam, w, h, depth=5, seed=3)
            buf.array[:] = 0
            r.set_option(abi.OPT_DEBUG_STALL_MS, 300)
            r.render_frame_async(cam, fd, buf)
            got_overlay = overlay(r, case)
            got_uv = r.camera_rays_uv(cam, 77, 45, uv)
            r.wait()
            r.set_option(abi.OPT_DEBUG_STALL_MS, 0)
            same(buf.array, want, "the frame in flight")
            same(got_overlay, oc.expected(*case), "the overlay behind it")
            assert got_uv.tobytes() == want_uv.tobytes()
            same(r.render_frame(cam, w, h, depth=5, seed=3), want, "the next frame")
    finally:
        buf.close()


# ---------------------------------------------------------------- after moved spheres

def oracle_overlay(nodes, cam=None):
    o = oc.cases._oracle()
    tree = o.tree_from_flat(nodes)
    try:
        return oc.overlay_of(tree, cam or oc.camera("default"), BIG)
    finally:
        o.free(tree)


def test_after_refit_update_and_rebuild(gpu, mirt):
    """The overlay is the oracle's of the tree the host path gives for the
    same spheres (mirt.refit_bvh, mirt.build_bvh), and differs from the one
    before the move."""
    cam = oc.camera("default")
    s0, _, nodes0 = oc.scene("r1000")
    n = len(s0)
    before = oc.expected("r1000", "default", BIG, -1)
    s1 = moved(s0, 2.0, 31)
    # mirt_scene_refit_device
    gpu.upload_device(s0, nodes0)
    same(gpu.bvh_overlay(cam, *BIG), before, "before")
    gpu.refit_scene(s1)
    assert gpu.last_refit_stats()["on_device"] == 1
    want = oracle_overlay(mirt.refit_bvh(nodes0, s1).nodes)
    assert (want != before).any()
    same(gpu.bvh_overlay(cam, *BIG), want, "after refit_device")
    # mirt_scene_update_device, both branches
    for branch, max_decay in (("refit", 0.0), ("rebuild", 1e-3)):
        gpu.upload(s0, mirt.Bvh(nodes0))
        hu = host_update(mirt, nodes0, s1, 0, n, max_decay, mirt.bvh_quality(nodes0, n)["cost"])
        assert hu["rebuilt"] == int(branch == "rebuild")
        _, _, res = gpu.update_scene(s1, 0, n, max_decay)
        assert res["rebuilt"] == hu["rebuilt"]
        want = oracle_overlay(hu["tree"])
        assert (want != before).any()
        same(gpu.bvh_overlay(cam, *BIG), want, f"after update_device, {branch}")
    # mirt_scene_build_device
    mine = s1.copy()
    built = mirt.build_bvh(mine).nodes
    gpu.build_scene(s1)
    assert gpu.last_scene_build_stats()["on_device"] == 1
    want = oracle_overlay(built)
    assert (want != before).any()
    same(gpu.bvh_overlay(cam, *BIG), want, "after build_scene_device")
    same(gpu.bvh_overlay(oc.camera("inside"), *BIG), oracle_overlay(built, oc.camera("inside")), "and from inside")


def test_on_a_context_that_shares_anothers_scene(mirt):
    cam = oc.camera("default")
    s0, _, nodes0 = oc.scene("r1000")
    s1 = moved(s0, 2.0, 32)
    before = oc.expected("r1000", "default", BIG, -1)
    want = oracle_overlay(mirt.refit_bvh(nodes0, s1).nodes)
    assert (want != before).any()
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
        A.upload(s0, mirt.Bvh(nodes0))
        B.share_scene(A)
        same(B.bvh_overlay(cam, *BIG), before, "the follower, before")
        A.refit_scene(s1)
        same(B.bvh_overlay(cam, *BIG), want, "the follower, after the owner's refit")
        same(A.bvh_overlay(cam, *BIG), want, "the owner")


# ---------------------------------------------------------------- arguments

def test_arguments(mirt):
    L = mirt.load()
    cam = oc.camera("default")
    out = np.full((4, 4, 4), 7, np.uint8)
    p = mirt.abi.ptr(out)
    call = lambda r, c, w, h, o: L.mirt_bvh_overlay(r.h, C.byref(c) if c is not None else None, w, h, -1, o)
    with mirt.Renderer(0) as r:
        assert call(r, cam, 4, 4, p) == E_NOSCENE
        upload(r, mirt, "r2")
        assert call(r, None, 4, 4, p) == E_INVALID
        assert call(r, cam, 4, 4, None) == E_INVALID
        for w, h in ((0, 4), (4, 0), (-1, 4), (4, -1), (oc.INT_MIN, 4), (4, oc.INT_MIN)):
            assert call(r, cam, w, h, p) == E_INVALID, (w, h)
        # 2^30 is the largest width or height: 2 * width is formed in int
        for w, h in ((2 ** 30 + 1, 1), (1, 2 ** 30 + 1), (oc.INT_MAX, 1), (1, oc.INT_MAX), (2 ** 30, 4), (65536, 65536)):
            assert call(r, cam, w, h, p) == E_INVALID, (w, h)
        assert b"mirt_bvh_overlay" in L.mirt_last_error()
        assert (out == 7).all()
        assert call(r, cam, 4, 4, p) == 0
        same(out, oc.overlay_of(oc.scene("r2")[1], cam, (4, 4)), "after the errors")

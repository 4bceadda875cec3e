"""Every walk, frame path, builder and install on hostile spheres
(tests/hostile_sphere_cases.py), against the CPU oracle, which
tests/test_hostile_spheres_host.py ties to the unmodified reference: negative,
zero, subnormal, NaN, infinite and overflowing radii, non-finite and far
centres, duplicates, giants around the o_bound threshold and dust.

The comparison rule is tests/test_hostile_rays_gpu.py's: hit, sphere, t and
colours byte for byte; point and normal byte for byte where the oracle's float
is not a NaN and a NaN where it is (the host file shows the oracle's records
hold no NaN on any of these scenes, so this never applies here; the tests
assert the count); the product's own identities without exception. The
builders and installs give the reference's tree, its sphere order and the
resident layout of mirt_scene_layout over them, whichever side ran; on_device
may be 0 only where csrc/tree.h's sphere_declined says so (restated in
`declined` below).

Why every loop these scenes enter terminates (read in csrc/trace.h,
csrc/render.hip, csrc/bvh_device.hip, csrc/scene_device.hip and
csrc/refit_device.hip). A sphere's numbers only ever decide a comparison;
no loop index moves by a value computed from a box or a sphere.

  the walks: as tests/test_hostile_rays_gpu.py states them -- every walk moves
    by next + 1, a skip link or a stack pop of a tree that mirt_scene_upload
    validated (skip > index, children nested in (i, skip)), whatever the boxes
    hold: inverted boxes (neg_r), +-inf boxes (inf_*, huge_r, far_c: a slab test
    on them gives NaN or inf distances, a false or true comparison), NaN
    areas. The sort keys of the four-wide walks pass through fminf(e, 3.0e38f).
  the packet walk's stack has 64 entries, one per level; the trees here are the
    reference's, at most 40 inner levels deep (the dense inf / huge / far
    scenes are exactly that chain), and scene_layout's `ordered` (asserted 1
    for every scene in the host file) is false for a tree whose depth + 2
    exceeds 64, which then takes the DFS walk
    (test_refit_device.test_deep_chain_takes_the_host_path has such a tree).
  Prune (r_max, c_max) and the origin bound are off (encloses == 0 or
    o_bound == 0) for every scene with a non-finite or negative sphere or
    C >= 6.0e4; where they are on, the constants are finite.
  the bounce kernel's queue loop and hemisphere: bounded by depth and by 4096
    tries, and read no sphere.
  device_build's level loop runs `for (d = depth;; d++)` until a level has no
    inner node; classify_kernel makes every node of level kMaxDepth = 40 a
    leaf, so at most 41 rounds whatever the SAH costs are (NaN and inf costs
    leave bvh.c's fallback split, best_split = 0, which the chain scenes take
    at every level). run_partition's jump rounds number ceil(log2(longest
    range)), computed on the host. subtree_kernel's walks carry a cap and
    report kCtlError instead of running on. size_kernel / emit_kernel run once
    per recorded level.
  scene_device's four-wide loop adds cnt > 0 HNodes per round against the bound
    cap_h = 1 + inner nodes and fails with an error past it; hnode_cut and
    live_node are bounded by nn steps.
  refit_device folds level by level from the resident ndepth's maximum down to
    0; a leaf's fold is bounded by kShort and by `end`.
"""
import numpy as np
import pytest

import denoise_cases as dc
import hostile_sphere_cases as sc
import reproject_cases as rpc
import test_planes_cases as cases
from test_hostile_rays_gpu import (CAMERA_SCHEDULES, DEVICE_NAN, check_per_ray, options, same, same_bytes, same_planes,
                                   walks)
from test_planes_gpu import schedules
from test_ray_frames_gpu import SCHEDULES
from test_refit_device import assert_same_layout, host_layout
from test_update_device import check_update, host_update

pytestmark = pytest.mark.gpu

N = sc.N
PLANES = ("t", "sphere", "normal")
# scenes with finite inputs that nothing declines, boxes that overflow included: built and refit on the device
ON_DEVICE = ("zero_r_4th", "tiny_r", "scales", "huge_r_sparse", "huge_r_4th", "far_c_sparse", "far_c_4th", "dups",
             "giant_wall", "giant_dome_50000", "giant_dome_59900", "giant_dome_61000", "giant_inplace", "dust_scene",
             "dust_radii")


def upload(gpu, mirt, name):
    s, _, nodes = sc.scene(name)
    gpu.upload(s, mirt.Bvh(nodes))
    return s


def declined(s):
    """csrc/tree.h sphere_declined over an array: a NaN or an infinity, a negative radius, or a box coordinate
    fl(c -+ r) that is -0.0."""
    c, r = s["center"], s["radius"]
    bad = ~np.isfinite(c).all(1) | ~np.isfinite(r) | (r < 0)
    with np.errstate(over="ignore", invalid="ignore"):
        for box in (c - r[:, None], c + r[:, None]):
            bad |= (np.ascontiguousarray(box).view(np.uint32) == 0x80000000).any(1)
    return bool(bad.any())


def test_which_scenes_are_declined():
    got = [name for name in sc.SCENES if not declined(sc.inputs(name)[0])]
    assert got == list(ON_DEVICE)
    assert not declined(cases.scene(N)[0])


# ---------------------------------------------------------------- the walks

@pytest.mark.parametrize("name", sc.SCENES)
def test_closest_hit_and_any_hit_on_every_walk(gpu, mirt, name):
    upload(gpu, mirt, name)
    for rs in sc.ray_sets(name):
        check_per_ray(gpu, mirt, sc.rays(name, *rs), sc.hits(name, *rs), sc.hits(name, *rs, False), f"{name} {rs}")


@pytest.mark.parametrize("name", sc.SCENES)
def test_trace_rays(gpu, mirt, name):
    abi = mirt.abi
    upload(gpu, mirt, name)
    for rs in sc.ray_sets(name):
        if rs[1:] != sc.SIZES[0]:
            continue
        flat = np.ascontiguousarray(sc.rays(name, *rs)).reshape(-1)
        for what, opts, use_bvh in (("default", {}, True), ("DFS", {abi.OPT_ORDERED: 0, abi.OPT_PRUNE: 0}, True),
                                    ("brute force", {}, False)):
            with options(gpu, abi, opts):
                for depth in sc.DEPTHS:
                    got = gpu.trace_ray(flat, depth=depth, use_bvh=use_bvh).reshape(rs[2], rs[1], 4)
                    same(got, sc.colours(name, *rs, depth, use_bvh), f"{name} {rs} trace_ray {what} depth {depth}")


@pytest.mark.parametrize("name", sc.SCENES)
def test_ray_frames_on_every_schedule(gpu, mirt, name):
    abi = mirt.abi
    upload(gpu, mirt, name)
    for rs in sc.ray_sets(name):
        _, w, h = rs
        rays = sc.rays(name, *rs)
        flat = np.ascontiguousarray(rays).reshape(-1)
        for schedule in SCHEDULES:
            depth, use_bvh, opts = schedules(abi)[schedule]
            what = f"{name} {rs} on {schedule}"
            with options(gpu, abi, opts):
                rgba, got = gpu.render_rays(rays, w, h, planes=PLANES, depth=depth, use_bvh=use_bvh)
                same(rgba, sc.colours(name, *rs, depth, use_bvh), what + " against the oracle")
                assert same_planes(got, sc.planes(name, *rs, use_bvh), what) == 0
                # the product's own identities
                same_bytes(rgba, gpu.trace_ray(flat, depth=depth, use_bvh=use_bvh), what + " against mirt_trace_rays")
                rec = gpu.closest_hit(flat, use_bvh=use_bvh).reshape(h, w)
                for k in PLANES:
                    same_bytes(got[k], rec[k], f"{what}: plane {k} against mirt_intersect_rays")
    rs = sc.ray_sets(name)[-1]   # the bounce pass's own options, on the ray set that sees most of the hostile spheres
    for what, opts in walks(abi)[5:]:
        with options(gpu, abi, opts):
            for depth in (5, 8):
                same(gpu.render_rays(sc.rays(name, *rs), rs[1], rs[2], depth=depth), sc.colours(name, *rs, depth),
                     f"{name} {rs}, {what}, depth {depth}")


# ---------------------------------------------------------------- camera frames

@pytest.mark.parametrize("name", sc.SCENES)
def test_camera_frames_through_the_packet_kernel(gpu, mirt, name):
    """render_frame and render_frame_planes at 44 x 26 and 77 x 45 against
    oracle.render on four schedules; with the primary cache on, the second
    frame is a HIT with the first one's bytes, and the filling frame is the
    walked one (a BYPASS both times where the scene is walked unpruned)."""
    abi = mirt.abi
    upload(gpu, mirt, name)
    # a tree that does not enclose its spheres is walked unpruned: no camera-packet kernel, a BYPASS (SCHEDULE)
    pruned = gpu.resident_layout()[0]["encloses"] == 1
    assert pruned == (name in ON_DEVICE or name == "neg_hidden")   # (but for it, the declined scenes are the unpruned ones)
    for cam_name, w, h in sc.ray_sets(name):
        cam = sc.camera(name, cam_name)
        want = sc.camera_frame(name, cam_name, w, h)
        for schedule in CAMERA_SCHEDULES:
            depth, use_bvh, opts = schedules(abi)[schedule]
            what = f"{name} camera {cam_name} {w}x{h} on {schedule}"
            with options(gpu, abi, opts):
                same(gpu.render_frame(cam, w, h, depth=depth, use_bvh=use_bvh), want, what)
                rgba, got = gpu.render_frame_planes(cam, w, h, depth=depth, use_bvh=use_bvh)
                same(rgba, want, what + " with planes")
                assert same_planes(got, sc.planes(name, cam_name, w, h, use_bvh), what) == 0
        same(gpu.render_frame(cam, w, h, depth=5, use_bvh=False), sc.camera_frame(name, cam_name, w, h, False),
             f"{name} camera {cam_name} {w}x{h} by brute force")
        with options(gpu, abi, {abi.OPT_PRIMARY_CACHE: 1}):
            first = gpu.render_frame(cam, w, h, depth=5)
            st = gpu.primary_cache_stats()
            assert (st["last"], st["valid"]) == (("fill", 1) if pruned else ("bypass", 0)), (name, st)
            second = gpu.render_frame(cam, w, h, depth=5)
            st = gpu.primary_cache_stats()
            assert st["last"] == ("hit" if pruned else "bypass") and (st["reason"] == "") == pruned, (name, st)
            same_bytes(second, first, f"{name} camera {cam_name} {w}x{h}: the frame from the cache")
            same(first, want, f"{name} camera {cam_name} {w}x{h}: the filling frame")


@pytest.mark.parametrize("name", sc.SCENES)
def test_a_shard_split_and_four_accumulating_samples(gpu, mirt, oracle, name):
    upload(gpu, mirt, name)
    rs = sc.ray_sets(name)[-1]
    _, w, h = rs
    rays = sc.rays(name, *rs)
    want = sc.colours(name, *rs, 5, True, seed=3, sample=2)
    seen = []
    for shard in range(3):
        kw = dict(depth=5, seed=3, sample=2, row_block=8, shard=shard, num_shards=3)
        rows = mirt.shard_rows(mirt.frame_desc(w, h, **kw))
        seen += list(rows)
        rgba, got = gpu.render_rays(np.ascontiguousarray(rays[rows]), w, h, planes=PLANES, **kw)
        same(rgba, want[rows], f"{name}: shard {shard}")
        same_planes(got, cases.planes_of(sc.hits(name, *rs)[rows], (len(rows), w)), f"{name}: shard {shard}")
    assert sorted(seen) == list(range(h))
    n = w * h
    acc = np.zeros(3 * n, np.float32)
    shown = None
    for k in range(6):
        shown = oracle.accumulate(sc.colours(name, *rs, 5, True, seed=5, sample=k), acc, k == 0, k + 1).reshape(h, w, 4)
    gpu.render_rays(rays, w, h, depth=5, seed=5, sample=0)
    gpu.render_rays(rays, w, h, depth=5, seed=5, sample=1, accumulate=True, frames=2)
    got = gpu.render_rays(np.stack([rays] * 4), w, h, depth=5, seed=5, sample=2, samples=4, accumulate=True, frames=3)
    same(got, shown, f"{name}: four accumulating samples")
    same_bytes(gpu.accum(3 * n), acc, f"{name}: the accumulation buffer")


@pytest.mark.parametrize("name", ["neg_r_4th", "giant_wall", "giant_dome_50000"])
def test_denoised_and_reprojected_frames(gpu, mirt, name):
    """mirt_render_frame_denoised against mirt_denoise_host, and the
    reprojected loop [A, B, A] against mirt_reproject_host, both fed the
    ORACLE's frame and planes: the wall behind every pixel, hits on
    negative-radius spheres, a dome around the camera."""
    upload(gpu, mirt, name)
    L = mirt.load()
    w, h = sc.SIZES[0]
    cam = sc.camera(name, "A")
    pl = sc.planes(name, "A", w, h)
    out, raw = gpu.render_frame_denoised(cam, w, h, raw=True, depth=5, seed=1, sample=1)
    frame = sc.camera_frame(name, "A", w, h, sample=1)
    same_bytes(raw, frame, f"{name}: raw against the oracle")
    same_bytes(out, dc.host_filter(L, w, h, pl["sphere"], pl["normal"], dc.DEFAULT, rgba=frame),
               f"{name}: out against the host filter of the oracle's frame and planes")
    assert (out != raw).any()
    gpu.history_reset()
    prev = None
    for k, cam_name in enumerate(["A", "B", "A"]):
        cam = sc.camera(name, cam_name)
        pl = sc.planes(name, cam_name, w, h)
        frame = sc.camera_frame(name, cam_name, w, h, sample=k)
        hist, want = rpc.host_step(L, cam, frame, pl["t"], pl["sphere"], prev, rpc.DEFAULT)
        prev = (cam, hist, pl["t"], pl["sphere"])
        out, raw = gpu.render_frame_reprojected(cam, w, h, params=rpc.DEFAULT, raw=True, depth=5, seed=1, sample=k)
        same_bytes(raw, frame, f"{name} frame {k} ({cam_name}): raw")
        same_bytes(out, want, f"{name} frame {k} ({cam_name}): out")
        same_bytes(gpu.history_read(), hist, f"{name} frame {k} ({cam_name}): the records")
        st = gpu.history_stats()
        assert st["reused"] + st["fresh"] + st["sky"] == w * h and st["frames"] == k + 1, (name, st)
    gpu.history_reset()


# ---------------------------------------------------------------- builders and installs

class finish:
    """MIRT_OPT_BUILD_FINISH set for a block, the default (1) restored."""

    def __init__(self, gpu, mirt, value):
        self.gpu, self.opt, self.value = gpu, mirt.abi.OPT_BUILD_FINISH, value

    def __enter__(self):
        self.gpu.set_option(self.opt, self.value)

    def __exit__(self, *a):
        self.gpu.set_option(self.opt, 1)


def in_resident_order(name):
    """The hostile scene's spheres in the order test_planes_cases.scene(1000) holds the ordinary ones."""
    s0 = cases.scene(N)[0]
    where = {sc.base()[i].tobytes(): i for i in range(N)}
    return sc.inputs(name)[0][[where[s0[i].tobytes()] for i in range(N)]]


@pytest.mark.parametrize("name", sc.SCENES)
def test_builds_give_the_references_tree(gpu, mirt, name):
    """gpu.build_bvh and mirt_scene_build_device, with the finish on and off."""
    pre = sc.inputs(name)[0]
    s, _, nodes = sc.scene(name)
    want = mirt.scene_layout(s, mirt.Bvh(nodes))
    on_device = int(name in ON_DEVICE)
    for value in (1, 0):
        with finish(gpu, mirt, value):
            what = f"{name}, finish {value}"
            mine = pre.copy()
            b = gpu.build_bvh(mine)
            st = gpu.last_build_stats()
            assert st["on_device"] == on_device, (what, st)
            same_bytes(mine, s, what + ": build_bvh's sphere order")
            same_bytes(b.nodes, nodes, what + ": build_bvh's tree")
            fin = gpu.last_build_finish()
            assert fin["moved"] == 0 and (value == 1 or fin["range"] == 0), (what, fin)
            reordered = gpu.build_scene(pre)
            st = gpu.last_scene_build_stats()
            assert st["on_device"] == on_device and st["nodes"] == len(nodes), (what, st)
            same_bytes(reordered, s, what + ": build_scene's sphere order")
            assert_same_layout(mirt, gpu.resident_layout(), want, what + ": build_scene")
    # and the scene just installed renders the oracle's frame
    w, h = sc.SIZES[0]
    same(gpu.render_frame(sc.camera(name, "A"), w, h, depth=5), sc.camera_frame(name, "A", w, h), name + " after build_scene")


@pytest.mark.parametrize("name", sc.SCENES)
def test_refits_to_and_on_the_hostile_scene(gpu, mirt, name):
    """mirt_scene_refit_device from the ordinary scene to the hostile spheres
    (the ordinary topology), and the identity refit of the hostile tree."""
    s0, _, nodes0 = cases.scene(N)
    moved = in_resident_order(name)
    on_device = int(name in ON_DEVICE)
    gpu.upload_device(s0, nodes0)
    got = gpu.refit_scene(moved, return_nodes=True)
    st = gpu.last_refit_stats()
    assert st["on_device"] == on_device and st["nodes"] == len(nodes0), (name, st)
    same_bytes(got.nodes, mirt.refit_bvh(nodes0, moved).nodes, name + ": the refit tree")
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes0, moved, N), name + ": to the hostile spheres")
    gpu.refit_scene(s0)
    assert gpu.last_refit_stats()["on_device"] == 1
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes0, s0, N), name + ": and back")
    s, _, nodes = sc.scene(name)
    gpu.upload_device(s, nodes)
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(s, mirt.Bvh(nodes)), name + ": upload_device")
    gpu.refit_scene(s)
    assert gpu.last_refit_stats()["on_device"] == on_device
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s, N), name + ": the identity refit")


@pytest.mark.parametrize("branch", ["refit", "rebuild"])
@pytest.mark.parametrize("name", sc.SCENES)
def test_updates_to_the_hostile_scene_and_back(gpu, mirt, oracle, name, branch):
    """mirt_scene_update, the refit branch (max_decay 0) and the rebuilding one
    (any decay is past 1e-3), from the ordinary scene to the hostile one and
    back; a rebuilt tree is the oracle's of the same spheres."""
    s0, _, nodes0 = cases.scene(N)
    moved = in_resident_order(name)
    max_decay = 0.0 if branch == "refit" else 1e-3
    gpu.upload(s0, mirt.Bvh(nodes0))
    base = mirt.bvh_quality(nodes0, N)["cost"]
    want = host_update(mirt, nodes0, moved, 0, N, max_decay, base)
    assert want["rebuilt"] == int(branch == "rebuild")
    if want["rebuilt"]:
        mine = moved.copy()
        t = oracle.build(mine)
        same_bytes(want["tree"], oracle.flatten(t), name + ": the host's rebuilt tree against the oracle's")
        oracle.free(t)
        same_bytes(want["spheres"], mine, name + ": the rebuilt order")
    check_update(mirt, gpu, gpu.update_scene(moved, 0, N, max_decay), want, f"{name}, {branch}",
                 on_device=int(name in ON_DEVICE))
    back = s0[want["perm"]]
    base = want["installed"]["cost"] if want["rebuilt"] else want["base_cost"]
    want2 = host_update(mirt, want["tree"], back, 0, N, max_decay, base)
    check_update(mirt, gpu, gpu.update_scene(back, 0, N, max_decay), want2, f"{name}, {branch}, and back")


def test_device_nan_patterns():
    print("device NaN patterns met by this file:", sorted(DEVICE_NAN) or "none")

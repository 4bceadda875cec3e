"""Frames with primary-hit planes on the GPU (mirt_render_frame_planes, _device,
_async): every plane byte-equal with the oracle's hit records of the frame's
camera rays (tests/test_planes_cases.py), on every schedule a frame can take,
and the colours byte-equal with the same frame without planes."""
import ctypes as C

import numpy as np
import pytest

import test_planes_cases as cases

pytestmark = pytest.mark.gpu

NAMES = ("t", "sphere", "normal")
E_NOSCENE = -3


def ok(r, rc):
    assert rc == 0, (rc, r.L.mirt_last_error().decode())


def upload(r, mirt, n):
    spheres, _, nodes = cases.scene(n)
    r.upload(spheres, mirt.Bvh(nodes))
    return spheres


def assert_planes(got, want, what):
    """Byte equality plane by plane; the count of differing elements goes into the message."""
    assert set(got) == set(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        diff = g.view(np.uint32) != w.view(np.uint32)
        assert not diff.any(), f"{what}: plane {k}: {int(diff.sum())} of {diff.size} words differ"


class options:
    """Schedule options set for one block and restored after it."""

    def __init__(self, r, opts):
        self.r, self.opts = r, opts

    def __enter__(self):
        self.old = {k: self.r.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.r.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.r.set_option(k, v)


def check_case(gpu, mirt, name, depth, use_bvh=True):
    c = cases.CASES[name]
    spheres = upload(gpu, mirt, c["n"])
    cam = cases.camera(name)
    plain = gpu.render_frame(cam, c["W"], c["H"], depth=depth, use_bvh=use_bvh)
    rgba, got = gpu.render_frame_planes(cam, c["W"], c["H"], depth=depth, use_bvh=use_bvh)
    want = cases.expected(name, use_bvh)
    assert_planes(got, want, f"case {name} depth {depth} bvh {use_bvh}")
    assert rgba.tobytes() == plain.tobytes()
    if depth == 1:   # base + 0.5 * black of the sphere the plane names
        hit = want["sphere"] >= 0
        assert (rgba[hit][:, :3] == spheres["color"][want["sphere"][hit]][:, :3]).all()


def schedules(abi):
    return {
        "wavefront_ordered_d5": (5, True, {}),
        "primary_only_d1": (1, True, {}),
        "tile_d5": (5, True, {abi.OPT_TRAVERSAL: abi.TRAV_TILE}),
        "unordered_deferred_d5": (5, True, {abi.OPT_ORDERED: 0, abi.OPT_DEFER: 1}),
        "unordered_undeferred_d5": (5, True, {abi.OPT_ORDERED: 0, abi.OPT_DEFER: 0}),
        "tile_unordered_d5": (5, True, {abi.OPT_TRAVERSAL: abi.TRAV_TILE, abi.OPT_ORDERED: 0}),
        "exact_slab_d5": (5, True, {abi.OPT_FAST_SLAB: 0}),
        "brute_force_d5": (5, False, {}),
        "brute_force_exact_slab_d5": (5, False, {abi.OPT_FAST_SLAB: 0}),
    }


@pytest.mark.parametrize("schedule", ["wavefront_ordered_d5", "primary_only_d1", "tile_d5", "unordered_deferred_d5",
                                      "unordered_undeferred_d5", "tile_unordered_d5", "exact_slab_d5",
                                      "brute_force_d5", "brute_force_exact_slab_d5"])
def test_case_a_on_every_schedule(gpu, mirt, schedule):
    depth, use_bvh, opts = schedules(mirt.abi)[schedule]
    with options(gpu, opts):
        check_case(gpu, mirt, "A", depth, use_bvh)


@pytest.mark.parametrize("depth", [5, 1])
def test_case_b_takes_the_unbounded_ordered_kernel(gpu, mirt, depth):
    upload(gpu, mirt, cases.CASES["B"]["n"])
    info, _ = gpu.resident_layout()
    assert info["ordered"] and info["o_bound"] > 0 and 600 > 4 * info["o_bound"], info
    check_case(gpu, mirt, "B", depth)


def test_case_c_and_five_samples_without_jitter(gpu, mirt):
    check_case(gpu, mirt, "C", 5)
    c = cases.CASES["C"]
    cam = cases.camera("C")
    plain = gpu.render_frame(cam, c["W"], c["H"], depth=5, samples=5)
    rgba, got = gpu.render_frame_planes(cam, c["W"], c["H"], depth=5, samples=5)
    assert rgba.tobytes() == plain.tobytes()
    want = cases.expected("C")
    for j in range(5):   # the same camera rays in every frame: every slab holds the one-sample planes
        assert_planes({k: got[k][j] for k in NAMES}, want, f"case C slab {j}")


def test_jittered_samples_of_a_shard_fresh_and_accumulating(gpu, mirt):
    """4x4 pixels x 4 frames packets (samples >= 4) of a jittered shard: the
    rays are mirt_camera_rays' of the same frame descriptor, the hits the
    oracle's on those rays; displays and accumulation equal the plain call's."""
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    upload(gpu, mirt, c["n"])
    cam = cases.camera("A")
    kw = dict(depth=5, samples=5, jitter=True, num_shards=3, shard=1, row_block=4)
    for extra in (dict(sample=0), dict(sample=5, accumulate=True, frames=6)):
        fd = mirt.frame_desc(W, H, **kw, **extra)
        n = len(mirt.shard_rows(fd))
        assert 0 < n < H
        rays = np.zeros((5 * n, W), mirt.abi.RAY)
        ok(gpu, gpu.L.mirt_camera_rays(gpu.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(rays)))
        want = cases.planes_of(cases.intersect(c["n"], rays), (5, n, W))
        if extra.get("accumulate"):   # the plain run: fresh, then accumulating
            gpu.render_frame(cam, W, H, **kw, sample=0)
        plain = gpu.render_frame(cam, W, H, **kw, **extra)
        plain_acc = gpu.accum(n * W * 3)
        if extra.get("accumulate"):
            gpu.render_frame(cam, W, H, **kw, sample=0)
        rgba, got = gpu.render_frame_planes(cam, W, H, **kw, **extra)
        assert_planes(got, want, f"jittered shard {extra}")
        assert rgba.tobytes() == plain.tobytes()
        assert gpu.accum(n * W * 3).tobytes() == plain_acc.tobytes()
        assert (want["sphere"] >= 0).any() and (want["sphere"] < 0).any()


def test_only_the_requested_plane_is_written(gpu, mirt):
    """`sphere` alone, blocking and device form: the other planes' buffers and
    the 64 guard elements behind every plane keep their pattern."""
    import torch
    c = cases.CASES["A"]
    W, H, n = c["W"], c["H"], c["W"] * c["H"]
    upload(gpu, mirt, c["n"])
    cam, fd = cases.camera("A"), mirt.frame_desc(W, H, depth=5)
    want = cases.expected("A")["sphere"].reshape(-1)
    out = np.zeros(n, np.uint32)
    t, s, nm = np.full(n + 64, 7.5, np.float32), np.full(n + 64, 0x5A5A5A5A, np.int32), np.full(3 * n + 64, 7.5, np.float32)
    pl = mirt.abi.PrimaryPlanes(None, s.ctypes.data, None)
    ok(gpu, gpu.L.mirt_render_frame_planes(gpu.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(out), C.byref(pl)))
    assert (s[:n] == want).all() and (s[n:] == 0x5A5A5A5A).all() and (t == 7.5).all() and (nm == 7.5).all()
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_t = torch.full((n + 64,), 7.5, dtype=torch.float32, device=dev)
    d_s = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_n = torch.full((3 * n + 64,), 7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    gpu.render_frame_planes_device(cam, fd, d_out.data_ptr(), {"sphere": d_s.data_ptr()})
    torch.cuda.synchronize()
    assert (d_s.cpu().numpy()[:n] == want).all() and bool((d_s[n:] == 0x5A5A5A5A).all())
    assert bool((d_t == 7.5).all()) and bool((d_n == 7.5).all())
    # each plane alone, with its guard
    for k, d, fill in (("t", d_t, 7.5), ("normal", d_n, 7.5)):
        gpu.render_frame_planes_device(cam, fd, d_out.data_ptr(), {k: d.data_ptr()})
        torch.cuda.synchronize()
        m = d.numel() - 64
        assert d[:m].cpu().numpy().tobytes() == cases.expected("A")[k].tobytes() and bool((d[m:] == fill).all())
    assert d_out.cpu().numpy().tobytes() == out.tobytes()


def test_device_and_async_forms_equal_the_blocking_one(gpu, mirt):
    import torch
    c = cases.CASES["A"]
    W, H, n = c["W"], c["H"], c["W"] * c["H"]
    upload(gpu, mirt, c["n"])
    cam, fd = cases.camera("A"), mirt.frame_desc(W, H, depth=5)
    rgba, want = gpu.render_frame_planes(cam, W, H, depth=5)
    # device pointers, on a caller's stream
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d = {"t": torch.zeros(n, dtype=torch.float32, device=dev), "sphere": torch.zeros(n, dtype=torch.int32, device=dev),
         "normal": torch.zeros(3 * n, dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    gpu.render_frame_planes_device(cam, fd, d_out.data_ptr(), {k: v.data_ptr() for k, v in d.items()},
                                   stream=stream.cuda_stream)
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == rgba.tobytes()
    assert_planes({k: v.cpu().numpy().reshape(want[k].shape) for k, v in d.items()}, want, "device form")
    # frames in flight on two contexts that share one scene, into page-locked memory
    with mirt.Renderer(0) as r1, mirt.Renderer(0) as r2:
        upload(r1, mirt, c["n"])
        r2.share_scene(r1)
        assert r1.scene_id() == r2.scene_id() != 0
        bufs = []
        for r in (r1, r2):
            out = mirt.HostBuffer((H, W, 4))
            pl = {"t": mirt.HostBuffer((H, W), np.float32), "sphere": mirt.HostBuffer((H, W), np.int32),
                  "normal": mirt.HostBuffer((H, W, 3), np.float32)}
            r.render_frame_planes_async(cam, fd, out, pl)
            bufs.append((out, pl))
        for r, (out, pl) in zip((r1, r2), bufs):
            r.wait()
            assert out.array.tobytes() == rgba.tobytes()
            assert_planes({k: b.array for k, b in pl.items()}, want, "async form")
        for out, pl in bufs:
            for b in (out, *pl.values()):
                b.close()


def test_planes_follow_a_scene_that_moved_and_was_rebuilt(mirt):
    """build_scene, then update_scene with a max_decay that forces the rebuild:
    the planes index the reordered spheres, and perm carries them back to the
    caller's."""
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    cam = cases.camera("A")
    with mirt.Renderer(0) as r:
        first = r.build_scene(mirt.create_random_spheres(1000, 1))
        moved = first.copy()
        moved["center"] += np.random.default_rng(7).normal(0.0, 2.0, (1000, 3)).astype(np.float32)
        reordered, perm, res = r.update_scene(moved, max_decay=1e-6)
        assert res["rebuilt"] == 1 and (perm != np.arange(1000)).any()
        hits = r.closest_hit(r.get_camera_rays(cam, W, H).reshape(-1))
        want = cases.planes_of(hits, (H, W))
        for depth in (1, 5):
            rgba, got = r.render_frame_planes(cam, W, H, depth=depth)
            assert_planes(got, want, f"moved scene depth {depth}")
            assert rgba.tobytes() == r.render_frame(cam, W, H, depth=depth).tobytes()
        hit = got["sphere"] >= 0
        assert hit.sum() >= 200 and (~hit).sum() >= 200
        s = got["sphere"][hit]
        rgba, _ = r.render_frame_planes(cam, W, H, depth=1)
        assert (rgba[hit][:, :3] == reordered["color"][s][:, :3]).all()
        assert moved[perm[s]].tobytes() == reordered[s].tobytes()


def test_empty_scene_no_scene_and_no_tree(gpu, mirt):
    W, H = 44, 26
    cam = mirt.default_camera()
    gpu.upload(np.zeros(0, mirt.abi.SPHERE), None)
    plain = gpu.render_frame(cam, W, H, depth=5, use_bvh=False)
    rgba, got = gpu.render_frame_planes(cam, W, H, depth=5, use_bvh=False)
    assert rgba.tobytes() == plain.tobytes()
    assert not got["t"].view(np.uint32).any() and (got["sphere"] == -1).all() and not got["normal"].view(np.uint32).any()
    with pytest.raises(mirt.MirtError):
        gpu.render_frame(cam, W, H, depth=5, use_bvh=True)
    with pytest.raises(mirt.MirtError):
        gpu.render_frame_planes(cam, W, H, depth=5, use_bvh=True)
    with mirt.Renderer(0) as r:   # no scene at all
        fd = mirt.frame_desc(W, H, depth=5, use_bvh=False)
        out, s = np.zeros(W * H, np.uint32), np.zeros(W * H, np.int32)
        pl = mirt.abi.PrimaryPlanes(None, s.ctypes.data, None)
        args = (r.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(out))
        assert r.L.mirt_render_frame_planes(*args, C.byref(pl)) == E_NOSCENE
        assert r.L.mirt_render_frame_planes_async(*args, C.byref(pl)) == E_NOSCENE
        assert r.L.mirt_render_frame_planes_device(*args, None, C.byref(pl), None) == E_NOSCENE

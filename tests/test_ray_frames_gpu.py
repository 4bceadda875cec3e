"""Ray frames on the GPU (mirt_render_rays, mirt_render_rays_device): frames
rendered from caller-given camera rays. Byte equality throughout: with the
plain frame when the rays are the pinhole's, with the oracle's trace_ray of the
same rays (tests/ray_frame_cases.py) and with mirt_trace_rays otherwise, on
every schedule a frame can take, through shards, several samples,
accumulation, the device form, planes and the primary cache."""
import ctypes as C

import numpy as np
import pytest

import ray_frame_cases as rc
import test_planes_cases as cases
from conftest import parse_frame_key, sha
from test_planes_gpu import assert_planes, ok, options, schedules, upload

pytestmark = pytest.mark.gpu

W, H = rc.W, rc.H
GOLDEN_KEY = "160x90_render100_d5_m1_b1_s1_c0_step1"
SCHEDULES = ["wavefront_ordered_d5", "primary_only_d1", "tile_d5", "unordered_deferred_d5", "unordered_undeferred_d5",
             "tile_unordered_d5", "exact_slab_d5", "brute_force_d5", "brute_force_exact_slab_d5"]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = (got != want).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ"


def test_pinhole_rays_give_the_golden_frame(gpu, mirt, golden, small):
    p = parse_frame_key(GOLDEN_KEY)
    s = mirt.create_random_spheres(p["n"], 1)
    gpu.upload(s, mirt.build_bvh(s))
    cam = mirt.abi.Camera.from_numpy(small["cameras"][p["cam"]])
    rays = gpu.get_camera_rays(cam, p["W"], p["H"])
    got = gpu.render_rays(rays, p["W"], p["H"], depth=p["depth"], use_bvh=p["use_bvh"], seed=p["seed"])
    assert sha(got[::p["step"]]) == golden["frames"][GOLDEN_KEY]["sha"]
    same(got, gpu.render_frame(cam, p["W"], p["H"], depth=p["depth"], use_bvh=p["use_bvh"], seed=p["seed"]), "golden")


@pytest.mark.parametrize("depth", [0, 1, 2, 5, 8])
def test_pinhole_rays_equal_the_plain_frame(gpu, mirt, depth):
    upload(gpu, mirt, rc.N)
    cam = cases.camera("A")
    fd = mirt.frame_desc(W, H, depth=depth)
    rays = np.zeros((H, W), mirt.abi.RAY)
    ok(gpu, gpu.L.mirt_camera_rays(gpu.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(rays)))
    got = gpu.render_rays(rays, W, H, depth=depth)
    same(got, gpu.render_frame(cam, W, H, depth=depth), f"depth {depth}")
    same(got, rc.colours("pinhole", depth=depth), f"depth {depth} against the oracle")
    if depth == 0:
        assert (got == np.array([0, 0, 0, 255], np.uint8)).all()


@pytest.mark.parametrize("name", rc.SETS)
def test_every_set_at_depth_5(gpu, mirt, name):
    upload(gpu, mirt, rc.N)
    rays = rc.rays(name)
    got = gpu.render_rays(rays, W, H, depth=5)
    same(got, rc.colours(name), name + " against the oracle")
    same(got, gpu.trace_ray(rays.reshape(-1), depth=5).reshape(H, W, 4), name + " against mirt_trace_rays")
    # a default BVH frame of depth 5 takes the wavefront schedule: its phases were timed
    out = (C.c_float * 2)()
    ok(gpu, gpu.L.mirt_last_phase_ms(gpu.h, out))
    assert out[0] > 0 and out[1] > 0


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_lens_and_ortho_on_every_schedule(gpu, mirt, schedule):
    depth, use_bvh, opts = schedules(mirt.abi)[schedule]
    upload(gpu, mirt, rc.N)
    with options(gpu, opts):
        for name in ("lens", "ortho"):
            got = gpu.render_rays(rc.rays(name), W, H, depth=depth, use_bvh=use_bvh)
            same(got, rc.colours(name, depth=depth, use_bvh=use_bvh), f"{name} on {schedule}")


def canary(n):
    return np.full(n, 0x5A5A5A5A, np.uint32)


@pytest.mark.parametrize("height,lead_skip", [(H, 0), (H, 1), (9, 0), (9, 1)])
def test_shards(gpu, mirt, height, lead_skip):
    """Shards 0..2 of 3 at row_block 8; at height 9 some shards are empty: MIRT_OK, nothing written."""
    upload(gpu, mirt, rc.N)
    full = rc.rays("lens")[:height]
    spheres, tree, _ = cases.scene(rc.N)
    want = cases._oracle().trace_rays(np.ascontiguousarray(full).reshape(-1), spheres, tree, depth=5, seed=3,
                                      sample=2).reshape(height, W, 4)
    seen = []
    for shard in range(3):
        kw = dict(depth=5, seed=3, sample=2, row_block=8, shard=shard, num_shards=3, lead_skip=lead_skip)
        fd = mirt.frame_desc(W, height, **kw)
        rows = mirt.shard_rows(fd)
        seen += list(rows)
        rays = np.ascontiguousarray(full[rows])
        if len(rows):
            got = gpu.render_rays(rays, W, height, **kw)
            same(got, want[rows], f"shard {shard} of height {height}, lead_skip {lead_skip}")
            continue
        # an empty shard: the rays are not read and nothing is written, planes or not
        out, t = canary(64), canary(64)
        pl = mirt.abi.PrimaryPlanes(t.ctypes.data, None, None)
        some = np.ascontiguousarray(full[:1])
        for planes in (None, C.byref(pl)):
            ok(gpu, gpu.L.mirt_render_rays(gpu.h, mirt.abi.ptr(some), C.byref(fd), mirt.abi.ptr(out), planes))
            ok(gpu, gpu.L.mirt_render_rays_device(gpu.h, mirt.abi.ptr(some), C.byref(fd), mirt.abi.ptr(out), None,
                                                  planes, None))
        gpu.wait()
        assert (out == 0x5A5A5A5A).all() and (t == 0x5A5A5A5A).all()
    assert sorted(seen) == list(range(height))
    if height == 9:
        assert sum(1 for s in range(3) if not len(mirt.shard_rows(mirt.frame_desc(W, 9, row_block=8, shard=s,
                                                                                  num_shards=3,
                                                                                  lead_skip=lead_skip)))) >= 1


def test_a_shard_row_is_trace_rays_at(gpu, mirt):
    upload(gpu, mirt, rc.N)
    kw = dict(depth=5, seed=7, sample=4, row_block=8, shard=1, num_shards=3)
    rows = mirt.shard_rows(mirt.frame_desc(W, H, **kw))
    rays = np.ascontiguousarray(rc.rays("surface")[rows])
    got = gpu.render_rays(rays, W, H, **kw)
    for r in (0, len(rows) - 1):
        out = np.zeros((W, 4), np.uint8)
        ok(gpu, gpu.L.mirt_trace_rays_at(gpu.h, mirt.abi.ptr(rays[r]), W, 5, 1, 7, 4, int(rows[r]) * W,
                                         mirt.abi.ptr(out)))
        same(got[r], out, f"row {rows[r]}")


@pytest.mark.parametrize("kw", [dict(), dict(row_block=8, shard=1, num_shards=3)], ids=["whole", "shard"])
def test_four_samples_fresh_and_accumulating(gpu, mirt, oracle, kw):
    """samples = 4, a re-sampled lens per slab: fresh, then (after two single
    frames) accumulating with frames = 3; displays and the accumulation buffer
    against Oracle.accumulate slab by slab."""
    upload(gpu, mirt, rc.N)
    rows = mirt.shard_rows(mirt.frame_desc(W, H, **kw))
    n = len(rows) * W
    slabs = np.stack([rc.lens(j)[rows] for j in range(4)])

    def expect(seq):
        """seq: (slab, sample) per frame, the first one fresh -> (display after the last, accumulation)."""
        acc = np.zeros(3 * n, np.float32)
        shown = None
        for k, (j, sample) in enumerate(seq):
            col = rc.colours("lens", seed=5, sample=sample, j=j)[rows]
            shown = oracle.accumulate(col, acc, k == 0, k + 1).reshape(len(rows), W, 4)
        return shown, acc

    got = gpu.render_rays(slabs, W, H, depth=5, seed=5, sample=0, samples=4, **kw)
    shown, acc = expect([(j, j) for j in range(4)])
    same(got, shown, "four fresh samples")
    assert gpu.accum(3 * n).tobytes() == acc.tobytes()
    # frames 0 and 1 one by one (slabs 2 and 3), then four at once as frames 2..5
    gpu.render_rays(slabs[2], W, H, depth=5, seed=5, sample=0, **kw)
    gpu.render_rays(slabs[3], W, H, depth=5, seed=5, sample=1, accumulate=True, frames=2, **kw)
    got = gpu.render_rays(slabs, W, H, depth=5, seed=5, sample=2, samples=4, accumulate=True, frames=3, **kw)
    shown, acc = expect([(2, 0), (3, 1)] + [(j, 2 + j) for j in range(4)])
    same(got, shown, "four accumulating samples")
    assert gpu.accum(3 * n).tobytes() == acc.tobytes()


def test_device_form_on_a_stream_with_an_accumulation_buffer(gpu, mirt, oracle):
    import torch
    upload(gpu, mirt, rc.N)
    n = W * H
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_rays = [torch.from_numpy(np.ascontiguousarray(rc.lens(j)).view(np.uint8).reshape(-1).copy()).to(dev)
              for j in range(2)]
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_acc = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    acc = np.zeros(3 * n, np.float32)
    for k in range(2):
        fd = mirt.frame_desc(W, H, depth=5, seed=2, sample=k, accumulate=k > 0, frames=k + 1)
        gpu.render_rays_device(d_rays[k].data_ptr(), fd, d_out.data_ptr(), d_acc.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        shown = oracle.accumulate(rc.colours("lens", seed=2, sample=k, j=k), acc, k == 0, k + 1)
        assert d_out.cpu().numpy().tobytes() == shown.tobytes(), k
        assert d_acc.cpu().numpy().tobytes() == acc.tobytes(), k


@pytest.mark.parametrize("schedule", ["wavefront_ordered_d5", "primary_only_d1", "tile_d5", "exact_slab_d5",
                                      "brute_force_d5", "brute_force_exact_slab_d5"])
def test_planes(gpu, mirt, schedule):
    depth, use_bvh, opts = schedules(mirt.abi)[schedule]
    upload(gpu, mirt, rc.N)
    with options(gpu, opts):
        for name in ("lens", "surface"):
            rays = rc.rays(name)
            rgba, got = gpu.render_rays(rays, W, H, planes=("t", "sphere", "normal"), depth=depth, use_bvh=use_bvh)
            assert_planes(got, rc.planes(rays, use_bvh), f"{name} on {schedule}")
            same(rgba, gpu.render_rays(rays, W, H, depth=depth, use_bvh=use_bvh), f"{name} on {schedule}")
            same(rgba, rc.colours(name, depth=depth, use_bvh=use_bvh), f"{name} on {schedule} against the oracle")


def test_planes_device_form_writes_only_what_was_asked(gpu, mirt):
    import torch
    upload(gpu, mirt, rc.N)
    n = W * H
    dev = torch.device("cuda", 0)
    rays = rc.rays("surface")
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_s = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gpu.render_rays_device(d_rays.data_ptr(), mirt.frame_desc(W, H, depth=5), d_out.data_ptr(),
                           d_planes={"sphere": d_s.data_ptr()})
    torch.cuda.synchronize()
    assert (d_s.cpu().numpy()[:n] == rc.hit_records("surface")["sphere"].reshape(-1)).all()
    assert bool((d_s[n:] == 0x5A5A5A5A).all())
    assert d_out.cpu().numpy().tobytes() == rc.colours("surface").tobytes()


def test_a_ray_frame_bypasses_the_primary_cache_and_leaves_it_valid(gpu, mirt):
    upload(gpu, mirt, rc.N)
    cam = cases.camera("A")
    with options(gpu, {mirt.abi.OPT_PRIMARY_CACHE: 1}):
        plain = gpu.render_frame(cam, W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["valid"]) == ("fill", 1), st
        got = gpu.render_rays(rc.rays("lens"), W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["valid"]) == ("bypass", "RAYS", 1), st
        same(got, rc.colours("lens"), "lens beside the cache")
        again = gpu.render_frame(cam, W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["hits"], st["fills"], st["bypassed"]) == ("hit", "", 1, 1, 1), st
        same(again, plain, "the frame from the cache")


def test_case_c_lens(gpu, mirt):
    c = cases.CASES["C"]
    upload(gpu, mirt, c["n"])
    rays = rc.lens(0, "C")
    spheres, tree, _ = cases.scene(c["n"])
    want = cases._oracle().trace_rays(np.ascontiguousarray(rays).reshape(-1), spheres, tree, depth=5)
    got = gpu.render_rays(rays, c["W"], c["H"], depth=5)
    same(got, want.reshape(c["H"], c["W"], 4), "case C")
    sphere = rc.cases.planes_of(cases.intersect(c["n"], rays), rays.shape)["sphere"]
    assert (sphere >= 0).any() and (sphere < 0).any()

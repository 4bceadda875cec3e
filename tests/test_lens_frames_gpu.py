"""Lens frames on the GPU (mirt_lens_rays, mirt_render_lens_frame, _device,
_async): depth of field computed in the frame's own camera pass. Byte equality
throughout: mirt_lens_rays with the numpy restatement of the definition
(tests/lens_frame_cases.py), the lens frame with the ray frame of those rays,
with the oracle's trace_ray of the restated rays, and -- at aperture 0 -- with
the plain frame; on every schedule, through shards, several samples,
accumulation, jitter, the device form, frames in flight and the primary cache."""
import ctypes as C

import numpy as np
import pytest

import lens_frame_cases as lc
import ray_frame_cases as rc
import test_planes_cases as cases
from conftest import parse_frame_key, sha
from test_planes_gpu import assert_planes, ok, options, schedules, upload
from test_ray_frames_gpu import GOLDEN_KEY, SCHEDULES, canary, same

pytestmark = pytest.mark.gpu

W, H = lc.W, lc.H
LENSES = sorted(lc.LENSES)
PINHOLE = (0.0, 50.0)
CANARY = 0x5A5A5A5A


def cam_a():
    return cases.camera("A")


@pytest.mark.parametrize("lens", LENSES)
def test_lens_rays_equal_the_restatement(gpu, mirt, lens):
    """Bit for bit, origin and direction: plain, jittered, a shard, and four
    slabs whose sample wraps in uint32."""
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), lc.LENSES[lens]
    lc.same_rays(gpu.lens_rays(cam, L, W, H), lc.lens_rays(lens), "one sample")
    lc.same_rays(gpu.lens_rays(cam, L, W, H, seed=3, sample=2, jitter=True), lc.lens_rays(lens, 3, 2, True), "jittered")
    for jitter in (False, True):
        kw = dict(seed=3, sample=0xFFFFFFFE, samples=4, jitter=jitter)
        lc.same_rays(gpu.lens_rays(cam, L, W, H, **kw), lc.slabs(lens, **kw), f"four slabs, jitter {jitter}")
        for shard in range(3):
            skw = dict(row_block=8, shard=shard, num_shards=3, lead_skip=1)
            rows = mirt.shard_rows(mirt.frame_desc(W, H, **skw))
            lc.same_rays(gpu.lens_rays(cam, L, W, H, **kw, **skw), lc.slabs(lens, rows=rows, **kw),
                         f"shard {shard}, jitter {jitter}")


@pytest.mark.parametrize("lens", LENSES)
@pytest.mark.parametrize("depth", [0, 1, 2, 5, 8])
def test_the_contract(gpu, mirt, lens, depth):
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), lc.LENSES[lens]
    rays = gpu.lens_rays(cam, L, W, H)
    lc.same_rays(rays, lc.lens_rays(lens), "mirt_lens_rays")
    got = gpu.render_lens_frame(cam, L, W, H, depth=depth)
    same(got, gpu.render_rays(rays, W, H, depth=depth), f"depth {depth} against the ray frame")
    same(got, lc.colours(lens, depth=depth), f"depth {depth} against the oracle")
    if depth == 0:
        assert (got == np.array([0, 0, 0, 255], np.uint8)).all()
        return
    rgba, planes = gpu.render_lens_frame(cam, L, W, H, planes=("t", "sphere", "normal"), depth=depth)
    same(rgba, got, f"depth {depth} with planes")
    hits = gpu.closest_hit(np.ascontiguousarray(rays).reshape(-1))
    assert_planes(planes, cases.planes_of(hits, (H, W)), f"depth {depth} against mirt_intersect_rays")
    assert_planes(planes, rc.planes(lc.lens_rays(lens)), f"depth {depth} against the oracle's hits")
    assert (planes["sphere"] >= 0).any() and (planes["sphere"] < 0).any()
    # aperture 0 is the plain frame
    same(gpu.render_lens_frame(cam, PINHOLE, W, H, depth=depth), gpu.render_frame(cam, W, H, depth=depth), "aperture 0")


def test_aperture_zero_gives_the_golden_frame(gpu, mirt, golden, small):
    p = parse_frame_key(GOLDEN_KEY)
    s = mirt.create_random_spheres(p["n"], 1)
    gpu.upload(s, mirt.build_bvh(s))
    cam = mirt.abi.Camera.from_numpy(small["cameras"][p["cam"]])
    got = gpu.render_lens_frame(cam, PINHOLE, p["W"], p["H"], depth=p["depth"], use_bvh=p["use_bvh"], seed=p["seed"])
    assert sha(got[::p["step"]]) == golden["frames"][GOLDEN_KEY]["sha"]


def test_aperture_zero_in_every_form(gpu, mirt):
    import torch
    upload(gpu, mirt, lc.N)
    cam = cam_a()
    kw = dict(depth=5, seed=3, sample=2, jitter=True)
    fd = mirt.frame_desc(W, H, **kw)
    want = gpu.render_frame(cam, W, H, **kw)
    want_rgba, want_planes = gpu.render_frame_planes(cam, W, H, **kw)
    same(want_rgba, want, "the plain frame with planes")
    same(gpu.render_lens_frame(cam, PINHOLE, W, H, **kw), want, "blocking")
    rgba, planes = gpu.render_lens_frame(cam, PINHOLE, W, H, planes=("t", "sphere", "normal"), **kw)
    same(rgba, want, "blocking with planes")
    assert_planes(planes, want_planes, "blocking with planes")
    rays = np.zeros((H, W), mirt.abi.RAY)
    ok(gpu, gpu.L.mirt_camera_rays(gpu.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(rays)))
    assert gpu.lens_rays(cam, PINHOLE, W, H, **kw).tobytes() == rays.tobytes()
    buf, t = mirt.HostBuffer((H, W, 4)), np.zeros((H, W), np.float32)
    try:
        gpu.render_lens_frame_async(cam, PINHOLE, fd, buf)
        gpu.wait()
        same(buf.array, want, "async")
        buf.array[:] = 0
        gpu.render_lens_frame_async(cam, PINHOLE, fd, buf, planes={"t": t})
        gpu.wait()
        same(buf.array, want, "async with planes")
        assert t.tobytes() == want_planes["t"].tobytes()
    finally:
        buf.close()
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(W * H, dtype=torch.int32, device=dev)
    d_s = torch.zeros(W * H, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for d_planes in (None, {"sphere": d_s.data_ptr()}):
        d_out.zero_()
        torch.cuda.synchronize()
        gpu.render_lens_frame_device(cam, PINHOLE, fd, d_out.data_ptr(), d_planes=d_planes)
        gpu.wait()
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want.tobytes(), d_planes
    assert d_s.cpu().numpy().tobytes() == want_planes["sphere"].tobytes()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_every_schedule(gpu, mirt, schedule):
    depth, use_bvh, opts = schedules(mirt.abi)[schedule]
    upload(gpu, mirt, lc.N)
    with options(gpu, opts):
        for lens in LENSES:
            got = gpu.render_lens_frame(cam_a(), lc.LENSES[lens], W, H, depth=depth, use_bvh=use_bvh)
            same(got, lc.colours(lens, depth=depth, use_bvh=use_bvh), f"{lens} on {schedule}")
        rgba, planes = gpu.render_lens_frame(cam_a(), lc.LENS, W, H, planes=("t", "sphere", "normal"), depth=depth,
                                             use_bvh=use_bvh)
        same(rgba, lc.colours("lens", depth=depth, use_bvh=use_bvh), f"planes on {schedule}")
        assert_planes(planes, rc.planes(lc.lens_rays("lens"), use_bvh), f"planes on {schedule}")


@pytest.mark.parametrize("height,lead_skip", [(H, 0), (H, 1), (9, 0), (9, 1)])
def test_shards(gpu, mirt, height, lead_skip):
    """Shards 0..2 of 3 at row_block 8 equal their rows of the full lens frame;
    at height 9 some shards are empty: MIRT_OK, nothing written."""
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), mirt.abi.Lens(*lc.LENS)
    full = gpu.render_lens_frame(cam, L, W, height, depth=5, seed=3, sample=2)
    if height == H:
        same(full, lc.colours("lens", seed=3, sample=2), "the full frame against the oracle")
    seen, empty = [], 0
    for shard in range(3):
        kw = dict(depth=5, seed=3, sample=2, row_block=8, shard=shard, num_shards=3, lead_skip=lead_skip)
        fd = mirt.frame_desc(W, height, **kw)
        rows = mirt.shard_rows(fd)
        seen += list(rows)
        if len(rows):
            same(gpu.render_lens_frame(cam, L, W, height, **kw), full[rows],
                 f"shard {shard} of height {height}, lead_skip {lead_skip}")
            continue
        empty += 1
        out, t, r = canary(64), canary(64), canary(64)
        pl = mirt.abi.PrimaryPlanes(t.ctypes.data, None, None)
        for planes in (None, C.byref(pl)):
            ok(gpu, gpu.L.mirt_render_lens_frame(gpu.h, C.byref(cam), C.byref(L), C.byref(fd), mirt.abi.ptr(out),
                                                 planes))
            ok(gpu, gpu.L.mirt_render_lens_frame_async(gpu.h, C.byref(cam), C.byref(L), C.byref(fd),
                                                       mirt.abi.ptr(out), planes))
            ok(gpu, gpu.L.mirt_render_lens_frame_device(gpu.h, C.byref(cam), C.byref(L), C.byref(fd),
                                                        mirt.abi.ptr(out), None, planes, None))
        ok(gpu, gpu.L.mirt_lens_rays(gpu.h, C.byref(cam), C.byref(L), C.byref(fd), mirt.abi.ptr(r)))
        gpu.wait()
        assert (out == CANARY).all() and (t == CANARY).all() and (r == CANARY).all()
    assert sorted(seen) == list(range(height))
    assert empty >= 1 if height == 9 else empty == 0


@pytest.mark.parametrize("kw", [dict(), dict(row_block=8, shard=1, num_shards=3)], ids=["whole", "shard"])
def test_four_samples_fresh_and_accumulating(gpu, mirt, oracle, kw):
    """samples = 4, fresh and (after two single frames) accumulating: equal to
    four successive one-sample lens frames, to the ray frame of the four slabs
    of mirt_lens_rays, and to the oracle's accumulation of the restated rays'
    colours; displays and the accumulation buffer."""
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), lc.LENS
    rows = mirt.shard_rows(mirt.frame_desc(W, H, **kw))
    n = len(rows) * W
    base = dict(depth=5, seed=5, **kw)

    def expect(samples):
        acc = np.zeros(3 * n, np.float32)
        shown = None
        for k, sample in enumerate(samples):
            col = lc.colours("lens", seed=5, sample=sample)[rows]
            shown = oracle.accumulate(col, acc, k == 0, k + 1).reshape(len(rows), W, 4)
        return shown, acc

    # fresh
    got = gpu.render_lens_frame(cam, L, W, H, sample=0, samples=4, **base)
    acc_got = gpu.accum(3 * n)
    shown, acc = expect(range(4))
    same(got, shown, "four fresh samples against the oracle")
    assert acc_got.tobytes() == acc.tobytes()
    slabs = gpu.lens_rays(cam, L, W, H, sample=0, samples=4, **base)
    same(gpu.render_rays(slabs, W, H, sample=0, samples=4, **base), got, "the ray frame of the four slabs")
    assert gpu.accum(3 * n).tobytes() == acc.tobytes()
    for k in range(4):
        one = gpu.render_lens_frame(cam, L, W, H, sample=k, accumulate=k > 0, frames=k + 1, **base)
    same(one, got, "four successive one-sample lens frames")
    assert gpu.accum(3 * n).tobytes() == acc.tobytes()
    # frames 0 and 1 one by one, then four at once as frames 2..5
    gpu.render_lens_frame(cam, L, W, H, sample=0, **base)
    gpu.render_lens_frame(cam, L, W, H, sample=1, accumulate=True, frames=2, **base)
    got = gpu.render_lens_frame(cam, L, W, H, sample=2, samples=4, accumulate=True, frames=3, **base)
    shown, acc = expect(range(6))
    same(got, shown, "four accumulating samples")
    assert gpu.accum(3 * n).tobytes() == acc.tobytes()


@pytest.mark.parametrize("lens", LENSES)
def test_a_jittered_lens_frame_is_the_ray_frame_of_its_jittered_rays(gpu, mirt, lens):
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), lc.LENSES[lens]
    for kw in (dict(), dict(samples=4), dict(row_block=8, shard=2, num_shards=3)):
        base = dict(depth=5, seed=3, sample=1, **kw)
        rays = gpu.lens_rays(cam, L, W, H, jitter=True, **base)
        got = gpu.render_lens_frame(cam, L, W, H, jitter=True, **base)
        same(got, gpu.render_rays(rays, W, H, **base), f"jittered, {kw}")   # jitter cleared for the ray frame only
        if not kw:
            lc.same_rays(rays, lc.lens_rays(lens, 3, 1, True), "jittered rays")
            same(got, lc.colours(lens, seed=3, sample=1, jitter=True), "jittered against the oracle")
            assert (got != gpu.render_lens_frame(cam, L, W, H, **base)).any()


def test_device_form_on_a_stream_with_planes_and_canaries(gpu, mirt, oracle):
    """Width 43 (tiles overhang), a caller's stream, a caller's d_accum over two
    accumulating launches of two samples, device planes; canaries behind every
    output."""
    import torch
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), lc.LENS
    w, S = 43, 2
    n = w * H
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def buf(count, dtype):
        return torch.full((count + 64,), CANARY, dtype=torch.int32, device=dev).view(dtype)

    d_out, d_acc = buf(S * n, torch.int32), buf(3 * n, torch.float32)
    d_t, d_s, d_n = buf(S * n, torch.float32), buf(S * n, torch.int32), buf(3 * S * n, torch.float32)
    torch.cuda.synchronize()
    acc = np.zeros(3 * n, np.float32)
    spheres, tree, _ = cases.scene(lc.N)
    for launch in range(2):
        kw = dict(depth=5, seed=2, sample=S * launch, samples=S, accumulate=launch > 0, frames=S * launch + 1)
        fd = mirt.frame_desc(w, H, **kw)
        gpu.render_lens_frame_device(cam, L, fd, d_out.data_ptr(), d_acc.data_ptr(),
                                     d_planes={"t": d_t.data_ptr(), "sphere": d_s.data_ptr(), "normal": d_n.data_ptr()},
                                     stream=stream.cuda_stream)
        stream.synchronize()
        rays = gpu.lens_rays(cam, L, w, H, **kw)
        for j in range(S):
            k = S * launch + j
            col = oracle.trace_rays(np.ascontiguousarray(rays[j]).reshape(-1), spheres, tree, depth=5, seed=2, sample=k)
            shown = oracle.accumulate(col, acc, k == 0, k + 1)
            assert d_out.cpu().numpy()[j * n:(j + 1) * n].tobytes() == shown.tobytes(), k
        assert d_acc.cpu().numpy()[:3 * n].tobytes() == acc.tobytes(), launch
        want = rc.planes(rays)
        got = {"t": d_t.cpu().numpy()[:S * n].reshape(S, H, w), "sphere": d_s.cpu().numpy()[:S * n].reshape(S, H, w),
               "normal": d_n.cpu().numpy()[:3 * S * n].reshape(S, H, w, 3)}
        assert_planes(got, want, f"launch {launch}")
    for name, d, used in (("out", d_out, S * n), ("acc", d_acc, 3 * n), ("t", d_t, S * n), ("sphere", d_s, S * n),
                          ("normal", d_n, 3 * S * n)):
        assert bool((d.view(torch.int32)[used:] == CANARY).all()), name


@pytest.mark.parametrize("zero_copy", [2, 0])
def test_frames_in_flight_on_three_contexts(gpu, mirt, zero_copy):
    """The accumulating display loop (main.c:379-408) through a lens: three
    rotated contexts on one accumulation buffer, mirt_render_lens_frame_async
    into page-locked memory, 12 frames; every delivered frame equals the
    blocking loop's."""
    upload(gpu, mirt, lc.N)
    cam, L, F = cam_a(), lc.LENS, 12
    spheres, _, nodes = cases.scene(lc.N)
    want = [gpu.render_lens_frame(cam, L, W, H, depth=5, seed=4, sample=k, accumulate=k > 0, frames=k + 1)
            for k in range(F)]
    same(want[0], lc.colours("lens", seed=4, sample=0), "the first frame against the oracle")
    acc_want = gpu.accum(3 * W * H)
    rs = [mirt.Renderer(0) for _ in range(3)]
    bufs = [mirt.HostBuffer((H, W, 4)) for _ in rs]
    try:
        for x in rs:
            x.upload(spheres, mirt.Bvh(nodes))
            x.share_accum(rs[0])
            x.set_option(mirt.abi.OPT_ZERO_COPY, zero_copy)
        got = [None] * F
        for k in range(F):
            i = k % 3
            rs[i].wait()
            if k >= 3:
                got[k - 3] = bufs[i].array.copy()
            fd = mirt.frame_desc(W, H, depth=5, seed=4, sample=k, accumulate=k > 0, frames=k + 1)
            rs[i].render_lens_frame_async(cam, L, fd, bufs[i])
        for k in range(F - 3, F):
            rs[k % 3].wait()
            got[k] = bufs[k % 3].array.copy()
        for k in range(F):
            same(got[k], want[k], f"frame {k}, zero copy {zero_copy}")
        assert rs[1].accum(3 * W * H).tobytes() == acc_want.tobytes()
    finally:
        for x in bufs:
            x.close()
        for x in rs:
            x.close()


def test_zero_copy_in_place_without_a_chain(gpu, mirt):
    """MIRT_OPT_ZERO_COPY 2, a private accumulation buffer: the lens kernels
    store straight into the page-locked frame."""
    upload(gpu, mirt, lc.N)
    cam, L = cam_a(), lc.LENS
    buf = mirt.HostBuffer((H, W, 4))
    try:
        with options(gpu, {mirt.abi.OPT_ZERO_COPY: 2}):
            for k in range(3):
                gpu.render_lens_frame_async(cam, L, mirt.frame_desc(W, H, depth=5, seed=4, sample=k), buf)
                gpu.wait()
                same(buf.array, lc.colours("lens", seed=4, sample=k), f"frame {k}")
    finally:
        buf.close()


def test_the_primary_cache(gpu, mirt):
    upload(gpu, mirt, lc.N)
    cam = cam_a()
    with options(gpu, {mirt.abi.OPT_PRIMARY_CACHE: 1}):
        plain = gpu.render_frame(cam, W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["valid"]) == ("fill", 1), st
        got = gpu.render_lens_frame(cam, lc.LENS, W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["valid"]) == ("bypass", "LENS", 1), st
        same(got, lc.colours("lens"), "the lens frame beside the cache")
        # aperture 0 is a plain frame: a hit
        again = gpu.render_lens_frame(cam, (0.0, 50.0), W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["hits"], st["fills"], st["bypassed"]) == ("hit", "", 1, 1, 1), st
        same(again, plain, "the aperture-0 frame from the cache")
        # a jittered lens frame is refused for its jitter first (the order of the enum)
        gpu.render_lens_frame(cam, lc.LENS, W, H, depth=5, jitter=True)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["valid"]) == ("bypass", "JITTER", 1), st

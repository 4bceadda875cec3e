"""Lens frames through mirt_multi (mirt_multi_render_lens_frames_async): only
the 8-byte lens travels to the ranks, each of which computes its rows' rays in
its own camera pass. Same-device ranks, gather and host-direct delivery, lanes
in flight, several frames per launch, fresh and accumulating, with rank 0's
lighter share: every delivered frame equals the single-context lens frame."""
import numpy as np
import pytest

import lens_frame_cases as lc
import test_planes_cases as cases
from test_planes_gpu import upload
from test_ray_frames_gpu import same

pytestmark = pytest.mark.gpu

W, H, F = lc.W, lc.H, 8
PINHOLE = (0.0, 50.0)


def single(gpu, mirt, lens, accumulate):
    """Frames 0 .. F - 1 of one context: fresh frames, or the accumulating loop."""
    upload(gpu, mirt, lc.N)
    cam = cases.camera("A")
    if lens[0] == 0.0:
        return [gpu.render_frame(cam, W, H, depth=5, seed=4, sample=k, accumulate=accumulate and k > 0,
                                 frames=k + 1 if accumulate else 1) for k in range(F)]
    return [gpu.render_lens_frame(cam, lens, W, H, depth=5, seed=4, sample=k, accumulate=accumulate and k > 0,
                                  frames=k + 1 if accumulate else 1) for k in range(F)]


@pytest.mark.parametrize("devices,direct", [([0, 0], False), ([0, 0], True), ([0, 0, 0], False), ([0, 0, 0], True)])
@pytest.mark.parametrize("lanes,lead_skip", [(1, 0), (3, 3)])
def test_launches_of_four_frames_equal_one_context(gpu, mirt, devices, direct, lanes, lead_skip):
    spheres, _, nodes = cases.scene(lc.N)
    cam, L = cases.camera("A"), lc.LENS
    want_fresh = single(gpu, mirt, L, False)
    same(want_fresh[0], lc.colours("lens", seed=4, sample=0), "one context against the oracle")
    want_acc = single(gpu, mirt, L, True)
    bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(F)]
    try:
        with mirt.MultiRenderer(devices, lanes=lanes, host_direct=direct) as m:
            m.set_option(mirt.abi.MULTI_OPT_LEAD_SKIP, lead_skip)
            m.upload(spheres, mirt.Bvh(nodes))
            for f0 in range(0, F, 4):   # fresh: two launches of four frames
                m.render_lens_frames_async(cam, L, mirt.frame_desc(W, H, depth=5, seed=4, sample=f0), bufs[f0:f0 + 4])
            m.wait()
            for k in range(F):
                same(bufs[k].array, want_fresh[k], f"fresh frame {k}")
            # the accumulating loop: a fresh frame, then launches of accumulating ones
            m.render_lens_frames_async(cam, L, mirt.frame_desc(W, H, depth=5, seed=4, sample=0), bufs[:1])
            m.render_lens_frames_async(cam, L, mirt.frame_desc(W, H, depth=5, seed=4, sample=1, accumulate=True,
                                                               frames=2), bufs[1:4])
            m.render_lens_frames_async(cam, L, mirt.frame_desc(W, H, depth=5, seed=4, sample=4, accumulate=True,
                                                               frames=5), bufs[4:8])
            m.wait()
            for k in range(F):
                same(bufs[k].array, want_acc[k], f"accumulating frame {k}")
    finally:
        for x in bufs:
            x.close()


def test_aperture_zero_is_the_plain_launch(gpu, mirt):
    spheres, _, nodes = cases.scene(lc.N)
    cam = cases.camera("A")
    want = single(gpu, mirt, PINHOLE, False)
    bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(8)]
    try:
        with mirt.MultiRenderer([0, 0], lanes=2) as m:
            m.upload(spheres, mirt.Bvh(nodes))
            fd = mirt.frame_desc(W, H, depth=5, seed=4, sample=0)
            m.render_lens_frames_async(cam, PINHOLE, fd, bufs[:4])
            m.render_frames_async(cam, fd, bufs[4:])
            m.wait()
            for k in range(4):
                same(bufs[k].array, bufs[4 + k].array, f"frame {k} against the plain launch")
                same(bufs[k].array, want[k], f"frame {k} against one context")
    finally:
        for x in bufs:
            x.close()


def test_a_sharded_descriptor_and_an_invalid_lens_are_rejected(mirt):
    spheres, _, nodes = cases.scene(lc.N)
    cam = cases.camera("A")
    with mirt.MultiRenderer([0, 0]) as m:
        m.upload(spheres, mirt.Bvh(nodes))
        out = np.zeros((H, W, 4), np.uint8)
        for lens in (lc.LENS, PINHOLE):
            with pytest.raises(mirt.MirtError):
                m.render_lens_frames_async(cam, lens, mirt.frame_desc(W, H, shard=1, num_shards=2), [out])
            with pytest.raises(mirt.MirtError):   # several frames need one sample per frame
                m.render_lens_frames_async(cam, lens, mirt.frame_desc(W, H, samples=2), [out, out.copy()])
        with pytest.raises(mirt.MirtError):
            m.render_lens_frames_async(cam, (-1.0, 50.0), mirt.frame_desc(W, H), [out])
        assert not out.any() and not m.failed

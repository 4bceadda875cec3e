"""Every place the wavefront schedule samples a bounce direction, against the
oracle's frame, byte for byte: the camera pass (tiles where every, some and no
pixel hits, a ragged tile edge at 72x24), the bounce pass's main loop (the
wave samples together, hemisphere_wave; refill thresholds 1, 20 and 64: sparse
to full shade passes), its quad drain and the solo chain that ends it (or
neither, with the drain off), with one frame and four frames per launch (the
row mapping's divisions by shard_rows). The frames are the smallest at which
all of these run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_refs = {}


def _setup(mirt, oracle, n):
    """The scene as the renderer holds it and the oracle's frames of it."""
    if n not in _refs:
        s = mirt.create_random_spheres(n, 1)
        b = mirt.build_bvh(s)
        so = mirt.create_random_spheres(n, 1)
        _refs[n] = (s, b, so, oracle.build(so), {})
    return _refs[n]


@pytest.fixture(scope="module", autouse=True)
def _free_trees(oracle):
    yield
    for entry in _refs.values():
        oracle.free(entry[3])
    _refs.clear()


def _ref(mirt, oracle, n, W, H, depth, sample):
    _, _, so, tree, frames = _setup(mirt, oracle, n)
    key = (W, H, depth, sample)
    if key not in frames:
        frames[key] = oracle.render(mirt.default_camera(), W, H, so, tree, depth=depth, mode=1, seed=3, sample=sample)
    return frames[key]


@pytest.mark.parametrize("depth", [2, 5])
@pytest.mark.parametrize("n", [100, 1000])
@pytest.mark.parametrize("W,H", [(64, 40), (72, 24)])
def test_shade_sites_match_oracle(gpu, mirt, oracle, W, H, n, depth):
    import torch
    abi = mirt.abi
    s, b = _setup(mirt, oracle, n)[:2]
    gpu.upload(s, b)
    cam = mirt.default_camera()
    old = gpu.get_option(abi.OPT_BOUNCE_THRESHOLD), gpu.get_option(abi.OPT_QUAD_DRAIN)
    try:
        for threshold in (1, 20, 64):
            for drain in (0, 1):
                gpu.set_option(abi.OPT_BOUNCE_THRESHOLD, threshold)
                gpu.set_option(abi.OPT_QUAD_DRAIN, drain)
                one = gpu.render_frame(cam, W, H, depth=depth, seed=3)
                assert (one == _ref(mirt, oracle, n, W, H, depth, 0)).all(), (threshold, drain)
                # four frames in one launch, each left raw in its slab
                fd = mirt.frame_desc(W, H, depth=depth, seed=3, sample=0, samples=4)
                out = torch.zeros((4, H, W), dtype=torch.int32, device="cuda")
                gpu.render_frame_device(cam, fd, out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = out.cpu().numpy().view(np.uint8).reshape(4, H, W, 4)
                for j in range(4):
                    assert (got[j] == _ref(mirt, oracle, n, W, H, depth, j)).all(), (threshold, drain, j)
    finally:
        gpu.set_option(abi.OPT_BOUNCE_THRESHOLD, old[0])
        gpu.set_option(abi.OPT_QUAD_DRAIN, old[1])

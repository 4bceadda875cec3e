"""mirt_camera_rays_uv (get_camera_ray at caller-given (u, v), batched): on the
pixel grid against the oracle's camera rays, across workgroup boundaries with a
canary behind the output, at arbitrary and non-finite (u, v) against a float32
restatement of camera_uv_kernel (tests/overlay_cases.py uv_rays) that is first
checked against the oracle, and the arguments. Rays compare byte for byte; a
float that is a NaN in the restatement must be a NaN on the device (the rule of
tests/test_hostile_rays_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import overlay_cases as oc

pytestmark = pytest.mark.gpu

E_INVALID = -1


def floats(rays):
    return np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6)


def same_rays(got, want, what):
    """Byte for byte where the reference float is no NaN, a NaN where it is; returns the number of NaN floats."""
    g, w = floats(got), floats(want)
    assert g.shape == w.shape, what
    nan = np.isnan(w)
    bad = np.where(nan, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32))
    assert not bad.any(), f"{what}: {int(bad.any(1).sum())} rays differ, first {int(np.argwhere(bad)[0][0])}: " \
                          f"{g[np.argwhere(bad)[0][0]]} != {w[np.argwhere(bad)[0][0]]}"
    return int(nan.sum())


@pytest.mark.parametrize("size", oc.UV_SIZES)
def test_the_pixel_grid_gives_the_oracles_camera_rays(gpu, oracle, small, size):
    w, h = size
    for name, cam in oc.uv_cameras(small).items():
        got = gpu.camera_rays_uv(cam, w, h, oc.pixel_uv(w, h).reshape(-1, 2)).reshape(h, w)
        want = oracle.camera_rays(cam, w, h)
        assert got.tobytes() == want.tobytes(), (name, size)
        if size == (77, 45):    # and the frame's own rays
            assert gpu.get_camera_rays(cam, w, h).tobytes() == want.tobytes(), name


def test_batch_sizes_and_the_canary(gpu, mirt, oracle):
    """n on both sides of a workgroup (256) and a grid of several, as prefixes
    of one list, through the C entry point into a buffer with a canary behind."""
    L = mirt.load()
    cam = mirt.default_camera()
    w, h = 160, 90
    uv = np.ascontiguousarray(oc.pixel_uv(w, h).reshape(-1, 2)[:max(oc.UV_BATCHES)])
    want = np.ascontiguousarray(oracle.camera_rays(cam, w, h)).reshape(-1)[:len(uv)]
    for n in oc.UV_BATCHES:
        out = np.zeros(n + 64, mirt.abi.RAY)
        raw = out.view(np.uint8)
        raw[:] = 0xA5
        assert L.mirt_camera_rays_uv(gpu.h, C.byref(cam), w, h, mirt.abi.ptr(uv), n, mirt.abi.ptr(out)) == 0
        assert out[:n].tobytes() == want[:n].tobytes(), n
        assert (out[n:].view(np.uint8) == 0xA5).all(), n


def test_arbitrary_and_non_finite_uv(gpu, oracle, small):
    cams = oc.uv_cameras(small)
    # the restatement is the oracle's on the pixel grid: it is not the code under test checking itself
    for name, cam in cams.items():
        got = oc.uv_rays(cam, 77, 45, oc.pixel_uv(77, 45))
        assert got.tobytes() == oracle.camera_rays(cam, 77, 45).tobytes(), name
    uv = oc.hostile_uv()
    nans = 0
    for name, cam in cams.items():
        for w, h in ((160, 90), (1, 1)):
            nans += same_rays(gpu.camera_rays_uv(cam, w, h, uv), oc.uv_rays(cam, w, h, uv), f"{name} {w} x {h}")
    assert nans > 300
    # a skewed, a zero and a non-finite camera: the fields are used as given
    for name in ("skew", "fwd_zero", "fwd_1e20", "pos_nan", "pos_inf", "fov_nan", "fov180", "fov0", "fov-45"):
        cam = oc.camera(name)
        same_rays(gpu.camera_rays_uv(cam, 160, 90, uv), oc.uv_rays(cam, 160, 90, uv), name)


def test_arguments(mirt):
    L = mirt.load()
    abi = mirt.abi
    cam = mirt.default_camera()
    uv = np.zeros((4, 2), np.float32)
    out = np.zeros(4, abi.RAY)
    out.view(np.uint8)[:] = 0x5A
    call = lambda r, c, w, h, u, n, o: L.mirt_camera_rays_uv(r.h, C.byref(c) if c is not None else None, w, h, u, n, o)
    with mirt.Renderer(0) as r:    # needs no scene
        p_uv, p_out = abi.ptr(uv), abi.ptr(out)
        assert call(r, cam, 16, 9, p_uv, 0, p_out) == 0
        assert call(r, cam, 16, 9, None, 0, None) == 0
        assert call(r, cam, 16, 9, p_uv, -1, p_out) == E_INVALID
        assert call(r, cam, 16, 9, p_uv, oc.INT_MIN, p_out) == E_INVALID
        assert call(r, None, 16, 9, p_uv, 4, p_out) == E_INVALID
        assert call(r, cam, 16, 9, None, 4, p_out) == E_INVALID
        assert call(r, cam, 16, 9, p_uv, 4, None) == E_INVALID
        for w, h in ((0, 9), (16, 0), (-16, 9), (16, -9)):
            assert call(r, cam, w, h, p_uv, 4, p_out) == E_INVALID, (w, h)
        assert b"mirt_camera_rays_uv" in L.mirt_last_error()
        assert (out.view(np.uint8) == 0x5A).all()
        assert call(r, cam, 16, 9, p_uv, 4, p_out) == 0
        assert out.tobytes() == oc.uv_rays(cam, 16, 9, uv).tobytes()

"""The lens frames' definition (csrc/lens.h, mirt.h mirt_lens) restated in
numpy, one float32 operation per operation of the definition and in its order,
and what a lens frame must show, from the oracle alone (no GPU).

For pixel (x, y) of RNG sample s of a W x H frame:

  key       = pixel_key(seed, y * W + x, s)
  (p, d)    = the pinhole's ray (the oracle's camera ray; under jitter the
              restated camera ray of the displaced sample point)
  (a, b)    = the first of 16 tries i with a * a + b * b < 1, a and b from draws
              0x7fffff00 + 2i and + 2i + 1, each (float)draw / 2^31 * 2 - 1;
              (0, 0) if none
  origin    = (p + L * a) + U * b, L = right * aperture, U = up * aperture
  direction = normalised ((p + d * focus) - origin)

The frame is test_planes_cases' case A (44 x 26 over scene(1000)); LENS is the
lens under test, WIDE one whose origins leave the tiles' coherence.
tests/test_lens_frames_host.py asserts that the cases cover their ground;
tests/test_lens_frames_gpu.py and test_lens_frames_multi.py render them.
"""
import functools

import numpy as np

import test_planes_cases as cases
from test_hemisphere_wave import draw, pixel_key

abi = cases.abi
F32, U64 = np.float32, np.uint64
W, H, N = 44, 26, 1000
LENS, WIDE = (0.5, 50.0), (4.0, 50.0)
LENSES = {"lens": LENS, "wide": WIDE}
LENS_DRAW0, JITTER_X, JITTER_Y, TRIES = 0x7FFFFF00, 0x7FFFFFF0, 0x7FFFFFF1, 16


def _vec(v):
    return np.array([v.x, v.y, v.z], F32)


def _unit(k, key):
    return draw(key, k).astype(F32) / F32(2147483648.0)


def keys(seed, sample, w=W, h=H):
    """The (h, w) contract keys of a full frame; `sample` wraps in uint32."""
    pixel = (np.arange(h, dtype=U64)[:, None] * U64(w) + np.arange(w, dtype=U64)[None, :])
    return pixel_key(U64(seed), pixel, U64(int(sample) & 0xFFFFFFFF))


def lens_points(key):
    """(a, b, tries): the accepted point of every key and the number of tries
    it took (TRIES + 1: none was accepted, the point is the centre)."""
    a = np.zeros(key.shape, F32)
    b = np.zeros(key.shape, F32)
    tries = np.full(key.shape, TRIES + 1, np.int32)
    for i in range(TRIES):
        ta = _unit(LENS_DRAW0 + 2 * i, key) * F32(2.0) - F32(1.0)
        tb = _unit(LENS_DRAW0 + 2 * i + 1, key) * F32(2.0) - F32(1.0)
        q = ta * ta
        q = q + tb * tb
        take = (tries > TRIES) & (q < F32(1.0))
        a, b = np.where(take, ta, a), np.where(take, tb, b)
        tries = np.where(take, i + 1, tries)
    return a, b, tries


def normalize(n):
    """The kernels' normalize3 (trace.h): zero for a zero length."""
    sq = n[..., 0] * n[..., 0]
    sq = sq + n[..., 1] * n[..., 1]
    sq = sq + n[..., 2] * n[..., 2]
    length = np.sqrt(sq)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = n / length[..., None]
    return np.where(length[..., None] != 0, out, F32(0.0)).astype(F32)


def pinhole(cam, key=None, w=W, h=H):
    """The camera rays of a full frame restated (render.hip camera_ray, oracle.c
    o_camera_ray_px): (origin, direction). key: the frame's keys, for a
    jittered frame's displaced sample points."""
    xf = np.broadcast_to(np.arange(w, dtype=F32)[None, :], (h, w))
    yf = np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w))
    if key is not None:
        xf = xf + _unit(JITTER_X, key)
        yf = yf + _unit(JITTER_Y, key)
    aspect = F32(w) / F32(h)
    fov_rad = F32(np.float64(cam.fov) * (np.pi / 180.0))
    half_h = F32(np.tan(np.float64(fov_rad / F32(2.0))))
    half_w = aspect * half_h
    hor = _vec(cam.right) * (F32(2.0) * half_w)
    ver = _vec(cam.up) * (F32(2.0) * half_h)
    u = (xf / F32(w) - F32(0.5)) * aspect
    v = -(yf / F32(h) - F32(0.5))
    d = _vec(cam.forward) + hor * u[..., None]
    d = d + ver * v[..., None]
    return np.broadcast_to(_vec(cam.position), (h, w, 3)), normalize(d.astype(F32))


def _rays(origin, direction):
    out = np.zeros(origin.shape[:-1], abi.RAY)
    out["origin"], out["direction"] = origin, direction
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lens_rays(lens="lens", seed=1, sample=0, jitter=False, case="A"):
    """The (H, W) abi.RAY rays of a full lens frame of one sample, restated."""
    aperture, focus = LENSES[lens]
    c = cases.CASES[case]
    cam = cases.camera(case)
    key = keys(seed, sample, c["W"], c["H"])
    if jitter:
        p, d = pinhole(cam, key, c["W"], c["H"])
    else:
        pin = cases.rays(case)   # the oracle's
        p, d = pin["origin"], pin["direction"]
    a, b, _ = lens_points(key)
    L = _vec(cam.right) * F32(aperture)
    U = _vec(cam.up) * F32(aperture)
    o = (p + L * a[..., None]) + U * b[..., None]
    f = p + d * F32(focus)
    return _rays(o.astype(F32), normalize((f - o).astype(F32)))


def slabs(lens="lens", seed=1, sample=0, samples=1, jitter=False, rows=None):
    """(samples, rows, W): slab j is RNG sample sample + j (in uint32)."""
    out = np.stack([lens_rays(lens, seed, (sample + j) & 0xFFFFFFFF, jitter) for j in range(samples)])
    return out if rows is None else np.ascontiguousarray(out[:, rows])


@functools.lru_cache(maxsize=None)
def colours(lens="lens", depth=5, use_bvh=True, seed=1, sample=0, jitter=False):
    """The full frame (H, W, 4) the oracle traces from the restated rays."""
    spheres, tree, _ = cases.scene(N)
    r = np.ascontiguousarray(lens_rays(lens, seed, sample, jitter)).reshape(-1)
    out = cases._oracle().trace_rays(r, spheres, tree, depth=depth, use_bvh=use_bvh, seed=seed,
                                     sample=sample).reshape(H, W, 4)
    out.setflags(write=False)
    return out


def same_rays(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for part in ("origin", "direction"):
        diff = (np.ascontiguousarray(got[part]).view(np.uint32) != np.ascontiguousarray(want[part]).view(np.uint32))
        assert not diff.any(), f"{what}: {int(diff.any(axis=-1).sum())} of {diff[..., 0].size} {part}s differ"

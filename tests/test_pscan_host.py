"""The arithmetic of the primary scan on the CPU (csrc/pscan.h through
mirt_pscan_camera / mirt_pscan_records: the code the kernels compile).

The scan is exact when, for every pixel whose camera ray records a hit (t, s),
  1. the pixel's 8x8 tile lies in the rectangle of s's record, and
  2. the record's depth key is not above the hit's depth: Z_s <= t (d.G).
Both are asserted here for every pixel of every frame of pscan_cases.FRAMES
against the oracle's primary hits, together with what they rest on: every
recorded hit lies within the reach R' of its sphere's centre (the frames' hits,
and a float32 sweep of grazing rays in the manner of tests/test_prune_bound.py),
and cameras the derivation does not cover classify as a bypass."""
import ctypes as C

import numpy as np
import pytest

import pscan_cases as cases

F = np.float32


def records(mirt, cam, W, H, geo):
    n = len(geo)
    z = np.zeros(n, np.float32)
    rect = np.zeros((n, 4), np.int32)
    reach = np.zeros(n, np.float64)
    rc = mirt.load().mirt_pscan_records(C.byref(cam), W, H, mirt.abi.ptr(geo), n, mirt.abi.ptr(z), mirt.abi.ptr(rect),
                                        mirt.abi.ptr(reach))
    assert rc == 0, rc
    return z, rect, reach


def forward(mirt, cam, W, H):
    g = np.zeros(3, np.float32)
    rho = C.c_double(0.0)
    rc = mirt.load().mirt_pscan_camera(C.byref(cam), W, H, mirt.abi.ptr(g), C.byref(rho))
    assert rc == 0, rc
    return g, rho.value


@pytest.mark.parametrize("name,W,H,n", cases.FRAMES, ids=[f"{c[0]}_{c[1]}x{c[2]}_{c[3]}" for c in cases.FRAMES])
def test_every_primary_hit_lies_in_its_record(mirt, name, W, H, n):
    cam = cases.camera(name, n)
    geo = cases.geo(n)
    z, rect, reach = records(mirt, cam, W, H, geo)
    g, rho = forward(mirt, cam, W, H)
    rays, hits = cases.primary_hits(name, W, H, n)
    s = hits["sphere"]
    hit = s >= 0
    ys, xs = np.nonzero(hit)
    print(f"{name} {W}x{H}/{n}: {hit.sum()} hit pixels, rho {rho:.3g}, "
          f"{(rect[:, 0] <= rect[:, 1]).sum()} records with a rectangle")
    if name not in ("looking_away",):
        assert hit.sum() > 0
    sh = s[hit]
    r = rect[sh]
    # 1. the tile lies in the rectangle
    inside = (xs // 8 >= r[:, 0]) & (xs // 8 <= r[:, 1]) & (ys // 8 >= r[:, 2]) & (ys // 8 <= r[:, 3])
    assert inside.all(), (name, int((~inside).sum()))
    # 2. the key is not above the hit's depth (the float values, exactly, in double)
    d = rays["direction"][hit].astype(np.float64)
    depth = hits["t"][hit].astype(np.float64) * (d @ g.astype(np.float64))
    assert (z[sh].astype(np.float64) <= depth).all(), (name, float((z[sh] - depth).max()))
    # what both rest on: the hit point within R' of the centre
    p = rays["origin"][hit].astype(np.float64) + hits["t"][hit].astype(np.float64)[:, None] * d
    dist = np.linalg.norm(p - geo[sh, :3].astype(np.float64), axis=1)
    assert (dist <= reach[sh]).all()
    if name == "far":
        tiles = {(x // 8, y // 8) for x, y in zip(xs, ys)}
        assert len(tiles) <= 2, tiles
    if name == "looking_away":
        assert (rect[:, 0] > rect[:, 1]).all()       # every leaf is behind the camera: no rectangle at all
    if name == "inside_sphere":
        assert (rect[0] == (0, (W + 7) // 8 - 1, 0, (H + 7) // 8 - 1)).all() and z[0] <= 0
    if name == "straddle":
        assert rect[0, 0] <= rect[0, 1] and z[0] < 0   # cut by the camera plane: kept, key behind the camera


def test_rectangles_are_tight_enough_to_be_worth_having(mirt):
    """The default 160 x 90 frame of 2,000 spheres: a record's rectangle is a
    few tiles, not the frame (a trivially true superset would pass the test above)."""
    cam = cases.camera("default")
    z, rect, _ = records(mirt, cam, 160, 90, cases.geo(2000))
    keep = rect[:, 0] <= rect[:, 1]
    area = ((rect[:, 1] - rect[:, 0] + 1) * (rect[:, 3] - rect[:, 2] + 1))[keep]
    print("records", keep.sum(), "mean tiles per record", area.mean(), "max", area.max(), "of", 20 * 12)
    # (some spheres lie outside the view: no rectangle)
    assert 1900 <= keep.sum() <= 2000 and area.mean() < 6 and area.max() <= 16


@pytest.mark.parametrize("name", cases.BAD_CAMERAS)
def test_cameras_outside_the_derivation_are_a_bypass(mirt, name):
    cam, want = cases.bad_camera(name)
    rc = mirt.load().mirt_pscan_camera(C.byref(cam), 160, 90, None, None)
    assert mirt.abi.PSCAN_CAM[rc] == want, (name, rc)
    z = np.zeros(1, np.float32)
    rect = np.zeros((1, 4), np.int32)
    geo = np.array([[0, 0, 0, 1]], np.float32)
    assert mirt.load().mirt_pscan_records(C.byref(cam), 160, 90, mirt.abi.ptr(geo), 1, mirt.abi.ptr(z),
                                          mirt.abi.ptr(rect), None) == rc


def test_invalid_arguments(mirt):
    cam = mirt.abi.default_camera()
    L = mirt.load()
    assert L.mirt_pscan_camera(None, 160, 90, None, None) < 0
    assert L.mirt_pscan_camera(C.byref(cam), 0, 90, None, None) < 0
    assert L.mirt_pscan_records(C.byref(cam), 160, 90, None, 1, None, None, None) < 0


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def test_recorded_hits_of_grazing_rays_lie_within_reach(mirt):
    """hit.c:19-39 in float32 (hit.c:28 in double) on rays aimed at the rim of
    their sphere, normalised as camera rays are: the hit point's distance from
    the centre against R' = pscan_reach, for camera positions in and around a
    scene of the oracle's size. The worst ratio is printed."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for radii in (lambda n: rng.uniform(0.5, 5.0, n), lambda n: 10 ** rng.uniform(-2, 2, n)):
        for _ in range(4):
            n = 200_000
            o = rng.uniform(-60, 60, 3).astype(F)
            c = rng.uniform(-60, 60, (n, 3)).astype(F)
            r = radii(n).astype(F)
            u = rng.normal(size=(n, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            d = c.astype(np.float64) + u * (rng.uniform(0.98, 1.02, n) * r)[:, None] - o
            d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
            oc = o[None, :] - c
            a = _dot(d, d)
            b = F(2) * _dot(oc, d)
            cc = _dot(oc, oc) - r * r
            disc = b * b - (F(4) * a) * cc
            ok = disc > 0
            with np.errstate(invalid="ignore"):
                t = (((-b).astype(np.float64) - np.sqrt(disc.astype(np.float64))) / (F(2) * a).astype(np.float64)).astype(F)
            ok &= t > F(1e-6)
            p = o.astype(np.float64) + t.astype(np.float64)[:, None] * d.astype(np.float64)
            dist = np.linalg.norm(p - c.astype(np.float64), axis=1)[ok]
            cam = mirt.abi.default_camera()
            cam.position.x, cam.position.y, cam.position.z = (float(v) for v in o)
            geo = np.ascontiguousarray(np.concatenate([c, r[:, None]], axis=1)[ok], np.float32)
            _, _, reach = records(mirt, cam, 160, 90, geo)
            assert ok.sum() > 1000
            # the excess over the radius, as a fraction of what R' allows over it
            ratio = (dist - geo[:, 3]) / (reach - geo[:, 3])
            worst = max(worst, float(ratio.max()))
            assert (dist <= reach).all()
    print("worst (|p - c| - r) / (R' - r):", worst)
    assert worst < 0.5

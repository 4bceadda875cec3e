"""The ray sets of tests/ray_frame_cases.py cover the ground the ray frames'
GPU tests rely on; from the oracle alone (no GPU)."""
import numpy as np

import ray_frame_cases as rc


def test_every_set_has_hits_and_misses():
    n = rc.W * rc.H
    for name in rc.SETS:
        for use_bvh in (True, False):
            hit = rc.hit_records(name, use_bvh)["sphere"] >= 0
            print(name, "bvh" if use_bvh else "brute", int(hit.sum()), "hits of", n)
            assert hit.sum() >= 0.05 * n and (~hit).sum() >= 0.05 * n, name
    for j in range(1, 4):   # the re-sampled lens slabs
        hit = rc.planes(rc.lens(j))["sphere"] >= 0
        assert hit.sum() >= 0.05 * n and (~hit).sum() >= 0.05 * n, j
        assert rc.lens(j).tobytes() != rc.lens(0).tobytes()


def test_zero_component_rays():
    ortho = rc.rays("ortho")["direction"]
    assert (ortho == np.array([0.0, 0.0, -1.0], np.float32)).all()
    zero = (rc.rays("pinhole")["direction"] == 0.0).any(axis=-1)
    assert 0 < zero.sum() < zero.size
    # some of them hit, so a walk that dropped them would show
    assert (rc.hit_records("ortho")["sphere"] >= 0).any()
    assert (rc.hit_records("pinhole")["sphere"][zero] >= 0).any()


def test_ortho_grid_leaves_the_scene():
    spheres, _, _ = rc.cases.scene(rc.N)
    reach = (np.abs(spheres["center"]) + spheres["radius"][:, None]).max(axis=0)
    o = rc.rays("ortho")["origin"]
    assert np.abs(o[..., 0]).max() > reach[0] and np.abs(o[..., 1]).max() > reach[1]


def test_far_origins_lie_beyond_four_times_the_origin_bound():
    bound = rc.o_bound()
    assert bound > 0
    far = np.abs(rc.rays("far")["origin"]).max(axis=-1)
    assert (far > 4 * bound).all(), (float(far.min()), bound)
    for name in ("pinhole", "lens", "surface"):   # ... and the near sets within it
        assert (np.abs(rc.rays(name)["origin"]).max(axis=-1) <= 4 * bound).all(), name


def test_lens_rays_are_not_normalised_and_leave_a_disc():
    r = rc.rays("lens")
    length = np.linalg.norm(r["direction"].astype(np.float64), axis=-1)
    assert length.min() >= rc.LEN_LO * (1 - 1e-5) and length.max() <= rc.LEN_HI * (1 + 1e-5)
    assert length.min() < 0.3 and length.max() > 3.5            # spans the range
    assert ((length < 0.9) | (length > 1.1)).mean() > 0.9
    cam = rc.cases.camera("A")
    off = r["origin"] - np.array([cam.position.x, cam.position.y, cam.position.z], np.float32)
    dist = np.linalg.norm(off, axis=-1)
    assert dist.max() <= rc.LENS_RADIUS * (1 + 1e-5) and dist.max() > 0.4 and (dist > 0).all()


def test_surface_rays_start_on_spheres():
    spheres, _, _ = rc.cases.scene(rc.N)
    pin = rc.hit_records("pinhole")
    hit = pin["sphere"] >= 0
    r = rc.rays("surface")
    s = spheres[pin["sphere"][hit]]
    dist = np.linalg.norm(r["origin"][hit].astype(np.float64) - s["center"], axis=-1)
    # on the sphere as far as binary32 places a hit point: hit.c's discriminant b^2 - 4ac has terms near
    # 1e4 from a camera 50 away (ulp 1e-3), and an error e in it moves the point e / (4 r) along the radius
    print("largest distance from the surface", float(np.abs(dist - s["radius"]).max()), "least radius",
          float(s["radius"].min()))
    assert np.abs(dist - s["radius"]).max() <= 4 * 2.0 ** -10 / (4 * s["radius"].min()) + 1e-4
    assert r["origin"][hit].tobytes() == pin["point"][hit].tobytes()
    assert r["direction"][hit].tobytes() == pin["normal"][hit].tobytes()
    assert r[~hit].tobytes() == rc.rays("pinhole")[~hit].tobytes()


def test_the_sets_differ_in_what_they_show():
    shown = {name: rc.colours(name).tobytes() for name in rc.SETS}
    assert len(set(shown.values())) == len(rc.SETS)
    # a ray frame's RNG stream is its pixel's and its sample's
    assert rc.colours("lens", sample=1).tobytes() != rc.colours("lens", sample=0).tobytes()

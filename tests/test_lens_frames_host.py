"""The lens frames' cases cover their ground (tests/lens_frame_cases.py, no GPU),
checked on the numpy restatement alone: the rejection loop runs more than once
but never to its fallback, the origins stay on the lens, and no lens ray has a
zero direction component (the route ray frames already test)."""
import numpy as np
import pytest

import lens_frame_cases as lc
import test_planes_cases as cases


def test_the_restated_pinhole_is_the_oracles():
    """The camera ray restated for jittered frames, without jitter, bit for bit."""
    for case in ("A", "B"):
        p, d = lc.pinhole(cases.camera(case))
        want = cases.rays(case)
        assert p.astype(np.float32).tobytes() == np.ascontiguousarray(want["origin"]).tobytes(), case
        assert np.ascontiguousarray(d).tobytes() == np.ascontiguousarray(want["direction"]).tobytes(), case


@pytest.mark.parametrize("seed", [1, 3])
def test_the_rejection_loop_runs_but_never_falls_back(seed):
    for sample in range(4):
        a, b, tries = lc.lens_points(lc.keys(seed, sample))
        late = int((tries >= 3).sum())
        print(f"seed {seed} sample {sample}: {late} pixels at the third try or later, longest {int(tries.max())}")
        assert (tries <= lc.TRIES).all(), "a pixel took the 16-rejection fallback"
        assert late >= 1
        q = a * a
        q = q + b * b
        assert (q < 1).all()


def test_the_sample_wraps_in_uint32():
    assert (lc.keys(3, 0x100000001) == lc.keys(3, 1)).all()
    s = lc.slabs("lens", seed=3, sample=0xFFFFFFFE, samples=4)
    assert s.shape == (4, lc.H, lc.W)
    assert s[2].tobytes() == lc.lens_rays("lens", 3, 0).tobytes() and s[3].tobytes() == lc.lens_rays("lens", 3, 1).tobytes()
    assert s[0].tobytes() != s[2].tobytes()


@pytest.mark.parametrize("lens", sorted(lc.LENSES))
@pytest.mark.parametrize("jitter", [False, True])
def test_origins_on_the_lens_and_no_zero_component(lens, jitter):
    aperture, _ = lc.LENSES[lens]
    cam = cases.camera("A")
    pos = np.array([cam.position.x, cam.position.y, cam.position.z], np.float64)
    for seed in (1, 3):
        for sample in range(4):
            r = lc.lens_rays(lens, seed, sample, jitter)
            dist = np.linalg.norm(r["origin"].astype(np.float64) - pos, axis=-1)
            assert (dist <= aperture * (1 + 1e-6)).all() and dist.max() > 0.9 * aperture
            assert (r["direction"] != 0).all()
            assert np.allclose(np.linalg.norm(r["direction"].astype(np.float64), axis=-1), 1.0, atol=1e-6)


def test_jitter_moves_the_rays_and_the_wide_lens_is_wider():
    assert lc.lens_rays("lens", 1, 0, True).tobytes() != lc.lens_rays("lens", 1, 0, False).tobytes()
    # one key, one lens point: the two lenses' origins differ by the apertures' ratio
    a = lc.lens_rays("lens", 1, 0)["origin"] - lc.lens_rays("lens", 1, 0)["origin"].mean(axis=(0, 1))
    b = lc.lens_rays("wide", 1, 0)["origin"] - lc.lens_rays("wide", 1, 0)["origin"].mean(axis=(0, 1))
    assert np.abs(b).max() > 7 * np.abs(a).max()

"""The walks' sphere test with t from float pairs (csrc/exact_t.h), on the GPU
through mirt_sphere_form_pairs: the filtered form as the kernels run it
(fast = 1, v_sqrt_f32 / v_rcp_f32 seeds) and with certification off (fast = 2:
every surviving pair takes the binary64 branch, which fast = 1 reaches about
once in ten thousand hits) both return the bits of the exact form (fast = 0), and
fast = 1 sends at most 1 % of the scene-like hits to the binary64 branch
(fast = 3 reports the branch per pair)."""
import numpy as np
import pytest

import exact_t_cases as X

F32 = X.F32
pytestmark = pytest.mark.gpu


def _agree(gpu, name, rays, sph, best):
    exact = gpu.sphere_form_pairs(rays, sph, best, fast=0)
    for fast in (1, 2):
        got = gpu.sphere_form_pairs(rays, sph, best, fast=fast)
        bad = np.flatnonzero(got.view(np.uint32) != exact.view(np.uint32))
        assert len(bad) == 0, (f"{name}: fast = {fast}: {len(bad)} of {len(rays)} differ from the exact form, first "
                               f"{rays[bad[0]]} {sph[bad[0]]} best {best[bad[0]]!r}: {got[bad[0]]!r} != "
                               f"{exact[bad[0]]!r}")
    return exact


def _bests(t):
    """+inf, the recorded t itself (a tie is a hit), and one float below it."""
    inf = np.full(len(t), np.inf, F32)
    with np.errstate(invalid="ignore"):
        tie = np.where(t > 0, t, inf).astype(F32)
        below = np.where(t > 0, np.nextafter(tie, F32(0)), inf).astype(F32)
    return inf, tie, below


def test_scene_like_pairs(gpu, mirt):
    """Set (a): bits, and the share sent to the binary64 branch."""
    o, d, c, r = X.scene_like(np.random.default_rng(901), 4_000_000)
    rays, sph = X.as_abi(mirt, o, d, c, r)
    inf = np.full(len(rays), np.inf, F32)
    t = _agree(gpu, "scene-like", rays, sph, inf)
    hits = t > 0
    b, disc, d2a = X.quadratic(o, d, c, r)
    want = np.where((disc > 0) & (X.reference_t(b, disc, d2a) > X.KEPS), X.reference_t(b, disc, d2a), F32(-1))
    assert (t.view(np.uint32) == want.astype(F32).view(np.uint32)).all()
    f64 = gpu.sphere_form_pairs(rays, sph, inf, fast=3).view(np.uint32)
    assert set(np.unique(f64)) <= {0, 1}
    share = float(f64.sum()) / float(hits.sum())
    print(f"  scene-like: {len(rays)} pairs, {int(hits.sum())} hits with t > kEps; the binary64 branch ran for "
          f"{int(f64.sum())} pairs ({100 * share:.4f}% of the hits)")
    assert hits.sum() > len(rays) // 4
    assert share <= 0.01


@pytest.mark.parametrize("which", ["near-midpoint", "edge"])
def test_hard_pairs(gpu, mirt, which):
    """Sets (b) and (c), with best at +inf, equal to t and one float below."""
    o, d, c, r = X.midpoint_cases() if which == "near-midpoint" else X.edge_cases(np.random.default_rng(902))
    rays, sph = X.as_abi(mirt, o, d, c, r)
    t = _agree(gpu, which, rays, sph, np.full(len(rays), np.inf, F32))
    assert (t > 0).sum() > len(rays) // 8
    if which == "near-midpoint":
        b, disc, d2a = X.quadratic(o, d, c, r)
        assert (t.view(np.uint32) == X.reference_t(b, disc, d2a).view(np.uint32)).all()
        f64 = gpu.sphere_form_pairs(rays, sph, np.full(len(rays), np.inf, F32), fast=3).view(np.uint32)
        print(f"  near-midpoint: the binary64 branch ran for {int(f64.sum())} of {len(rays)}")
        assert 0 < f64.sum() < len(rays)    # both branches decide pairs of this set
    for best in _bests(t)[1:]:
        got = _agree(gpu, which, rays, sph, best)
        with np.errstate(invalid="ignore"):
            want = np.where((t > 0) & (t <= best), t, F32(-1)).astype(F32)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_rejects_unknown_mode(gpu, mirt):
    rays, sph = X.as_abi(mirt, *X.scene_like(np.random.default_rng(1), 4))
    out = np.zeros(4, np.uint32)
    p = mirt.abi.ptr
    best = np.full(4, np.inf, F32)
    assert gpu.L.mirt_sphere_form_pairs(gpu.h, p(rays), p(sph), p(best), 4, 4, p(out)) == -1

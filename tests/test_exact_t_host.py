"""csrc/exact_t.h on the CPU, through mirt_exact_t_pairs: hit.c:28's t from
float pairs. The whole correctness condition: a CERTIFIED result equals the
binary64 expression rounded to float32 (numpy) bit for bit -- for square-root
and reciprocal seeds anywhere within -2 .. +2 ulp of the correctly rounded
ones, which covers v_sqrt_f32 / v_rcp_f32 (1 ulp) with room. Uncertified pairs
cost time, not correctness: on scene-like pairs they are capped at 1 % of the
hits with t > kEps (the header's bound E = 2^-39 (|b| + s) / 2a leaves far
fewer)."""
import itertools

import numpy as np
import pytest

import exact_t_cases as X

F32 = X.F32
OFFSETS = (-2, -1, 0, 1, 2)


def _pairs(mirt, L, b, disc, d2a, ks, kr):
    """(th, certified) with the root seed moved by ks ulps and both
    reciprocal seeds by kr ulps."""
    with np.errstate(all="ignore"):
        s = X.move_ulps(np.sqrt(disc), ks)
        rs = X.move_ulps(F32(1) / s, kr)
        rd = X.move_ulps(F32(1) / d2a, kr)
    th = np.zeros(len(b), F32)
    cert = np.zeros(len(b), np.uint8)
    p = mirt.abi.ptr
    rc = L.mirt_exact_t_pairs(len(b), p(b), p(disc), p(d2a), p(np.ascontiguousarray(s)), p(np.ascontiguousarray(rs)),
                              p(np.ascontiguousarray(rd)), p(th), p(cert))
    assert rc == 0, L.mirt_last_error()
    return th, cert != 0


def _check(mirt, name, o, d, c, r, cap=None):
    L = mirt.load()
    b, disc, d2a = X.quadratic(o, d, c, r)
    # the seeds are moved as bit patterns: positive normal roots and reciprocals only (anything else is never
    # certified, which the unmoved seeds of set (c) check below)
    with np.errstate(all="ignore"):
        movable = (disc >= F32(2.0 ** -100)) & (disc <= F32(2.0 ** 100)) & (d2a >= F32(2.0 ** -100)) & \
                  (d2a <= F32(2.0 ** 100))
    b, disc, d2a = (np.ascontiguousarray(v[movable]) for v in (b, disc, d2a))
    want = X.reference_t(b, disc, d2a)
    above = want > X.KEPS
    worst = 0.0
    for ks, kr in itertools.product(OFFSETS, OFFSETS):
        th, cert = _pairs(mirt, L, b, disc, d2a, ks, kr)
        bad = np.flatnonzero(cert & (th.view(np.uint32) != want.view(np.uint32)))
        assert len(bad) == 0, (f"{name}: seeds {ks:+d}/{kr:+d} ulp: {len(bad)} certified results differ from the "
                               f"binary64 t, first b={b[bad[0]]!r} disc={disc[bad[0]]!r} 2a={d2a[bad[0]]!r}: "
                               f"{th[bad[0]]!r} != {want[bad[0]]!r}")
        worst = max(worst, float((~cert & above).sum()) / max(int(above.sum()), 1))
    print(f"  {name}: {len(b)} pairs with disc > 0, {int(above.sum())} with t > kEps; uncertified among those, "
          f"worst seed offsets: {100 * worst:.3f}%")
    if cap is not None:
        assert above.sum() > len(o) // 4
        assert worst <= cap, f"{name}: {100 * worst:.3f}% of the hits with t > kEps are uncertified (cap 1%)"
    return worst


@pytest.fixture(scope="module")
def scene_pairs():
    return X.scene_like(np.random.default_rng(901), 4_000_000)


def test_scene_like_pairs_certified_results_are_exact_and_common(mirt, scene_pairs):
    """Set (a): about 4 M scene-like pairs under all 25 seed offsets; at most
    1 % of the hits with t > kEps uncertified."""
    with np.errstate(all="ignore"):
        keep = X.quadratic(*scene_pairs)[1] > 0
    _check(mirt, "scene-like", *(v[keep] for v in scene_pairs), cap=0.01)


def test_near_midpoint_pairs(mirt):
    """Set (b): the 10,000 pairs of a 10^8 scan nearest a rounding midpoint."""
    o, d, c, r = X.midpoint_cases()
    assert len(o) == 10_000
    b, disc, d2a = X.quadratic(o, d, c, r)
    assert (X.midpoint_distance(b, disc, d2a) < 1e-3).all()
    _check(mirt, "near-midpoint", o, d, c, r)


def test_edge_cases(mirt):
    """Set (c): cancellation, t around kEps, binade edges, huge and tiny |d|,
    subnormal discriminants. Nothing outside the proof's range is certified,
    no power of two, no zero / subnormal / non-finite th."""
    o, d, c, r = X.edge_cases(np.random.default_rng(902))
    _check(mirt, "edge", o, d, c, r)
    L = mirt.load()
    b, disc, d2a = X.quadratic(o, d, c, r)
    with np.errstate(all="ignore"):
        hit = disc > 0
    b, disc, d2a = (np.ascontiguousarray(v[hit]) for v in (b, disc, d2a))
    th, cert = _pairs(mirt, L, b, disc, d2a, 0, 0)
    want = X.reference_t(b, disc, d2a)
    assert (th[cert].view(np.uint32) == want[cert].view(np.uint32)).all()
    lo, hi = F32(2.0 ** -30), F32(2.0 ** 30)
    with np.errstate(all="ignore"):
        in_range = (disc >= lo) & (disc <= hi) & (d2a >= lo) & (d2a <= hi) & (np.abs(b) <= hi)
    assert not cert[~in_range].any() and (~in_range).sum() > 1000
    m, e = np.frexp(th[cert])
    assert np.isfinite(th[cert]).all() and (np.abs(th[cert]) >= F32(2.0 ** -126)).all() and (np.abs(m) != 0.5).all()
    pow2 = np.abs(np.frexp(want)[0]) == 0.5
    assert pow2.sum() >= 50 and not cert[pow2].any()
    assert cert.sum() > 1000    # (the cancelling pairs, t ~ 0 against |b| + s ~ 1, cannot be certified)
    # not reached with disc <= 0 or NaN
    z = np.array([0.0, -1.0, np.nan], F32)
    one = np.ones(3, F32)
    _, cz = _pairs(mirt, L, one, z, one + one, 0, 0)
    assert not cz.any()


def test_rejects_bad_arguments(mirt):
    L = mirt.load()
    assert L.mirt_exact_t_pairs(-1, None, None, None, None, None, None, None, None) == -1
    assert L.mirt_exact_t_pairs(1, None, None, None, None, None, None, None, None) == -1
    assert L.mirt_last_error().decode() == "mirt_exact_t_pairs: invalid arguments"
    assert L.mirt_exact_t_pairs(0, None, None, None, None, None, None, None, None) == 0

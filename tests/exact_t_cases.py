"""Inputs and the numpy reference shared by tests/test_exact_t_host.py,
tests/test_exact_t_gpu.py and scripts/make_exact_t_golden.py: (ray, sphere)
pairs for the float-pair form of hit.c:28's t (csrc/exact_t.h), hit.c:22-25's
floats of a pair, and T = RN32 of the binary64 expression."""
import os

import numpy as np

F32 = np.float32
KEPS = F32(0.000001)
GOLDEN_MIDPOINTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_t_midpoints.npz")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def scene_like(rng, n):
    """Set (a): origins in the bench cloud's box (+-40, +-20, -10 .. 5), sphere
    centres 0.5 - 30 units away, radii 0.5 - 5, unit directions aimed within
    about the sphere's angular radius of its centre (half of them hit, from
    inside and outside). Returns float32 (origin, direction, centre, radius)."""
    o = rng.uniform([-40, -20, -10], [40, 20, 5], size=(n, 3))
    dist = rng.uniform(0.5, 30.0, size=(n, 1))
    c = o + dist * _unit(rng, n)
    r = rng.uniform(0.5, 5.0, size=n)
    aim = (c - o) / dist + _unit(rng, n) * (rng.uniform(0.0, 1.6, size=(n, 1)) * np.minimum(r[:, None] / dist, 1.0))
    d = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(F32)
    # unit in float32 as normalize3 leaves it: one more float32 normalisation
    d = d / np.sqrt((d * d).sum(axis=1, dtype=F32), dtype=F32)[:, None]
    return o.astype(F32), d.astype(F32), c.astype(F32), r.astype(F32)


def quadratic(o, d, c, r):
    """hit.c:22-25 in float32, operation by operation: (b, disc, 2a)."""
    with np.errstate(all="ignore"):
        oc = o - c

        def dot(p, q):
            return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
        a = dot(d, d)
        b = F32(2) * dot(oc, d)
        cc = dot(oc, oc) - r * r
        disc = b * b - (F32(4) * a) * cc
        return b.astype(F32), disc.astype(F32), (F32(2) * a).astype(F32)


def t64(b, disc, d2a):
    """hit.c:28 in binary64, before the cast to float."""
    with np.errstate(all="ignore"):
        return (-b.astype(np.float64) - np.sqrt(disc.astype(np.float64))) / d2a.astype(np.float64)


def reference_t(b, disc, d2a):
    with np.errstate(all="ignore"):
        return t64(b, disc, d2a).astype(F32)


def midpoint_distance(b, disc, d2a):
    """|T64 - the nearest float32 rounding midpoint| in ulps of T (0 .. 0.5)."""
    with np.errstate(all="ignore"):
        x = t64(b, disc, d2a)
        t = x.astype(F32)
        ulp = np.spacing(np.abs(t)).astype(np.float64)
        return 0.5 - np.abs(x - t.astype(np.float64)) / ulp


def move_ulps(x, k):
    """Positive finite float32 x moved by k ulps (its bit pattern + k)."""
    return (x.view(np.int32) + np.int32(k)).view(F32)


# tests/test_filtered_forms.py's REGRESSION_SUBNORMAL_DISC: hits whose float
# discriminant is subnormal (origin, direction, centre, radius)
SUBNORMAL_DISC = [
    ((24.533575, 30.492432, -32.63027), (-3.2698698e-18, -5.0390267e-18, 4.472186e-19),
     (12.886415, 12.516208, -31.2687), 0.23283343),
    ((-2961.7927, 8.618334, 6.5228534), (4.9334296e-20, -9.309416e-20, 2.5584113e-20),
     (-2960.5205, 7.458422, 6.6698794), 0.6743745),
    ((59024.133, 59034.62, -58985.3), (-1.0065886e-19, -1.0191529e-19, 2.1899454e-19),
     (59015.258, 59025.53, -58966.17), 0.17619625),
    ((60954.79, 32.35749, 60951.984), (-3.101837e-20, 3.5089477e-20, 9.778309e-20),
     (60954.51, 32.483982, 60952.55), 0.12646852),
]


def edge_cases(rng):
    """Set (c), float32 (origin, direction, centre, radius):
      * cancelling: origins on (and a few ulps off) a sphere's surface, so that
        -b ~ sqrt(disc) and t ~ 0, straddling kEps when moved back along the ray
        by about kEps;
      * binade edges: axis-aligned rays whose t is a power of two exactly, and
        the floats around it;
      * huge and tiny |d|: scene-like pairs with the direction scaled by
        2^-70 .. 2^50 (t, disc and 2a leave the certified range both ways);
      * the subnormal-discriminant regression pairs."""
    parts = []
    # cancelling / kEps
    n = 20000
    c = rng.uniform(-30, 30, size=(n, 3))
    r = rng.uniform(0.5, 5.0, size=n)
    nrm = _unit(rng, n)
    d = _unit(rng, n)
    d = np.where(((d * nrm).sum(axis=1) > 0)[:, None], -d, d)   # into the sphere: the near root is the origin
    back = np.concatenate([np.zeros(n // 2), rng.uniform(0.0, 3e-6, size=n - n // 2)])
    o = c + r[:, None] * nrm - back[:, None] * d
    parts.append((o, d, c, r))
    # binade edges: o = (0, 0, -(2^k + r)), d = +z, centre 0: t = 2^k; and origins a few ulps around
    ks = np.arange(-6, 8)
    r = np.array([0.5, 1.0, 2.0, 3.0])
    K, R = np.meshgrid(2.0 ** ks, r, indexing="ij")
    K, R = K.ravel(), R.ravel()
    for off in range(-3, 4):
        z = (-(K + R)).astype(F32)
        z = (z.view(np.int32) + np.int32(off)).view(F32)
        o = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
        d = np.tile(np.array([[0.0, 0.0, 1.0]]), (len(z), 1))
        parts.append((o, d, np.zeros((len(z), 3)), R))
    # huge and tiny |d|
    o, d, c, r = scene_like(rng, 40000)
    scale = (2.0 ** rng.integers(-70, 51, size=len(o))).astype(F32)
    with np.errstate(all="ignore"):
        parts.append((o, d * scale[:, None], c, r))
    # subnormal discriminants
    parts.append(tuple(np.array([p[k] for p in SUBNORMAL_DISC]) for k in range(4)))
    return tuple(np.concatenate([np.asarray(p[k], np.float64) for p in parts]).astype(F32) for k in range(4))


def midpoint_cases():
    """Set (b): the committed near-midpoint pairs (scripts/make_exact_t_golden.py)."""
    with np.load(GOLDEN_MIDPOINTS, allow_pickle=False) as z:
        return z["origin"], z["direction"], z["center"], z["radius"]


def as_abi(mirt, o, d, c, r):
    """(rays, spheres) records for Renderer.sphere_form_pairs."""
    rays = np.zeros(len(o), mirt.abi.RAY)
    rays["origin"], rays["direction"] = o, d
    sph = np.zeros(len(o), mirt.abi.SPHERE)
    sph["center"], sph["radius"] = c, r
    return rays, sph

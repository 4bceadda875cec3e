"""Hostile rays: the inputs of tests/test_hostile_rays_host.py (the oracle alone,
no GPU) and tests/test_hostile_rays_gpu.py. "Rays are used as given": every
family below is something mirt.h admits -- non-finite components, zero
directions, |d| from 2^-95 to 2^127, origins at the float range's end -- on
ray_frame_cases' grid, so each family is both a batch for the per-ray entry
points (flat index i = y * W + x) and a ray frame of 44 x 26 over
test_planes_cases.scene(1000), derived from the pinhole rays of case A:

  nf_origin, nf_dir  +inf, -inf, NaN in one component, cycling through component
                     (i % 3) and value ((i // 3) % 3); every fourth pixel gets a
                     second, every eighth a third non-finite component (seeded)
  zero_dir           direction (+-0, +-0, +-0), the eight sign patterns by i % 8
  tiny               direction times 2^-k, k uniform in 60..95 per pixel: below
                     k = 70 ordinary, 74..81 the reference records t = +inf
                     with a NaN normal, from 82 on everything misses
  tiny_inf           k in 74..81 only
  huge               direction times 2^k, k in 55..127
  far_origin         by i % 3: one origin component (cycling) at +-3.0e38, the
                     origin times 1e30, the origin times 2^40
  mixed_<mask>_<src> the base rays with hostile ones substituted where the mask
                     holds; src `tiny` takes tiny_inf's ray of the same pixel,
                     src `nf` nf_origin's or nf_dir's by (i // 4) % 2

The masks, and where each puts a hostile ray. A per-ray kernel (intersect_kernel,
bvh_any_kernel, trace_rays_kernel, the brute-force kernels) gives ray i to lane
i % 64 of wave i // 64, one ray per lane; the quad batch (intersect_quad_kernel)
gives ray i to the four lanes 4 (i % 16) .. + 3 of the 16-ray wave i // 16; a ray
frame's kernels (ray_primary_kernel, ray_path_kernel) give the 8 x 8 tile
(y // 8, x // 8) to one wave, pixel (y, x) to lane 8 (y % 8) + x % 8, and W = 44
is a multiple of four, so x % 4 == i % 4.

  quad   i % 4 == 0        one lane of every quad of a per-ray wave and of a
                           frame's wave (DPP neighbours, the quad-wide ballots of
                           wide_lane_step's gate loop); in the quad batch one ray
                           in four, so four hostile quads per 16-ray wave
  wave   i % 64 != 63      all but one lane of a per-ray wave: the ordinary ray
                           sits alone in the wave's ballots, the chunked walk's
                           queue (closest_hit's gm loop) and the LDS stack columns
  waves  (i // 64) % 2     whole per-ray waves hostile, their neighbours in the
                           workgroup (256 threads = four waves, one LDS stack
                           array) ordinary; in the quad batch four 16-ray waves
  tiles  checkerboard      whole 8 x 8 tiles: whole waves of a ray frame hostile,
                           and the bounce kernel's queue fed by the ordinary
                           tiles only

A second scene, test_filtered_forms.lattice_scene(far=True): fp16-exact boxes,
touching spheres, eight exact duplicates (which the reference's build keeps in
one leaf each, where its walk tests only the first: they never tie there)
and no origin bound (o_bound == 0), with its own tiny_inf and nf_origin sets
from lattice_rays, and a mixed set (every fourth ray tiny_inf's, the others
ordinary).

A third scene, `twins`: exact duplicates in leaves of their own (a hand-made
flat tree), where every hit is an exact tie that hit.c gives to the later leaf:
at finite t for ordinary rays, which reach the walks that merge candidates
across a quad (cand_better), and at t = +inf for every fourth ray. (No ray
with all direction components of 2^-40 or more can record t = +inf: that needs
|o - c| / |d| above 3.4e38 while |o - c|^2 stays below it. So infinite ties
occur only in the chunked walk.)

Cameras: case A's with a NaN position component (x, y, z separately), +inf in z,
1e30 in x, 3.0e38 in y, fov 0, 180 and NaN, and two yaw / pitch pairs through
mirt_camera_update that give `forward` an exact zero component.

Everything is seeded, computed once and read-only. The oracle's results per
family (hit records of the tree walk and of brute force, colours at depths 1, 5
and 8) are cached like ray_frame_cases._colours.
"""
import functools
import importlib

import numpy as np

import ray_frame_cases as rc
import test_planes_cases as cases

abi = cases.abi
W, H, N = rc.W, rc.H, rc.N
F32 = np.float32
DEPTHS = (1, 5, 8)
NF_VALUES = np.array([np.inf, -np.inf, np.nan], F32)

PLAIN = ("nf_origin", "nf_dir", "zero_dir", "tiny", "tiny_inf", "huge", "far_origin")
MASKS = ("quad", "wave", "waves", "tiles")
MIXED = tuple(f"mixed_{m}_{s}" for m in MASKS for s in ("tiny", "nf"))
FAMILIES = PLAIN + MIXED
MAY_HOLD_NAN = ("tiny", "tiny_inf") + MIXED   # the oracle's records hold no NaN outside these
ALL_MISS = ("nf_origin", "nf_dir", "zero_dir", "far_origin")   # and `huge` from k = 64 on


def _frozen(a):
    a.setflags(write=False)
    return a


def _flat():
    return np.arange(W * H).reshape(H, W)


def base():
    return cases.rays("A")


def _scaled(k):
    """The base rays with the direction times 2^k (exact: a power of two, no result below the subnormal range)."""
    out = base().copy()
    out["direction"] = (base()["direction"].astype(np.float64) * (2.0 ** k)[..., None]).astype(F32)
    return out


@functools.lru_cache(maxsize=None)
def exponents(name):
    """The per-pixel k of `tiny`, `tiny_inf` (direction times 2^-k) and `huge` (times 2^k)."""
    lo, hi, seed = {"tiny": (60, 95, 11), "tiny_inf": (74, 81, 12), "huge": (55, 127, 13)}[name]
    return _frozen(np.random.default_rng(seed).integers(lo, hi + 1, (H, W)))


def _non_finite(field, seed):
    rng = np.random.default_rng(seed)
    out = base().copy()
    i = _flat()
    v = out[field]
    comp = i % 3
    yy, xx = np.indices((H, W))
    v[yy, xx, comp] = NF_VALUES[(i // 3) % 3]
    for every, step in ((4, 1), (8, 2)):
        m = i % every == every - 1
        v[yy[m], xx[m], (comp[m] + step) % 3] = NF_VALUES[rng.integers(0, 3, int(m.sum()))]
    return out


def mask(name):
    """(H, W) bool: where a mixed set holds a hostile ray."""
    i = _flat()
    yy, xx = np.indices((H, W))
    return {"quad": i % 4 == 0, "wave": i % 64 != 63, "waves": (i // 64) % 2 == 1,
            "tiles": (yy // 8 + xx // 8) % 2 == 1}[name]


@functools.lru_cache(maxsize=None)
def rays(name):
    if name == "base":
        return base()
    if name == "nf_origin":
        return _frozen(_non_finite("origin", 21))
    if name == "nf_dir":
        return _frozen(_non_finite("direction", 22))
    if name == "zero_dir":
        out = base().copy()
        signs = np.array([[(-0.0 if (p >> c) & 1 else 0.0) for c in range(3)] for p in range(8)], F32)
        out["direction"] = signs[_flat() % 8]
        return _frozen(out)
    if name in ("tiny", "tiny_inf"):
        return _frozen(_scaled(-exponents(name)))
    if name == "huge":
        return _frozen(_scaled(exponents(name)))
    if name == "far_origin":
        out = base().copy()
        i = _flat()
        o = out["origin"]
        yy, xx = np.indices((H, W))
        m = i % 3 == 0
        o[yy[m], xx[m], (i[m] // 3) % 3] = np.where((i[m] // 9) % 2 == 0, F32(3.0e38), F32(-3.0e38))
        with np.errstate(over="ignore"):
            o[i % 3 == 1] = (o[i % 3 == 1].astype(np.float64) * 1e30).astype(F32)
        o[i % 3 == 2] = o[i % 3 == 2] * F32(2.0 ** 40)
        return _frozen(out)
    if name.startswith("mixed_"):
        _, m, src = name.split("_")
        hostile = mask(m)
        out = base().copy()
        if src == "tiny":
            out[hostile] = rays("tiny_inf")[hostile]
        else:
            first = hostile & ((_flat() // 4) % 2 == 0)
            out[first] = rays("nf_origin")[first]
            out[hostile & ~first] = rays("nf_dir")[hostile & ~first]
        return _frozen(out)
    raise KeyError(name)


def substituted(name):
    """The mask of a mixed set (H, W)."""
    return mask(name.split("_")[1])


@functools.lru_cache(maxsize=None)
def hits(name, use_bvh=True):
    """The oracle's abi.HIT records of a family, (H, W)."""
    return _frozen(cases.intersect(N, rays(name), use_bvh).reshape(H, W))


@functools.lru_cache(maxsize=None)
def colours(name, depth=5, use_bvh=True, seed=1, sample=0):
    """Oracle.trace_rays of the full-frame array (pixel index y * W + x), (H, W, 4)."""
    spheres, tree, _ = cases.scene(N)
    out = cases._oracle().trace_rays(np.ascontiguousarray(rays(name)).reshape(-1), spheres, tree, depth=depth,
                                     use_bvh=bool(use_bvh), seed=seed, sample=sample).reshape(H, W, 4)
    return _frozen(out)


def nan_elements(records):
    """How many float elements of abi.HIT records (t, point, normal) are NaN."""
    return int(np.isnan(records["t"]).sum() + np.isnan(records["point"]).sum() + np.isnan(records["normal"]).sum())


def counts(name):
    """The figures MEASUREMENTS.md records per family, from the oracle alone."""
    h, b = hits(name), hits(name, False)
    inf_t = (h["hit"] != 0) & np.isposinf(h["t"])
    return dict(hits=int((h["hit"] != 0).sum()), inf_t=int(inf_t.sum()),
                finite_t=int(((h["hit"] != 0) & np.isfinite(h["t"])).sum()),
                nan_normals=int(np.isnan(h["normal"]).any(-1).sum()), nan_elements=nan_elements(h),
                brute_hits=int((b["hit"] != 0).sum()), brute_nan_elements=nan_elements(b),
                tree_vs_brute_records=int((h["sphere"] != b["sphere"]).sum()),
                tree_vs_brute_colours=int((colours(name) != colours(name, use_bvh=False)).any(-1).sum()),
                colours=len(np.unique(colours(name).reshape(-1, 4), axis=0)))


# ---------------------------------------------------------------- the lattice

LATTICE_SETS = ("lattice_tiny_inf", "lattice_nf_origin", "lattice_mixed_quad_tiny")


@functools.lru_cache(maxsize=None)
def lattice():
    """(spheres as the oracle's build reordered them, its tree handle, the flat tree) of
    test_filtered_forms.lattice_scene(far=True)."""
    import test_filtered_forms as ff
    mirt = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")
    o = cases._oracle()
    s = ff.lattice_scene(mirt, far=True)
    tree = o.build(s)
    nodes = o.flatten(tree)
    return _frozen(s), tree, _frozen(nodes)


@functools.lru_cache(maxsize=None)
def lattice_rays(name):
    import test_filtered_forms as ff
    s, _, _ = lattice()
    like = ff.lattice_rays(np.random.default_rng(41), s, n_each=200)
    assert len(like) <= 2000
    out = like.copy()
    if name == "lattice_tiny_inf":
        k = np.random.default_rng(42).integers(74, 82, len(like))
        d = like["direction"].astype(np.float64)
        norm = np.linalg.norm(d, axis=1)
        d /= np.where(norm > 0, norm, 1.0)[:, None]   # (a direction that underflowed to zero stays zero)
        out["direction"] = (d * (2.0 ** -k)[:, None]).astype(F32)
    elif name == "lattice_nf_origin":
        i = np.arange(len(like))
        out["origin"][i, i % 3] = NF_VALUES[(i // 3) % 3]
        m = i % 4 == 3
        out["origin"][i[m], (i[m] + 1) % 3] = NF_VALUES[np.random.default_rng(43).integers(0, 3, int(m.sum()))]
    elif name == "lattice_mixed_quad_tiny":   # ordinary rays beside hostile ones, without an origin bound
        hostile = np.arange(len(like)) % 4 == 0
        out[hostile] = lattice_rays("lattice_tiny_inf")[hostile]
    elif name != "lattice_base":
        raise KeyError(name)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def lattice_hits(name, use_bvh=True):
    s, tree, _ = lattice()
    return _frozen(cases._oracle().intersect(tree, s, lattice_rays(name), use_bvh))


@functools.lru_cache(maxsize=None)
def lattice_colours(name, depth=5, use_bvh=True, seed=1):
    s, tree, _ = lattice()
    return _frozen(cases._oracle().trace_rays(lattice_rays(name), s, tree, depth=depth, use_bvh=bool(use_bvh), seed=seed))


def lattice_duplicates():
    """Indices (into the reordered spheres) of the spheres that have an exact duplicate."""
    s, _, _ = lattice()
    _, inv, cnt = np.unique(np.column_stack([s["center"], s["radius"]]), axis=0, return_inverse=True,
                            return_counts=True)
    return np.flatnonzero(cnt[inv.ravel()] > 1)


# ---------------------------------------------------------------- twins

def flat_tree(spheres):
    """A flat pre-order tree (abi.NODE) with ONE sphere per leaf over the spheres in array order, split at the
    middle index; a leaf's box is fl(c -+ r). No builder makes it: the reference's build keeps exact duplicates
    in one leaf, and its walk tests only a leaf's first sphere, so there the twins never tie."""
    lo = spheres["center"] - spheres["radius"][:, None]
    hi = spheres["center"] + spheres["radius"][:, None]
    out = []

    def build(a, b):
        i = len(out)
        out.append(None)
        if b - a > 1:
            build(a, (a + b) // 2)
            build((a + b) // 2, b)
        out[i] = (lo[a:b].min(0), hi[a:b].max(0), a if b - a == 1 else -1, len(out))

    build(0, len(spheres))
    nodes = np.zeros(len(out), abi.NODE)
    for i, node in enumerate(out):
        nodes[i] = node
    return nodes


TWINS_N, TWINS_W, TWINS_H = 1024, 32, 32


@functools.lru_cache(maxsize=None)
def twins():
    """32 spheres of radius 1.5 on a grid, each followed by its exact duplicate, every sphere in a leaf of its
    own: every ray that hits sphere 2j hits 2j + 1 at the same t -- finite or +inf -- and hit.c records the
    later leaf, 2j + 1 (brute force, with its strict `<`, the first). (spheres, the oracle's tree, flat tree)."""
    g = np.arange(-6, 7, 4)
    c = np.repeat(np.array([(x, y, z) for z in g[:2] for y in g for x in g], np.float64), 2, axis=0)
    s = np.zeros(len(c), abi.SPHERE)
    s["center"], s["radius"] = c, 1.5
    i = np.arange(len(c))
    s["color"] = np.stack([(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 17) % 256, np.full(len(c), 255)], 1)
    nodes = flat_tree(s)
    return _frozen(s), cases._oracle().tree_from_flat(nodes), _frozen(nodes)


@functools.lru_cache(maxsize=None)
def twins_rays():
    """1024 rays (a 32 x 32 frame) aimed into the spheres from about 30 away; every fourth with its direction
    times 2^-k, k in 74..81 (t = +inf), the others unit (finite ties, directions without a tiny component:
    the walks that merge candidates with cand_better)."""
    s, _, _ = twins()
    rng = np.random.default_rng(51)
    n = TWINS_N
    k = rng.integers(0, len(s), n)
    origin = (s["center"][k] + rng.normal(size=(n, 3)) * 30).astype(F32)
    d = s["center"][k] + rng.uniform(-1, 1, (n, 3)) * 0.8 - origin
    d /= np.linalg.norm(d, axis=1)[:, None]
    out = np.zeros(n, abi.RAY)
    out["origin"], out["direction"] = origin, d
    hostile = np.arange(n) % 4 == 0
    scale = 2.0 ** -rng.integers(74, 82, n)
    out["direction"][hostile] = (d[hostile] * scale[hostile, None]).astype(F32)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def twins_hits(use_bvh=True):
    s, tree, _ = twins()
    return _frozen(cases._oracle().intersect(tree, s, twins_rays(), use_bvh))


@functools.lru_cache(maxsize=None)
def twins_colours(depth=5, use_bvh=True, seed=1):
    s, tree, _ = twins()
    return _frozen(cases._oracle().trace_rays(twins_rays(), s, tree, depth=depth, use_bvh=bool(use_bvh), seed=seed))


# ---------------------------------------------------------------- cameras

CAMERAS = ("nan_x", "nan_y", "nan_z", "inf_z", "1e30_x", "3e38_y", "fov_0", "fov_180", "fov_nan",
           "forward_y0", "forward_x0")
CAMERA_SIZES = ((44, 26), (77, 45))


def camera(name):
    cam = cases.camera("A")
    if name == "A":
        return cam
    pos = {"nan_x": ("x", np.nan), "nan_y": ("y", np.nan), "nan_z": ("z", np.nan), "inf_z": ("z", np.inf),
           "1e30_x": ("x", 1e30), "3e38_y": ("y", 3.0e38)}
    fov = {"fov_0": 0.0, "fov_180": 180.0, "fov_nan": np.nan}
    turn = {"forward_y0": (-np.pi + 0.5, 0.0), "forward_x0": (0.0, 0.3)}   # sin(0) is an exact zero
    if name in pos:
        setattr(cam.position, *pos[name])
    elif name in fov:
        cam.fov = fov[name]
    else:
        cam.yaw, cam.pitch = turn[name]
        if name == "forward_x0":   # yaw 0 looks along +z: from the far side of the scene
            cam.position.z = -50.0
        importlib.import_module("cs201_sah-bvh_ray_tracer_amd").camera_update(cam)
    return cam


@functools.lru_cache(maxsize=None)
def camera_frame(name, width, height, use_bvh=True, depth=5, seed=1):
    """Oracle.render of a camera, (height, width, 4)."""
    spheres, tree, _ = cases.scene(N)
    return _frozen(cases._oracle().render(camera(name), width, height, spheres, tree, depth=depth, use_bvh=use_bvh,
                                          mode=1, seed=seed))


@functools.lru_cache(maxsize=None)
def camera_planes(name, width, height, use_bvh=True):
    """{"t", "sphere", "normal"} of the camera's own rays, from the oracle."""
    r = cases._oracle().camera_rays(camera(name), width, height)
    return cases.planes_of(cases.intersect(N, r, use_bvh), (height, width))

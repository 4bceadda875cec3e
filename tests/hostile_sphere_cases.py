"""Hostile spheres: the inputs of tests/test_hostile_spheres_host.py (the oracle
and the host builder, no GPU) and tests/test_hostile_spheres_gpu.py. "Spheres
are used as given" (mirt.h): every scene below is the 1000 INPUT spheres of
test_planes_cases.scene(1000) (render_scene(1, 1000), before any build) with
some radii or centres replaced, then built by the oracle. hostile_ray_cases is
the dual: ordinary spheres, hostile rays.

Where a family has a sparse and a dense variant, the sparse one changes the
three spheres FIXED (the tree stays rich), the dense one every 4th or 16th
sphere (the tree degenerates or collapses to a chain).

  neg_r_sparse, neg_r_4th, neg_r_all   radii negated: inverted boxes c - r > c + r
  zero_r_4th      every fourth radius 0
  tiny_r          every second radius times 2^-k, k in 10..140 (seeded): through
                  subnormal r, and r * r == 0 from k = 75 on
  scales          every radius times 2^k, k in -16..2 (seeded)
  nan_r_*, nan_c_*  NaN radius; NaN in centre component (ordinal % 3)
  inf_r_*, inf_c_*  +-inf radius (alternating); +-inf in one centre component
  huge_r_sparse   radii 2^20, 2^64, 2^127; huge_r_4th 2^k, k in 20..127: r * r
                  overflows from 2^64 on, every box area overflows
  far_c_sparse    one centre component times 2^10, 2^50, 2^100; far_c_4th 2^k,
                  k in 10..100
  dups            s[1::2] = s[0::2]
  neg_hidden      sphere 1 = sphere 0, then sphere 0's radius -6 (larger than any other |r|):
                  the pair never splits, shares a depth-40 leaf whose first
                  sphere, the positive one, is the only one hit.c tests, and the
                  leaf's box is the positive one's: the tree still encloses, and
                  r_max / c_max must come from |r|
  giant_wall      sphere 0 replaced by one of radius 3e4 tangent behind the scene
  giant_dome_<R>  sphere 0 replaced by one of radius 5.0e4, 5.99e4, 6.1e4 around
                  the origin: the o_bound threshold 6.0e4 of layout_rules.h between
                  the last two
  giant_inplace   the radii of FIXED replaced by 1e3, 3e4, 5.9e4
  dust_scene      centres times 2^-10, radii times 2^-20
  dust_radii      radii times 2^-12

Cameras, by name: "A" is case A's (0, 4, 50), fov 45, looking down -z; "B" case
B's; the others keep -z and move: `inside` sits at the centre of the first
hostile sphere, `near<j>` three radii in front of the hostile sphere with the
j-th largest |r| (the fov narrowed where the scene is dust), `far` at z = 2^22
(outside huge_r_sparse's 2^20 sphere). A ray set is (camera, width, height);
every scene has A's 44 x 26 and 77 x 45 and its extra cameras at 44 x 26. Each
is both a per-ray batch (index y * W + x) and a ray frame.

Everything is seeded, computed once, read-only and cached, the oracle's results
(hit records of the tree walk and of brute force, colours, camera frames)
included. `hostile(name)` marks the changed spheres in the REORDERED array,
`on_hostile` the rays whose primary hit is one of them.
"""
import functools

import numpy as np

import hostile_ray_cases as hc
import test_planes_cases as cases

abi = cases.abi
N = 1000
F32 = np.float32
FIXED = (137, 500, 863)
DEPTHS = (1, 5, 8)
SIZES = ((44, 26), (77, 45))

SCENES = ("neg_r_sparse", "neg_r_4th", "neg_r_all", "zero_r_4th", "tiny_r", "scales",
          "nan_r_sparse", "nan_r_16th", "nan_c_sparse", "nan_c_16th",
          "inf_r_sparse", "inf_r_4th", "inf_c_sparse", "inf_c_4th",
          "huge_r_sparse", "huge_r_4th", "far_c_sparse", "far_c_4th", "dups", "neg_hidden",
          "giant_wall", "giant_dome_50000", "giant_dome_59900", "giant_dome_61000", "giant_inplace",
          "dust_scene", "dust_radii")
# families whose hostile spheres can be hit: one ray set each with >= 50 primary hits on them
HIT_FAMILIES = {"neg_r": ("neg_r_sparse", "neg_r_4th", "neg_r_all"), "scales": ("scales",),
                "huge_r sparse": ("huge_r_sparse",), "giant wall": ("giant_wall",),
                "dust": ("dust_scene", "dust_radii")}
NEVER_HIT = ("zero_r_4th", "nan_r_sparse", "nan_r_16th", "nan_c_sparse", "nan_c_16th", "inf_r_sparse", "inf_r_4th",
             "inf_c_sparse", "inf_c_4th")   # and tiny_r from k = 75 on
EXTRA_CAMERAS = {"neg_r_sparse": ("inside", "near0"), "neg_r_4th": ("inside",), "neg_r_all": ("inside",),
                 "scales": ("B",), "huge_r_sparse": ("far",), "giant_wall": ("B",), "giant_inplace": ("B",),
                 "giant_dome_50000": ("B",), "dust_scene": ("near0", "near1"), "dust_radii": ("near0", "near1"),
                 "tiny_r": ("near0",)}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def base():
    """The 1000 input spheres, in input order."""
    return _frozen(cases._oracle().render_scene(1, N))


def _every(step):
    return np.arange(N) % step == 0


@functools.lru_cache(maxsize=None)
def exponents(name):
    lo, hi, seed = {"tiny_r": (10, 140, 61), "scales": (-16, 2, 62), "huge_r_4th": (20, 127, 63),
                    "far_c_4th": (10, 100, 64)}[name]
    return _frozen(np.random.default_rng(seed).integers(lo, hi + 1, N))


def _pow2(k):
    return np.ldexp(np.float64(1.0), k)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(input spheres, bool mask of the hostile ones), both in input order."""
    s = base().copy()
    r, c = s["radius"], s["center"]
    fixed = np.zeros(N, bool)
    fixed[list(FIXED)] = True
    kind, _, variant = name.rpartition("_")
    m = {"sparse": fixed, "4th": _every(4), "16th": _every(16), "all": np.ones(N, bool)}.get(variant)
    idx = None if m is None else np.flatnonzero(m)
    j = None if m is None else np.arange(len(idx))
    if kind == "neg_r":
        r[m] = -r[m]
    elif kind == "zero_r":
        r[m] = 0.0
    elif name == "tiny_r":
        m = np.arange(N) % 2 == 1
        r[m] = (r[m].astype(np.float64) * _pow2(-exponents(name)[m])).astype(F32)
    elif name == "scales":
        m = np.ones(N, bool)
        r[:] = (r.astype(np.float64) * _pow2(exponents(name))).astype(F32)
    elif kind == "nan_r":
        r[m] = np.nan
    elif kind == "nan_c":
        c[idx, j % 3] = np.nan
    elif kind == "inf_r":
        r[idx] = np.where(j % 2 == 0, np.inf, -np.inf)
    elif kind == "inf_c":
        c[idx, j % 3] = np.where((j // 3) % 2 == 0, np.inf, -np.inf)
    elif name == "huge_r_sparse":
        r[idx] = _pow2(np.array([20, 64, 127]))
    elif name == "huge_r_4th":
        r[idx] = _pow2(exponents(name)[idx])
    elif name == "far_c_sparse":
        c[idx, j % 3] = (c[idx, j % 3].astype(np.float64) * _pow2(np.array([10, 50, 100]))).astype(F32)
    elif name == "far_c_4th":
        c[idx, j % 3] = (c[idx, j % 3].astype(np.float64) * _pow2(exponents(name)[idx])).astype(F32)
    elif name == "dups":
        s[1::2] = s[0::2]
        m = np.ones(N, bool)
    elif name == "neg_hidden":
        m = np.arange(N) < 2
        s[1] = s[0]
        r[0] = -6.0
    elif name == "giant_wall":
        m = np.arange(N) == 0
        zmin = float((base()["center"][:, 2] - base()["radius"]).min())
        c[0] = (0.0, 0.0, zmin - 3.0e4)
        r[0] = 3.0e4
    elif kind == "giant_dome":
        m = np.arange(N) == 0
        c[0] = (0.0, 0.0, 0.0)
        r[0] = float(variant)
    elif name == "giant_inplace":
        m = fixed
        r[list(FIXED)] = (1.0e3, 3.0e4, 5.9e4)
    elif name == "dust_scene":
        m = np.ones(N, bool)
        c[:] = c * F32(2.0 ** -10)
        r[:] = r * F32(2.0 ** -20)
    elif name == "dust_radii":
        m = np.ones(N, bool)
        r[:] = r * F32(2.0 ** -12)
    else:
        raise KeyError(name)
    return _frozen(s), _frozen(m.copy())


@functools.lru_cache(maxsize=None)
def scene(name):
    """(spheres as the oracle's build reordered them, its tree handle, the flat tree)."""
    o = cases._oracle()
    s = inputs(name)[0].copy()
    tree = o.build(s)
    return _frozen(s), tree, _frozen(o.flatten(tree))


@functools.lru_cache(maxsize=None)
def hostile(name):
    """bool mask over the REORDERED spheres: the ones the scene changed (a build only permutes: the 20 bytes of
    a sphere find its input index; byte-equal spheres are equally hostile)."""
    s_in, m = inputs(name)
    where = {s_in[i].tobytes(): bool(m[i]) for i in range(N)}
    s = scene(name)[0]
    return _frozen(np.array([where[s[i].tobytes()] for i in range(N)]))


# ---------------------------------------------------------------- cameras and rays

def _largest(name, j):
    """The hostile sphere (input order) with the j-th largest finite |r|."""
    s, m = inputs(name)
    r = np.where(m & np.isfinite(s["radius"]), np.abs(s["radius"]), -1.0)
    return s[np.argsort(-r, kind="stable")[j]]


def camera(name, cam):
    out = cases.camera("B" if cam == "B" else "A")
    if cam in ("A", "B"):
        return out
    if cam == "inside":
        s, m = inputs(name)
        p = s["center"][np.flatnonzero(m)[0]]
    elif cam == "far":
        p = (0.0, 0.0, 2.0 ** 22)
    elif cam.startswith("near"):
        sp = _largest(name, int(cam[4:]))
        p = sp["center"].astype(np.float64) + (0.0, 0.0, 3.0 * abs(float(sp["radius"])))
    else:
        raise KeyError(cam)
    out.position = abi.Vec3(*[float(F32(v)) for v in p])
    return out


def ray_sets(name):
    return [("A", w, h) for w, h in SIZES] + [(cam, *SIZES[0]) for cam in EXTRA_CAMERAS.get(name, ())]


@functools.lru_cache(maxsize=None)
def rays(name, cam, w, h):
    """(h, w) abi.RAY: the camera's own rays, from the oracle. (A's depend on no scene: one array.)"""
    if cam in ("A", "B") and name is not None:
        return rays(None, cam, w, h)
    return _frozen(cases._oracle().camera_rays(camera(name, cam), w, h))


@functools.lru_cache(maxsize=None)
def hits(name, cam, w, h, use_bvh=True):
    s, tree, _ = scene(name)
    flat = np.ascontiguousarray(rays(name, cam, w, h)).reshape(-1)
    return _frozen(cases._oracle().intersect(tree, s, flat, use_bvh).reshape(h, w))


@functools.lru_cache(maxsize=None)
def colours(name, cam, w, h, depth=5, use_bvh=True, seed=1, sample=0):
    """Oracle.trace_rays of the ray set (pixel index y * w + x), (h, w, 4)."""
    s, tree, _ = scene(name)
    flat = np.ascontiguousarray(rays(name, cam, w, h)).reshape(-1)
    return _frozen(cases._oracle().trace_rays(flat, s, tree, depth=depth, use_bvh=bool(use_bvh), seed=seed,
                                              sample=sample).reshape(h, w, 4))


@functools.lru_cache(maxsize=None)
def camera_frame(name, cam, w, h, use_bvh=True, depth=5, seed=1, sample=0):
    """Oracle.render of the camera, (h, w, 4)."""
    s, tree, _ = scene(name)
    return _frozen(cases._oracle().render(camera(name, cam), w, h, s, tree, depth=depth, use_bvh=use_bvh, mode=1,
                                          seed=seed, sample=sample))


def planes(name, cam, w, h, use_bvh=True):
    return cases.planes_of(hits(name, cam, w, h, use_bvh), (h, w))


def on_hostile(name, cam, w, h, use_bvh=True):
    """(h, w) bool: the rays whose recorded sphere is a hostile one."""
    rec = hits(name, cam, w, h, use_bvh)
    return (rec["hit"] != 0) & hostile(name)[np.clip(rec["sphere"], 0, N - 1)]


def nan_elements(records):
    return hc.nan_elements(records)


def tree_depth(nodes):
    """The deepest node's depth (the root's is 0)."""
    ends, deepest = [], 0
    skip = (nodes["skip"] & abi.SKIP_MASK).astype(np.int64)
    for i in range(len(nodes)):
        while ends and ends[-1] <= i:
            ends.pop()
        deepest = max(deepest, len(ends))
        if nodes["sphere"][i] < 0:
            ends.append(int(skip[i]))
    return deepest


def counts(name, cam="A", w=44, h=26):
    """The figures MEASUREMENTS.md records per scene and ray set, from the oracle alone."""
    rec, brute = hits(name, cam, w, h), hits(name, cam, w, h, False)
    nodes = scene(name)[2]
    return dict(nodes=len(nodes), hits=int((rec["hit"] != 0).sum()), on_hostile=int(on_hostile(name, cam, w, h).sum()),
                nan_elements=nan_elements(rec), brute_hits=int((brute["hit"] != 0).sum()),
                brute_on_hostile=int(on_hostile(name, cam, w, h, False).sum()), brute_nan_elements=nan_elements(brute),
                tree_vs_brute_records=int((rec["sphere"] != brute["sphere"]).sum()),
                tree_vs_brute_colours=int((colours(name, cam, w, h) != colours(name, cam, w, h, use_bvh=False))
                                          .any(-1).sum()))


def mask_shares(name, cam="A"):
    """Per lane mask of hostile_ray_cases.mask (44 x 26): the share of the mask's rays, and of the other rays,
    that hit a hostile sphere -- where such rays sit beside ordinary ones in a wave, a quad and a tile."""
    on = on_hostile(name, cam, *SIZES[0])
    return {m: (round(float(on[hc.mask(m)].mean()), 3), round(float(on[~hc.mask(m)].mean()), 3)) for m in hc.MASKS}

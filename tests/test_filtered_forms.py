"""The filtered box and sphere tests of csrc/trace.h against the CPU oracle,
pair by pair, on inputs aimed at their error margins.

Every fast path of the walks (slab_fast, slab_cons_fast with and without
margins, sphere_t<true>, the Prune entry test) decides an outcome only where
a hand-written bound says hit.c would decide the same. The walks meet a ray
within a few margins of a decision by accident; here every pair is built to
lie there: rays grazing box edges, origins on faces and sphere surfaces,
silhouette rays, directions scaled until the quadratic under- and overflows,
components around the 2^-40 `generic` threshold, scenes at and beyond the
fp16 range. The diagnostic entry points (mirt_box_form_pairs,
mirt_sphere_form_pairs) call the same device functions as the walks.

The reference of every assertion is oracle.aabb_pairs / sphere_pairs /
intersect (the C restatement of hit.c on the CPU); comparisons are exact
(flags, bit patterns, bytes). The numpy float32 restatements below only
CLASSIFY pairs, to assert that the inputs do sit at the margins.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
EPS = F32(0.000001)   # constants.h:6
TINY = F32(2.0 ** -40)  # trace.h slab_ray: below it a direction component is `generic`


# ---------------------------------------------------------------- helpers

def _abi():
    from importlib import import_module
    return import_module("cs201_sah-bvh_ray_tracer_amd").abi


def _rays(o, d):
    r = np.zeros(len(o), _abi().RAY)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        r["origin"] = o
        r["direction"] = d
    return r


def _boxes(lo, hi):
    b = np.zeros(len(lo), _abi().AABB)
    b["min"] = lo
    b["max"] = hi
    return b


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _cat(parts):
    return np.concatenate(parts)


def _oinf(rays):
    # numpy's max propagates a NaN, which then compares false ("beyond the bound"). The device's fmaxf DROPS a
    # NaN component (bounce_slab_ray, prune_m0), so there an origin with a NaN and two small components counts
    # as within the bound; no family here has such an origin (tests/test_hostile_rays_gpu.py runs them)
    return np.abs(rays["origin"]).max(axis=1)


def _generic(rays):
    return ~(np.abs(rays["direction"]) >= TINY).all(axis=1)


def _f64(a):
    return np.asarray(a, F32).astype(np.float64)


# ---------------------------------------------------------------- box families

def _box_geometry(rng, n, shift, snap):
    corner = rng.uniform(-50, 50, (n, 3))
    side = 10.0 ** rng.uniform(-2, 1.5, (n, 3))
    if snap:   # planes that fp16 stores exactly: halves and integers below 2048, and 0
        corner = np.round(corner * 2) / 2
        side = np.maximum(np.round(side * 2) / 2, 0.5)
        corner[rng.random((n, 3)) < 0.1] = 0.0
    lo = _f64(corner + shift)
    hi = _f64(lo + side)
    return lo, hi


def edge_grazing(rng, n, shift=0.0, snap=False, origin_hook=None):
    """Rays through a point on a box edge moved in or out by a relative
    2^[-26, -14], from 1-100 box diagonals away; half of the directions
    normalised, half not."""
    lo, hi = _box_geometry(rng, n, shift, snap)
    ar = np.arange(n)
    ctr = (lo + hi) / 2
    p = np.where(rng.random((n, 3)) < 0.5, lo, hi)
    ax = rng.integers(0, 3, n)   # the axis the edge runs along
    run = lo[ar, ax] + rng.random(n) * (hi - lo)[ar, ax]
    p[ar, ax] = run
    move = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-26, -14, n)
    q = ctr + (p - ctr) * (1 + move)[:, None]
    q[ar, ax] = run
    diag = np.linalg.norm(hi - lo, axis=1)
    o = ctr + _unit(rng, n) * (diag * rng.uniform(1, 100, n))[:, None]
    if origin_hook is not None:
        o = origin_hook(o)
    o = _f64(o)
    d = q - o
    norm = np.linalg.norm(d, axis=1)
    scale = np.where(rng.random(n) < 0.5, 1 / norm, 2.0 ** rng.uniform(-6, 6, n) / norm)
    return _rays(o, d * scale[:, None]), _boxes(lo, hi)


def face_origins(rng, n, shift=0.0, snap=False):
    """What bounce rays are: the origin on a box face, directions over the
    whole sphere."""
    lo, hi = _box_geometry(rng, n, shift, snap)
    ar = np.arange(n)
    o = lo + rng.random((n, 3)) * (hi - lo)
    ax = rng.integers(0, 3, n)
    o[ar, ax] = np.where(rng.random(n) < 0.5, lo[ar, ax], hi[ar, ax])
    d = _unit(rng, n) * np.where(rng.random(n) < 0.5, 1.0, 2.0 ** rng.uniform(-6, 6, n))[:, None]
    return _rays(o, d), _boxes(lo, hi)


def scale_directions(rng, rays):
    """|d| from 2^-70 to 2^60: a = d.d, 2a and the discriminant under- and
    overflow; the reciprocals leave the normal range."""
    out = rays.copy()
    k = rng.integers(-70, 61, len(rays))
    with np.errstate(over="ignore", under="ignore"):
        out["direction"] = (rays["direction"].astype(np.float64) * (2.0 ** k)[:, None]).astype(F32)
    return out


def poke_directions(rng, rays):
    """One or two components at 0, -0, a denormal, or 2^-41 .. 2^-39 around
    the `generic` threshold, either sign."""
    out = rays.copy()
    t = float(TINY)
    vals = np.array([0.0, -0.0, 1e-42, -1e-42, t / 2, -t / 2, t, -t, 2 * t, -2 * t,
                     float(np.nextafter(TINY, F32(0))), float(np.nextafter(TINY, F32(1)))], F32)
    n = len(rays)
    ar = np.arange(n)
    d = out["direction"]
    d[ar, rng.integers(0, 3, n)] = vals[rng.integers(0, len(vals), n)]
    two = rng.random(n) < 0.25
    d[ar[two], rng.integers(0, 3, n)[two]] = vals[rng.integers(0, len(vals), n)[two]]
    return out


def non_finite_pairs(rng, like_rays, like_second):
    """A few inf / NaN origins and directions on otherwise ordinary pairs."""
    n = 96
    rays = like_rays[:n].copy()
    vals = np.array([np.inf, -np.inf, np.nan], F32)
    ar = np.arange(n)
    field = np.where(ar % 2 == 0, 0, 1)
    comp = rng.integers(0, 3, n)
    v = vals[ar % 3]
    rays["origin"][ar[field == 0], comp[field == 0]] = v[field == 0]
    rays["direction"][ar[field == 1], comp[field == 1]] = v[field == 1]
    return rays, like_second[:n].copy()


def box_family_set(rng, n, shift=0.0):
    """name -> (rays, boxes): the edge-grazing and face-origin families, their
    fp16-exact variants, and the direction-scale variants of both."""
    fam = {
        "edge": edge_grazing(rng, n, shift),
        "edge_fp16_exact": edge_grazing(rng, n // 2, shift, snap=True),
        "face": face_origins(rng, n, shift),
        "face_fp16_exact": face_origins(rng, n // 2, shift, snap=True),
    }
    for base in ("edge", "face"):
        r, b = fam[base]
        fam[base + "_scaled"] = (scale_directions(rng, r[: n // 2]), b[: n // 2])
        fam[base + "_poked"] = (poke_directions(rng, r[: n // 2]), b[: n // 2])
    return fam


SHIFTS = {"unit": 0.0, "3000": 3000.0, "5.9e4": 5.9e4, "6.1e4": 6.1e4}


def _shift_vec(rng, name):
    """The families moved by the named magnitude along a random signed subset
    of the axes (at least one)."""
    s = SHIFTS[name]
    m = rng.integers(0, 2, 3)
    m[rng.integers(0, 3)] = 1
    return s * m * rng.choice([-1.0, 1.0], 3)


def classify_slab_fast(rays, boxes):
    """numpy float32 restatement (no fma) of slab_fast's gap, above and m for
    the rays that take it: (took, decided, near, undecided) masks, `near`
    being decided with the deciding quantity within 64 m. Classification
    only -- never the subject of an assertion about the kernel."""
    o, d = rays["origin"], rays["direction"]
    took = ~_generic(rays) & np.isfinite(o).all(1) & np.isfinite(d).all(1)
    with np.errstate(all="ignore"):
        inv = F32(1) / d
        oi = o * inv
        t1 = boxes["min"] * inv - oi
        t2 = boxes["max"] * inv - oi
        tmin = np.minimum(t1, t2).max(1)
        tmax = np.maximum(t1, t2).min(1)
        mo = np.abs(oi).max(1) * F32(2.0 ** -22)
        m = (np.abs(tmin) + np.abs(tmax)) * F32(2.0 ** -20) + F32(2) * mo
        gap = tmax - tmin
        above = tmax - EPS
        passed = (gap > m) & (above > m)
        failed = (gap < -m) | (above < -m)
        decided = took & (passed | failed)
        near = decided & ((np.abs(gap) <= 64 * m) | (np.abs(above) <= 64 * m))
        undecided = took & ~(passed | failed)
    return took, decided, near, undecided


# ---------------------------------------------------------------- sphere families

def sphere_pool(rng, n, shift=0.0):
    abi = _abi()
    s = np.zeros(n, abi.SPHERE)
    s["center"] = rng.uniform(-50, 50, (n, 3)) + shift
    s["radius"] = 10.0 ** rng.uniform(-1, 1.5, n)
    i = np.arange(n)
    s["color"] = np.stack([(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 17) % 256, np.full(n, 255)], 1)
    return s


def silhouette(rng, pool, n):
    """Aimed at c + u r (1 +- 10^[-8, -2]), u perpendicular to c - o."""
    i = rng.integers(0, len(pool), n)
    c, r = _f64(pool["center"][i]), _f64(pool["radius"][i])
    o = _f64(c + _unit(rng, n) * (r * 10.0 ** rng.uniform(0.3, 2.5, n))[:, None])
    w = c - o
    u = np.cross(w, _unit(rng, n))
    u /= np.linalg.norm(u, axis=1)[:, None]
    f = 1 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, -2, n)
    d = c + u * (r * f)[:, None] - o
    norm = np.linalg.norm(d, axis=1)
    scale = np.where(rng.random(n) < 0.5, 1 / norm, 2.0 ** rng.uniform(-6, 6, n) / norm)
    return _rays(o, d * scale[:, None]), pool[i].copy(), i


def surface_origins(rng, pool, n):
    """Origin on the sphere's own surface (a bounce ray against the sphere it
    left), directions over the whole sphere: the recorded t is the near root,
    a rounding residue around EPS."""
    i = rng.integers(0, len(pool), n)
    c, r = _f64(pool["center"][i]), _f64(pool["radius"][i])
    o = c + _unit(rng, n) * r[:, None]
    return _rays(o, _unit(rng, n)), pool[i].copy(), i


def through_spheres(rng, pool, n):
    """Rays that hit the sphere squarely, from outside -- the hits whose t the
    pruning bound and the best-so-far comparisons are about."""
    i = rng.integers(0, len(pool), n)
    c, r = _f64(pool["center"][i]), _f64(pool["radius"][i])
    o = _f64(c + _unit(rng, n) * (r * 10.0 ** rng.uniform(0.1, 2, n))[:, None])
    d = c + _unit(rng, n) * (r * rng.random(n))[:, None] - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    d *= np.where(rng.random(n) < 0.5, 1.0, 2.0 ** rng.uniform(-6, 6, n))[:, None]
    return _rays(o, d), pool[i].copy(), i


def axis_rays(rng, pool, n):
    """Zero-component and sub-2^-40 directions that still meet the sphere:
    along one axis (or nearly), offset from the centre by less than r."""
    i = rng.integers(0, len(pool), n)
    c, r = _f64(pool["center"][i]), _f64(pool["radius"][i])
    ar = np.arange(n)
    ax = rng.integers(0, 3, n)
    off = _unit(rng, n) * (r * rng.random(n))[:, None]
    off[ar, ax] = 0.0
    d = np.zeros((n, 3))
    d[ar, ax] = rng.choice([-1.0, 1.0], n) * np.where(rng.random(n) < 0.5, 1.0, 2.0 ** rng.uniform(-6, 6, n))
    o = c + off - d / np.abs(d[ar, ax])[:, None] * (r * rng.uniform(1.5, 30, n))[:, None]
    small = np.array([0.0, -0.0, 2.0 ** -45, -2.0 ** -45, 2.0 ** -41, 1e-42])
    for k in (1, 2):   # the other two components: zero, or too small to be normal-range reciprocals
        d[ar, (ax + k) % 3] = small[rng.integers(0, len(small), n)]
    return _rays(o, d), pool[i].copy(), i


def sphere_family_set(rng, pool, n):
    fam = {
        "silhouette": silhouette(rng, pool, n),
        "surface": surface_origins(rng, pool, n),
        "through": through_spheres(rng, pool, n // 2),
        "axis": axis_rays(rng, pool, n // 4),
    }
    for base in ("silhouette", "surface"):
        r, s, i = fam[base]
        fam[base + "_scaled"] = (scale_directions(rng, r[: n // 2]), s[: n // 2], i[: n // 2])
        fam[base + "_poked"] = (poke_directions(rng, r[: n // 2]), s[: n // 2], i[: n // 2])
    return fam


def classify_sphere_filter(rays, spheres, best):
    """numpy float32 restatement of sphere_t<true>'s estimate te and margin M:
    |te - best| <= 64 M. Classification only."""
    with np.errstate(all="ignore"):
        o, d = rays["origin"], rays["direction"]
        oc = o - spheres["center"]

        def dot(a, b):
            return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        a = dot(d, d)
        b = F32(2) * dot(oc, d)
        c = dot(oc, oc) - spheres["radius"] * spheres["radius"]
        disc = b * b - (F32(4) * a) * c
        sq = np.sqrt(np.maximum(disc, F32(0)))
        inv2a = F32(1) / (F32(2) * a)
        te = (-b - sq) * inv2a
        m = (np.abs(b) + sq) * np.abs(inv2a) * F32(2.0 ** -18)
        return np.abs(te - best) <= 64 * m


# ---------------------------------------------------------------- scenes

def two_sphere_scene(mirt, S):
    """A scene whose coordinate bound is S: unit spheres at (+-(S - 1), 0, 0)."""
    s = np.zeros(2, mirt.abi.SPHERE)
    s["center"] = [[S - 1, 0, 0], [-(S - 1), 0, 0]]
    s["radius"] = 1
    s["color"] = [[200, 30, 30, 255], [30, 30, 200, 255]]
    return s, mirt.build_bvh(s)


def origin_bound(spheres, nodes):
    """Host restatement of the upload's bound C (DevScene::o_bound) and of the
    growth 2^-19 C: (C as float32 or 0 when the scene has none, growth)."""
    abi = _abi()
    c_max = F32(0)
    for s in spheres:
        c_max = max(c_max, F32(np.abs(s["center"]).max()) + F32(abs(s["radius"])))
    cb = float(c_max)
    for nd in nodes:
        if nd["skip"] & abi.NODE_EMPTY:
            continue
        v = np.concatenate([nd["bmin"], nd["bmax"]])
        v = np.abs(v[np.isfinite(v)])
        if len(v):
            cb = max(cb, float(v.max()))
    cb = cb * (1.0 + 2.0 ** -10) + 2.0 ** -10
    if not cb < 6.0e4:
        return F32(0), 0.0
    return F32(cb), cb * 2.0 ** -19


def grown(boxes, grow, fp16):
    """The box as the upload stores it: each face moved out by `grow` and
    rounded outward (build_pnodes), then, for the four-wide nodes, rounded
    outward to fp16 (build_hnodes)."""
    out = boxes.copy()
    lo = np.nextafter((boxes["min"].astype(np.float64) - grow).astype(F32), F32(-np.inf))
    hi = np.nextafter((boxes["max"].astype(np.float64) + grow).astype(F32), F32(np.inf))
    if fp16:
        hl = lo.astype(np.float16)
        hl = np.where(hl.astype(F32) > lo, np.nextafter(hl, np.float16(-np.inf)), hl)
        hh = hi.astype(np.float16)
        hh = np.where(hh.astype(F32) < hi, np.nextafter(hh, np.float16(np.inf)), hh)
        assert (hl.astype(F32) <= lo).all() and (hh.astype(F32) >= hi).all()
        lo, hi = hl.astype(F32), hh.astype(F32)
    out["min"], out["max"] = lo, hi
    return out


def _share(mask):
    return float(np.mean(mask)) if len(mask) else 0.0


def _assert_both_outcomes(name, ref):
    p = _share(ref != 0)
    print(f"  {name}: {len(ref)} pairs, oracle passes {100 * p:.1f}%")
    assert 0.10 <= p <= 0.90, f"{name}: oracle outcome share {p:.3f} leaves one outcome below 10%"


# ---------------------------------------------------------------- P1 / P2

N_BOX = 40_000   # per base family and magnitude


@pytest.fixture(scope="module")
def box_cases(oracle):
    """magnitude -> (rays, boxes, oracle flags, {family: slice}); computed once."""
    cases = {}
    for k, name in enumerate(SHIFTS):
        rng = np.random.default_rng(1000 + k)
        fam = box_family_set(rng, N_BOX, _shift_vec(rng, name))
        fam["non_finite"] = non_finite_pairs(rng, *fam["edge"])
        parts, at = {}, 0
        for f, (r, b) in fam.items():
            parts[f] = slice(at, at + len(r))
            at += len(r)
        rays = _cat([fam[f][0] for f in fam])
        boxes = _cat([fam[f][1] for f in fam])
        cases[name] = (rays, boxes, oracle.aabb_pairs(rays, boxes), parts)
    return cases


@pytest.fixture()
def unit_scene(gpu, mirt):
    s, b = two_sphere_scene(mirt, 100.0)
    gpu.upload(s, b)
    return s, b


@pytest.mark.parametrize("mag", list(SHIFTS))
def test_p1_exact_forms_equal_the_oracle(gpu, mirt, box_cases, unit_scene, mag):
    """P1: slab<true> and slab_box<true>, pruning off, equal hit.c's flag on
    every pair, generic rays included; and the families do sit at slab_fast's
    margins."""
    abi = mirt.abi
    rays, boxes, ref, parts = box_cases[mag]
    best = np.full(len(rays), INF)
    for f in ("edge", "edge_fp16_exact", "face", "face_fp16_exact"):
        _assert_both_outcomes(f"{mag}/{f}", ref[parts[f]])
    took, decided, near, undecided = classify_slab_fast(rays, boxes)
    e = parts["edge"]
    print(f"  {mag}/edge: filter decides within 64 margins {100 * _share(near[e]):.1f}%, "
          f"undecided {100 * _share(undecided[e]):.1f}%; all families: {100 * _share(near):.1f}% / "
          f"{100 * _share(undecided):.1f}%, generic {100 * _share(~took):.1f}%")
    assert _share(near[e]) >= 0.05 and _share(undecided[e]) >= 0.05
    assert _share(near) >= 0.05 and _share(undecided) >= 0.05
    assert _share(~took) >= 0.05   # the exact fallback for zero / tiny components runs too
    try:
        gpu.set_option(abi.OPT_PRUNE, 0)
        for form in (abi.BOX_FORM_SLAB, abi.BOX_FORM_SLAB_BOX):
            got = gpu.box_form_pairs(rays, boxes, best, form)
            bad = np.flatnonzero(got != ref)
            assert len(bad) == 0, (f"form {form}: {len(bad)} pairs differ from the oracle, first "
                                   f"{rays[bad[0]]} {boxes[bad[0]]} oracle {ref[bad[0]]}")
    finally:
        gpu.set_option(abi.OPT_PRUNE, 1)


@pytest.mark.parametrize("mag", list(SHIFTS))
def test_p2_conservative_form_loses_no_pass(gpu, mirt, box_cases, unit_scene, mag):
    """P2: slab_cons<false>, pruning off, passes every pair hit.c passes."""
    abi = mirt.abi
    rays, boxes, ref, _ = box_cases[mag]
    try:
        gpu.set_option(abi.OPT_PRUNE, 0)
        got = gpu.box_form_pairs(rays, boxes, np.full(len(rays), INF), abi.BOX_FORM_CONS)
    finally:
        gpu.set_option(abi.OPT_PRUNE, 1)
    lost = np.flatnonzero((ref != 0) & (got == 0))
    print(f"  {mag}: extra passes {100 * _share((got != 0) & (ref == 0)):.2f}% of {len(ref)} pairs")
    assert len(lost) == 0, f"{len(lost)} passes lost, first {rays[lost[0]]} {boxes[lost[0]]}"
    assert (ref != 0).sum() > len(ref) // 10


# ---------------------------------------------------------------- P3

def _bound_origins(rng, C):
    """Origin hook: a quarter of the origins as generated, the rest with one
    coordinate at +-C, +-nextabove(C), +-4C or +-nextabove(4C) (float32) and
    the others within C."""
    C = F32(C)
    edge = np.array([C, np.nextafter(C, INF), F32(4) * C, np.nextafter(F32(4) * C, INF)], F32).astype(np.float64)

    def hook(o):
        n = len(o)
        ar = np.arange(n)
        kind = rng.integers(0, 6, n)
        put = kind < 4
        o = np.where(put[:, None], np.clip(o, -float(C), float(C)), o)
        ax = rng.integers(0, 3, n)
        v = edge[np.minimum(kind, 3)] * rng.choice([-1.0, 1.0], n)
        o[ar[put], ax[put]] = v[put]
        return o
    return hook


@pytest.mark.parametrize("S,shift", [(100.0, "unit"), (3100.0, "3000"), (59900.0, "5.9e4")])
def test_p3_margin_free_form_on_grown_boxes(gpu, mirt, oracle, S, shift):
    """P3: slab_cons<true> on the box as the upload stores it (grown by
    2^-19 C, with and without the outward fp16 rounding) passes every pair
    hit.c passes on the un-grown box, for origins within C (bounce rule) or 4C
    (camera rule); an origin beyond the bound takes the exact path and so
    equals hit.c on the stored box."""
    abi = mirt.abi
    s, b = two_sphere_scene(mirt, S)
    C, grow = origin_bound(s, b.nodes)
    assert C > 0 and abs(float(C) - (S * (1 + 2.0 ** -10) + 2.0 ** -10)) <= S * 2.0 ** -23
    gpu.upload(s, b)
    rng = np.random.default_rng(int(S))
    sv = _shift_vec(rng, shift)
    hook = _bound_origins(rng, C)
    sets = [edge_grazing(rng, N_BOX, sv, origin_hook=hook),
            edge_grazing(rng, N_BOX, sv, snap=True, origin_hook=hook),
            edge_grazing(rng, N_BOX // 2, sv),
            face_origins(rng, N_BOX, sv), face_origins(rng, N_BOX // 2, sv, snap=True)]
    rays = _cat([r for r, _ in sets])
    boxes = _cat([bx for _, bx in sets])
    rays = _cat([rays, poke_directions(rng, rays[::4]), scale_directions(rng, rays[1::4])])
    boxes = _cat([boxes, boxes[::4], boxes[1::4]])
    assert np.abs(_cat([boxes["min"], boxes["max"]])).max() <= C   # the lemma's premise on the boxes
    ref = oracle.aabb_pairs(rays, boxes)
    best = np.full(len(rays), INF)
    oi = _oinf(rays)
    # pruning off: with it, the exact path also drops what pruned_any's zero-component test drops -- boxes hit.c
    # passes although the ray never enters them; P5 is about that
    try:
        gpu.set_option(abi.OPT_PRUNE, 0)
        for fp16 in (False, True):
            stored = grown(boxes, grow, fp16)
            ref_stored = oracle.aabb_pairs(rays, stored)
            for form, bound in ((abi.BOX_FORM_CONS_BOUNCE, C), (abi.BOX_FORM_CONS_CAMERA, F32(4) * C)):
                inside = oi <= bound
                got = gpu.box_form_pairs(rays, stored, best, form)
                bare = gpu.box_form_pairs(rays, boxes, best, form)
                needs = (ref != 0) & inside
                print(f"  S {S:g} fp16 {fp16} form {form}: {int(inside.sum())} origins inside, {int((~inside).sum())} "
                      f"beyond; oracle passes {int(needs.sum())} inside; without the growth the form would lose "
                      f"{int((needs & (bare == 0)).sum())}; extra passes {int((inside & (got != 0) & (ref == 0)).sum())}")
                assert inside.sum() > len(rays) // 10 and (~inside).sum() > len(rays) // 50
                assert needs.sum() > len(rays) // 20 and ((ref == 0) & inside).sum() > len(rays) // 100
                lost = np.flatnonzero(needs & (got == 0))
                assert len(lost) == 0, (f"form {form} fp16 {fp16}: {len(lost)} passes lost, first "
                                        f"{rays[lost[0]]} {boxes[lost[0]]} stored {stored[lost[0]]}")
                bad = np.flatnonzero(~inside & (got != ref_stored))
                assert len(bad) == 0, (f"form {form} fp16 {fp16}: {len(bad)} origins beyond the bound differ from "
                                       f"the oracle, first {rays[bad[0]]} {stored[bad[0]]}")
    finally:
        gpu.set_option(abi.OPT_PRUNE, 1)
    if shift == "unit":   # planes that fp16 stores exactly: only the growth separates the stored box from hit.c's
        lo = sets[1][1]["min"]
        assert (lo.astype(np.float16).astype(F32) == lo).all() and (lo == 0).mean() > 0.05


# ---------------------------------------------------------------- P4

N_SPH = 24_000


def _next(t, up):
    return np.nextafter(t, INF if up else -INF)


def _best_list(t, hit):
    """best values around the recorded t (hits) or fixed ones (misses)."""
    one = F32(1)
    with np.errstate(all="ignore"):
        around = [t, _next(t, False), _next(t, True),
                  t * (one + F32(2.0 ** -18)), t * (one - F32(2.0 ** -18)),
                  t * (one + F32(2.0 ** -17)), t * (one - F32(2.0 ** -17))]
    fixed = [F32(1), F32(1e-3), F32(100), F32(1e4), F32(3e-6), F32(1e-5), F32(0.5)]
    out = [np.full(len(t), INF), np.full(len(t), EPS), np.full(len(t), _next(EPS, True))]
    for a, f in zip(around, fixed):
        out.append(np.where(hit, a, f).astype(F32))
    return out


@pytest.fixture(scope="module")
def sphere_cases(oracle):
    cases = {}
    for k, name in enumerate(SHIFTS):
        rng = np.random.default_rng(2000 + k)
        pool = sphere_pool(rng, 2048, _shift_vec(rng, name))
        fam = sphere_family_set(rng, pool, N_SPH)
        r0, s0, _ = fam["silhouette"]
        nf_r, nf_s = non_finite_pairs(rng, r0, s0)
        fam["non_finite"] = (nf_r, nf_s, None)
        parts, at = {}, 0
        for f, v in fam.items():
            parts[f] = slice(at, at + len(v[0]))
            at += len(v[0])
        rays = _cat([fam[f][0] for f in fam])
        sph = _cat([fam[f][1] for f in fam])
        cases[name] = (rays, sph, oracle.sphere_pairs(rays, sph), parts)
    return cases


@pytest.mark.parametrize("mag", list(SHIFTS))
def test_p4_filtered_sphere_test_equals_the_oracle(gpu, mirt, sphere_cases, mag):
    """P4: sphere_t<true>(best) has the bits of sphere_t<false>(best), and
    both are hit.c's t when it hits with t <= best, else -1, for best at, one
    ulp around, and 2^-18 / 2^-17 around the recorded t, at EPS, and +inf."""
    rays, sph, ref, parts = sphere_cases[mag]
    hit = ref["hit"] != 0
    t = ref["t"]
    if mag in ("unit", "3000"):
        _assert_both_outcomes(f"{mag}/silhouette", hit[parts["silhouette"]])
    if mag == "unit":
        sh = hit[parts["surface"]]
        st = t[parts["surface"]][sh]
        print(f"  surface origins: {100 * _share(sh):.1f}% hit, t < 1e-3 {100 * _share(st < 1e-3):.1f}%, "
              f"t < 1e-5 {100 * _share(st < 1e-5):.1f}%")
        assert 0.10 <= _share(sh) <= 0.90 and _share(st < 1e-3) > 0.9
    bests = _best_list(t, hit)
    R = _cat([rays] * len(bests))
    S = _cat([sph] * len(bests))
    B = _cat(bests)
    H = _cat([hit] * len(bests))
    T = _cat([t] * len(bests))
    with np.errstate(invalid="ignore"):
        want = np.where(H & (T <= B), T, F32(-1)).astype(F32)
    near = classify_sphere_filter(R, S, B)
    print(f"  {mag}: {len(R)} evaluations, {int(H.sum())} on hits, {100 * _share(near[H]):.1f}% of those within 64 M "
          f"of best; oracle hits {100 * _share(hit):.1f}% of {len(rays)} pairs")
    assert _share(near[H]) >= 0.05 and H.sum() > len(R) // 20
    fast = gpu.sphere_form_pairs(R, S, B, fast=True)
    exact = gpu.sphere_form_pairs(R, S, B, fast=False)
    for name, got in (("sphere_t<false>", exact), ("sphere_t<true>", fast)):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (f"{name}: {len(bad)} of {len(R)} differ from the oracle, first {R[bad[0]]} "
                               f"{S[bad[0]]} best {B[bad[0]]!r}: got {got[bad[0]]!r}, oracle {want[bad[0]]!r}")


# Found by P4 on its first run: hits whose float discriminant is subnormal, from directions of length 1e-18 ..
# 1e-20. v_sqrt_f32 reads a subnormal as zero; with |b| as small, the lost root exceeds the filter's margin and
# sphere_t<true> ruled out a hit at t == best (returned -1 where hit.c records t). (origin, direction, centre,
# radius), float32 as printed:
REGRESSION_SUBNORMAL_DISC = [
    ((24.533575, 30.492432, -32.63027), (-3.2698698e-18, -5.0390267e-18, 4.472186e-19),
     (12.886415, 12.516208, -31.2687), 0.23283343),
    ((-2961.7927, 8.618334, 6.5228534), (4.9334296e-20, -9.309416e-20, 2.5584113e-20),
     (-2960.5205, 7.458422, 6.6698794), 0.6743745),
    ((59024.133, 59034.62, -58985.3), (-1.0065886e-19, -1.0191529e-19, 2.1899454e-19),
     (59015.258, 59025.53, -58966.17), 0.17619625),
    ((60954.79, 32.35749, 60951.984), (-3.101837e-20, 3.5089477e-20, 9.778309e-20),
     (60954.51, 32.483982, 60952.55), 0.12646852),
]


def test_regression_subnormal_discriminant(gpu, mirt, oracle):
    """The named pairs above: the filtered sphere test equals hit.c for every
    best around the recorded t."""
    n = len(REGRESSION_SUBNORMAL_DISC)
    rays = _rays([p[0] for p in REGRESSION_SUBNORMAL_DISC], [p[1] for p in REGRESSION_SUBNORMAL_DISC])
    sph = np.zeros(n, mirt.abi.SPHERE)
    sph["center"] = [p[2] for p in REGRESSION_SUBNORMAL_DISC]
    sph["radius"] = [p[3] for p in REGRESSION_SUBNORMAL_DISC]
    ref = oracle.sphere_pairs(rays, sph)
    assert (ref["hit"] == 1).all() and (ref["t"] > 1e18).all()
    with np.errstate(all="ignore"):   # the case: a positive subnormal float discriminant
        oc = rays["origin"] - sph["center"]
        d = rays["direction"]
        dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]   # noqa: E731
        b = F32(2) * dot(oc, d)
        disc = b * b - (F32(4) * dot(d, d)) * (dot(oc, oc) - sph["radius"] * sph["radius"])
    assert ((disc > 0) & (disc < F32(2.0 ** -126))).all()
    for best in _best_list(ref["t"], ref["hit"] != 0):
        with np.errstate(invalid="ignore"):
            want = np.where(ref["t"] <= best, ref["t"], F32(-1)).astype(F32)
        for fast in (False, True):
            got = gpu.sphere_form_pairs(rays, sph, best, fast=fast)
            assert got.tobytes() == want.tobytes(), (fast, best, got, want)


# ---------------------------------------------------------------- P5

@pytest.mark.parametrize("mag", ["unit", "3000"])
def test_p5_pruning_drops_no_box_that_holds_the_hit(gpu, mirt, oracle, mag):
    """P5: for every pair whose sphere hit.c records at t, a box that contains
    the sphere's leaf box fl(c -+ r) (the leaf box itself, random supersets) is
    not pruned while best >= t: with best in {t, nextabove(t), 2t, inf} the
    exact forms still equal hit.c's flag on the box and the conservative forms
    still pass whatever hit.c passes. (hit.c's own slab test rejects a few
    leaf boxes whose sphere test hits -- grazing rays; its walk never tests
    those spheres, and no form may pass them either where it is exact. They
    are counted below.) The uploaded scene holds the family's spheres, so
    c_max / r_max are the ones the bound assumes."""
    abi = mirt.abi
    rng = np.random.default_rng(77 + len(mag))
    pool = sphere_pool(rng, 2048, _shift_vec(rng, mag))
    bvh = mirt.build_bvh(pool)
    gpu.upload(pool, bvh)
    C, grow = origin_bound(pool, bvh.nodes)
    assert C > 0
    n = 16_000
    fam = [through_spheres(rng, pool, n), silhouette(rng, pool, n), surface_origins(rng, pool, n),
           axis_rays(rng, pool, n)]
    zero_comp = slice(3 * n, 4 * n)
    rays = _cat([f[0] for f in fam])
    sph = _cat([f[1] for f in fam])
    rays = _cat([rays, scale_directions(rng, rays[::4])])
    sph = _cat([sph, sph[::4]])
    ref = oracle.sphere_pairs(rays, sph)
    hit = ref["hit"] != 0
    gen = _generic(rays)
    print(f"  {mag}: {int(hit.sum())} of {len(rays)} pairs hit; zero / tiny-component rays among the hits "
          f"{int((hit & gen).sum())}")
    assert hit[zero_comp].mean() > 0.5 and gen[zero_comp].all()   # pruned_any's own branch has hits to drop
    assert hit.sum() > len(rays) // 4
    rays, sph, t = rays[hit], sph[hit], ref["t"][hit]
    c, r = sph["center"], sph["radius"]
    leaf = _boxes(c - r[:, None], c + r[:, None])   # float32 arithmetic: bvh.c's fl(c -+ r)
    cm = float(np.abs(_cat([bvh.nodes["bmin"], bvh.nodes["bmax"]])).max())
    grow_by = 10.0 ** rng.uniform(-3, 2, (len(leaf), 6))
    sup = _boxes(np.maximum(leaf["min"].astype(np.float64) - grow_by[:, :3], -cm),
                 np.minimum(leaf["max"].astype(np.float64) + grow_by[:, 3:], cm))
    assert (sup["min"] <= leaf["min"]).all() and (sup["max"] >= leaf["max"]).all()
    inside = _oinf(rays) <= C
    with np.errstate(over="ignore"):
        bests = [t, _next(t, True), (F32(2) * t).astype(F32), np.full(len(t), INF)]
    for kind, box in (("leaf", leaf), ("superset", sup)):
        want = oracle.aabb_pairs(rays, box)
        print(f"  {kind}: hit.c's slab test rejects {int((want == 0).sum())} of {len(want)} boxes whose sphere hits")
        assert (want != 0).mean() > 0.9
        for best in bests:
            for form in (abi.BOX_FORM_SLAB, abi.BOX_FORM_SLAB_BOX):
                got = gpu.box_form_pairs(rays, box, best, form)
                bad = np.flatnonzero(got != want)
                assert len(bad) == 0, (f"{kind} form {form}: {len(bad)} differ, first {rays[bad[0]]} "
                                       f"{box[bad[0]]} best {best[bad[0]]!r} oracle {want[bad[0]]}")
            got = gpu.box_form_pairs(rays, box, best, abi.BOX_FORM_CONS)
            lost = np.flatnonzero((want != 0) & (got == 0))
            assert len(lost) == 0, (f"{kind} slab_cons<false>: {len(lost)} pruned, first {rays[lost[0]]} "
                                    f"{box[lost[0]]} best {best[lost[0]]!r}")
            for fp16 in (False, True):
                stored = grown(box, grow, fp16)
                for form in (abi.BOX_FORM_CONS_BOUNCE, abi.BOX_FORM_CONS_CAMERA):
                    got = gpu.box_form_pairs(rays, stored, best, form)
                    lost = np.flatnonzero((want != 0) & (got == 0))
                    assert len(lost) == 0, (f"{kind} form {form} fp16 {fp16}: {len(lost)} pruned, first "
                                            f"{rays[lost[0]]} {stored[lost[0]]} best {best[lost[0]]!r}")
    assert inside.mean() > 0.5


# ---------------------------------------------------------------- the lattice through every walk

def lattice_scene(mirt, far=False):
    """Spheres whose boxes fp16 stores exactly: centres on even integers,
    radii 1 and 0.5, touching neighbours, eight exact duplicates (equal t),
    distinct colours. far: one more sphere beyond 6e4, which leaves the scene
    without an origin bound (o_bound == 0)."""
    abi = mirt.abi
    g = np.arange(-6, 6, 2)
    c = np.array(list(itertools.product(g, g, g)), np.float64)
    r = np.where((c.sum(1) / 2) % 3 == 0, 0.5, 1.0)
    dup = np.arange(0, len(c), 27)[:8]
    c, r = np.concatenate([c, c[dup]]), np.concatenate([r, r[dup]])
    if far:
        c, r = np.concatenate([c, [[7.0e4, 0, 0]]]), np.concatenate([r, [1.0]])
    s = np.zeros(len(c), abi.SPHERE)
    s["center"], s["radius"] = c, r
    i = np.arange(len(c))
    s["color"] = np.stack([(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 17) % 256, np.full(len(c), 255)], 1)
    assert len(s) <= 512 and len(np.unique(s["color"], axis=0)) == len(s)
    return s


def lattice_rays(rng, s, n_each=1900):
    """<= 20k rays at the lattice's silhouettes, box edges and corners, and
    tangent points, from outside, from sphere surfaces and from points exactly
    on box planes."""
    s = s[np.abs(s["center"]).max(1) < 100]
    parts = [silhouette(rng, s, n_each)[0], surface_origins(rng, s, n_each)[0], axis_rays(rng, s, n_each)[0]]
    i = rng.integers(0, len(s), n_each)
    c, r = _f64(s["center"][i]), _f64(s["radius"][i])
    ext = lambda k: c[:k] + _unit(rng, k) * rng.uniform(9, 40, k)[:, None]   # noqa: E731
    # leaf-box corners and edges, moved by a relative 2^[-26, -14]
    sg = rng.choice([-1.0, 1.0], (n_each, 3))
    sg[np.arange(n_each), rng.integers(0, 3, n_each)] *= np.where(rng.random(n_each) < 0.5, 1.0, rng.random(n_each))
    q = c + sg * r[:, None] * (1 + rng.choice([-1.0, 1.0], n_each) * 2.0 ** rng.uniform(-26, -14, n_each))[:, None]
    o = _f64(ext(n_each))
    parts.append(_rays(o, q - o))
    # tangent points of touching neighbours: c + r e_k
    e = np.eye(3)[rng.integers(0, 3, n_each)] * rng.choice([-1.0, 1.0], n_each)[:, None]
    q = c + e * r[:, None]
    o = _f64(ext(n_each))
    d = q - o
    parts.append(_rays(o, d / np.linalg.norm(d, axis=1)[:, None]))
    # origins exactly on box planes (odd integers and halves), any direction and along the axes
    o = rng.uniform(-8, 8, (n_each, 3))
    ax = rng.integers(0, 3, n_each)
    o[np.arange(n_each), ax] = (c + e * r[:, None])[np.arange(n_each), ax]
    d = _unit(rng, n_each)
    al = rng.random(n_each) < 0.3
    d[al] = np.eye(3)[rng.integers(0, 3, int(al.sum()))] * rng.choice([-1.0, 1.0], int(al.sum()))[:, None]
    parts.append(_rays(o, d))
    # the plane origins again, aimed at silhouettes
    o2 = _f64(o)
    u = _unit(rng, n_each)
    w = c - o2
    u = np.cross(w, u)
    u /= np.maximum(np.linalg.norm(u, axis=1), 1e-30)[:, None]
    parts.append(_rays(o2, c + u * (r * (1 + rng.choice([-1.0, 1.0], n_each) * 10.0 ** rng.uniform(-8, -2, n_each)))[:, None] - o2))
    rays = _cat(parts)
    rays = _cat([rays, scale_directions(rng, rays[::8]), poke_directions(rng, rays[3::8])])
    assert len(rays) <= 20_000
    return rays


def test_lattice_rays_through_every_walk(gpu, mirt, oracle):
    """The families' rays at a scene of fp16-exact boxes, touching spheres and
    duplicates, through every closest-hit walk, any-hit and trace_ray, byte
    for byte against the oracle's tree walk and brute force. (Its first run
    found 182 misses with |d| of 1e8 .. 1e19 whose sky colour differed: the
    gradient passes 2^31, where the reference's x86 conversion gives
    0x80000000 and the device's saturated; trace.h int_x86.)"""
    abi = mirt.abi
    s = lattice_scene(mirt)
    bvh = mirt.build_bvh(s)   # reorders s as the reference's build does
    s2 = s.copy()
    gpu.upload(s, bvh)
    rays = lattice_rays(np.random.default_rng(31), s)
    tree = oracle.build(s2)
    assert s2.tobytes() == s.tobytes()
    opts = (abi.OPT_QUAD_BATCH, abi.OPT_ORDERED, abi.OPT_PRUNE, abi.OPT_FAST_SLAB)
    try:
        ref = oracle.intersect(tree, s2, rays)
        brute = oracle.intersect(None, s2, rays, use_bvh=False)
        col = oracle.trace_rays(rays, s2, tree, depth=5, mode=1, seed=3)
        hits = ref["hit"] != 0
        print(f"  lattice: {len(rays)} rays, {100 * hits.mean():.1f}% hit; tree and brute force differ on "
              f"{int((ref['sphere'] != brute['sphere']).sum())}")
        assert 0.10 <= hits.mean() <= 0.90
        _, inv, cnt = np.unique(np.column_stack([s2["center"], s2["radius"]]), axis=0, return_inverse=True,
                                return_counts=True)
        dup = np.flatnonzero(cnt[inv.ravel()] > 1)
        assert len(dup) == 16 and np.isin(ref["sphere"], dup).sum() > 100   # equal t does occur
        walks = [("quad batch", {}), ("per-lane four-wide", {abi.OPT_QUAD_BATCH: 0}),
                 ("DFS", {abi.OPT_ORDERED: 0, abi.OPT_PRUNE: 0}), ("exact slab", {abi.OPT_FAST_SLAB: 0})]
        for name, off in walks:
            for o in opts:
                gpu.set_option(o, off.get(o, 1))
            got = gpu.closest_hit(rays)
            bad = np.flatnonzero((got.view(np.uint8).reshape(len(rays), -1) != ref.view(np.uint8).reshape(len(rays), -1)).any(1))
            assert len(bad) == 0, f"{name}: {len(bad)} rays differ, first {rays[bad[0]]}: {got[bad[0]]} != {ref[bad[0]]}"
            assert (gpu.any_hit(rays, use_bvh=True) == ref["hit"]).all(), name
            if name in ("quad batch", "DFS"):
                assert (gpu.trace_ray(rays, depth=5, seed=3) == col).all(), name
        for o in opts:
            gpu.set_option(o, 1)
        got = gpu.closest_hit(rays, use_bvh=False)
        assert got.tobytes() == brute.tobytes()
        assert (gpu.any_hit(rays, use_bvh=False) == brute["hit"]).all()
    finally:
        for o in opts:
            gpu.set_option(o, 1)
        oracle.free(tree)


def _lattice_cameras(mirt, C):
    C = F32(C)
    cams = {}
    for name, pos in (("inside", (1.0, 1.0, 1.0)),
                      ("on a lattice plane", (3.0, 1.0, 12.0)),
                      ("inside C", (0.5, 1.5, float(np.nextafter(C, F32(0))))),
                      ("beyond C", (0.5, 1.5, float(np.nextafter(C, INF)))),
                      ("inside 4C", (0.5, 1.5, float(np.nextafter(F32(4) * C, F32(0))))),
                      ("beyond 4C", (0.5, 1.5, float(np.nextafter(F32(4) * C, INF))))):
        cam = mirt.default_camera()
        cam.position = mirt.abi.Vec3(*pos)
        cams[name] = cam
    return cams


@pytest.mark.parametrize("far", [False, True])
def test_lattice_frames(gpu, mirt, oracle, far):
    """The bounce kernel's and the packet kernel's margin-free walks are
    reached only through frames: the lattice at depth 5 from cameras inside
    it, exactly on a box plane, and either side of C and 4C, with the origin
    bound in force and (far) without one."""
    s = lattice_scene(mirt, far)
    bvh = mirt.build_bvh(s)
    s2 = s.copy()
    gpu.upload(s, bvh)
    near = lattice_scene(mirt)
    C_near, _ = origin_bound(near, mirt.build_bvh(near).nodes)   # the bound the cameras straddle, in both scenes
    C, _ = origin_bound(s, bvh.nodes)
    assert (C == 0) == far and C_near > 7
    tree = oracle.build(s2)
    try:
        for name, cam in _lattice_cameras(mirt, C_near).items():
            for W, H, seed in ((64, 36, 1), (77, 45, 2)):
                img = gpu.render_frame(cam, W, H, depth=5, seed=seed)
                ref = oracle.render(cam, W, H, s2, tree, depth=5, use_bvh=True, mode=1, seed=seed)
                bad = int((img != ref).any(-1).sum())
                assert bad == 0, f"camera {name} {W}x{H}: {bad} pixels differ"
                assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 50, name
    finally:
        oracle.free(tree)


# ---------------------------------------------------------------- the zero-origin hole

def _unbounded_scene(mirt):
    s = np.zeros(3, mirt.abi.SPHERE)
    s["center"] = [[3, 0, 0], [-3, 0, 0], [7.0e4, 0, 0]]
    s["radius"] = 1
    s["color"] = [[200, 30, 30, 255], [30, 30, 200, 255], [30, 200, 30, 255]]
    return s, mirt.build_bvh(s)


def zero_origin_pairs(rng, n):
    """The edge-grazing family moved so that every origin is an exact zero,
    in all eight sign combinations."""
    rays, boxes = edge_grazing(rng, n)
    o = rays["origin"].astype(np.float64)
    lo, hi = _f64(boxes["min"].astype(np.float64) - o), _f64(boxes["max"].astype(np.float64) - o)
    signs = np.array(list(itertools.product([0.0, -0.0], repeat=3)))[np.arange(n) % 8]
    return _rays(signs, rays["direction"]), _boxes(lo, hi)


def test_zero_origin_takes_the_exact_test_without_a_bound(gpu, mirt, oracle):
    """A scene without an origin bound (o_bound == 0: a sphere beyond the fp16
    range) never had its boxes grown, so every bounce ray must take the exact
    test -- also one whose origin is exactly (+-0, +-0, +-0), which passes
    max|o| <= 0. The margin-free forms must EQUAL hit.c's flag on such a
    scene, on every pair. (Before the rule asked for o_bound > 0, the bounce
    form differed from hit.c on 12,877 of these 220,000 pairs.)"""
    abi = mirt.abi
    s, b = _unbounded_scene(mirt)
    assert origin_bound(s, b.nodes)[0] == 0
    gpu.upload(s, b)
    rng = np.random.default_rng(5)
    rays, boxes = zero_origin_pairs(rng, 200_000)
    assert (rays["origin"] == 0).all() and len(np.unique(np.signbit(rays["origin"]), axis=0)) == 8
    r2, b2 = edge_grazing(rng, 20_000)
    rays, boxes = _cat([rays, r2]), _cat([boxes, b2])
    ref = oracle.aabb_pairs(rays, boxes)
    _assert_both_outcomes("zero origins", ref[:200_000])
    took, decided, near, undecided = classify_slab_fast(rays, boxes)
    print(f"  filter decides within 64 margins {100 * _share(near):.1f}%, undecided {100 * _share(undecided):.1f}%")
    assert _share(near) >= 0.05 and _share(undecided) >= 0.05
    best = np.full(len(rays), INF)
    for form in (abi.BOX_FORM_CONS_BOUNCE, abi.BOX_FORM_CONS_CAMERA):
        got = gpu.box_form_pairs(rays, boxes, best, form)
        bad = np.flatnonzero(got != ref)
        print(f"  form {form}: {len(bad)} of {len(rays)} pairs differ from the oracle")
        assert len(bad) == 0, f"form {form}: {len(bad)} pairs differ, first {rays[bad[0]]} {boxes[bad[0]]}"


def _zero_bounce_scene(mirt, oracle):
    """A camera and a scene (without an origin bound) whose centre-ish pixel's
    ray records t == 8.0f exactly from the position -8 d: the bounce ray then
    starts at fl(o + 8 d) = (0, 0, 0). The sphere radius is searched on the
    CPU until the recorded t is exactly 8."""
    abi = mirt.abi
    W, H, px, py = 64, 36, 29, 15
    cam = mirt.default_camera()
    d = oracle.camera_rays(cam, W, H, rows=[py])[0, px]["direction"].copy()
    pos = (F32(-8) * d).astype(F32)
    cam.position = abi.Vec3(*[float(v) for v in pos])
    ray = oracle.camera_rays(cam, W, H, rows=[py])[0, px:px + 1].copy()
    assert (ray["direction"][0] == d).all() and (ray["origin"][0] == pos).all()
    radii = (1.0 + np.arange(4096) / 4096.0).astype(F32)
    sph = np.zeros(len(radii), abi.SPHERE)
    sph["radius"] = radii
    sph["center"] = d[None, :].astype(np.float64) * radii[:, None].astype(np.float64)
    sph["color"] = [90, 160, 220, 255]
    h = oracle.sphere_pairs(np.repeat(ray, len(radii)), sph)
    ok = np.flatnonzero((h["hit"] != 0) & (h["t"] == F32(8)) & (h["point"] == 0).all(1))
    if len(ok) == 0:
        return None
    rng = np.random.default_rng(9)
    others = sphere_pool(rng, 40)
    others["radius"] = rng.uniform(0.5, 2.0, 40)
    ang = rng.uniform(0, 2 * np.pi, 40)   # a ring round the camera ray, in view and in the bounce's way
    rad = rng.uniform(4, 9, 40)
    others["center"] = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-4, 5, 40)], 1)
    far = np.zeros(1, abi.SPHERE)
    far["center"], far["radius"], far["color"] = [7.0e4, 0, 0], 1, [9, 9, 9, 255]
    return cam, _cat([sph[ok[:1]], others, far]), (W, H, px, py), ray


def test_zero_origin_bounce_frame(gpu, mirt, oracle):
    """A frame that delivers an exact-zero bounce origin to the bounce kernel
    on a scene without an origin bound."""
    found = _zero_bounce_scene(mirt, oracle)
    assert found is not None, "no radius with a recorded t of exactly 8 among 4096 candidates"
    cam, s, (W, H, px, py), ray = found
    bvh = mirt.build_bvh(s)
    s2 = s.copy()
    assert origin_bound(s, bvh.nodes)[0] == 0
    gpu.upload(s, bvh)
    tree = oracle.build(s2)
    try:
        h = oracle.intersect(tree, s2, ray)
        assert h["hit"][0] == 1 and h["t"][0] == F32(8) and (h["point"][0] == 0).all()   # the bounce starts at 0
        for depth in (5, 2):
            img = gpu.render_frame(cam, W, H, depth=depth, seed=1)
            ref = oracle.render(cam, W, H, s2, tree, depth=depth, use_bvh=True, mode=1, seed=1)
            assert int((img != ref).any(-1).sum()) == 0
        assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 50
    finally:
        oracle.free(tree)

"""The reprojection with a motion (csrc/reproject.h, mirt.h mirt_sphere_motion)
restated in numpy on top of reproject_cases, one float32 operation per
operation of the definition, and the cases its tests run (no GPU).

A motion: geo (n, 4) float32 {centre, radius}, the scene the current frame's
sphere plane indexes; geo_prev (m, 4), the previous frame's scene; prev_index
(n,) int32 or None (the identity): entry s is the index in geo_prev of the
sphere that is now s. Steps 2, 3 and 8 of reproject_cases become:

  2  X = p + d * t.
  2a !(0 <= s < n): no history. sp = prev_index[s] (or s);
     !(0 <= sp < m): no history.
  2b g = geo[s], gp = geo_prev[sp]. All four floats equal (a NaN is unequal):
     Xp = X. Otherwise k = gp.r / g.r; o = X - g.c; o = o * k; Xp = gp.c + o.
  3  e = Xp - p_prev; then as before.
  8  a tap needs sphere_prev[q] == sp (not s).

Real cases, on reproject_cases' 44 x 26 frame over scene(1000): the previous
frame is camera A's frame of the scene as built; the current frame is the
oracle's frame and planes of the MOVED scene (the same spheres in the same
order over the refit tree) from camera A ("_A") or one MOVE_SPEED step to the
right ("_right"). "still": nothing moved. "diffused": test_update_device.moved
with sigma 0.5 (every centre, and every radius by 0.5 .. 1.5). "shifted": every
tenth sphere moved rigidly by SHIFT, several pixels. "radii": radii scaled by
0.5 .. 1.5 alone. "permuted": the diffused scene with the previous scene's
order permuted, prev_index the inverse.

Synthetic cases, on reproject_cases' two cameras over a surface at distance 16
with spheres placed around it: 5 x 3, 1 x 1, 7 x 1 and 1 x 7 images; 70 x 5,
which crosses the kernel's 64 x 4 tile in both directions; "range_9_3": s ==
num_spheres, s huge and negative beyond -1, prev_index of -1 and of num_prev;
"radius_9_3": radii 0 and NaN, current and previous; "counts_5_3": num_prev !=
num_spheres.
"""
import ctypes as C
import functools

import numpy as np

import lens_frame_cases as lc
import reproject_cases as rc
import test_planes_cases as cases

mirt = rc.mirt
abi = rc.abi
F32 = np.float32
W, H, N = rc.W, rc.H, rc.N
PARAMS = rc.PARAMS
SKY, FIRST, BEHIND, NO_TAP, REUSED = rc.SKY, rc.FIRST, rc.BEHIND, rc.NO_TAP, rc.REUSED
NO_SPHERE = 5   # step 2a: s or prev_index[s] out of range
SIGMA = 0.5
# units; a pixel of case A is about 1.6 units at the scene's depth: 3 pixels along x, 1 along y. Chosen on the CPU so
# that the plain reprojection reuses less than half of the shifted spheres' pixels (it reuses 3 of 61)
SHIFT = np.array([4.8, 1.6, 0.0], F32)
SHIFT_EVERY = 10

same_bytes = rc.same_bytes


def geo_of(spheres):
    """(n, 4) float32 {centre, radius}: MIRT_LAYOUT_GEO's first n elements."""
    out = np.zeros((len(spheres), 4), F32)
    out[:, :3], out[:, 3] = spheres["center"], spheres["radius"]
    return out


def moved_point(c):
    """Steps 2, 2a, 2b for every pixel: (Xp (H, W, 3) float32, ok (H, W), sp (H, W) int64)."""
    w, h = c["width"], c["height"]
    cur = rc.cam_consts(c["cam"], w, h)
    _, d = lc.pinhole(c["cam"], None, w, h)
    geo, geo_prev, idx = c["geo"], c["geo_prev"], c["prev_index"]
    s = c["sphere"].astype(np.int64)
    with np.errstate(all="ignore"):
        X = cur["p"] + d * c["t"][..., None]
        inside = (s >= 0) & (s < len(geo))
        si = np.where(inside, s, 0)
        sp = idx[si].astype(np.int64) if idx is not None else si
        ok = inside & (sp >= 0) & (sp < len(geo_prev))
        g, gp = geo[si], geo_prev[np.where(ok, sp, 0)]
        equal = (gp == g).all(axis=-1)
        k = gp[..., 3] / g[..., 3]
        o = X - g[..., :3]
        o = o * k[..., None]
        Xm = gp[..., :3] + o
        Xp = np.where(equal[..., None], X, Xm)
    assert Xp.dtype == F32
    return Xp, ok, sp


def project(c):
    """Steps 2 - 5 with the motion: (xf, yf, zf, l, ok, sp)."""
    w, h = c["width"], c["height"]
    prv = rc.cam_consts(c["cam_prev"], w, h)
    Xp, ok, sp = moved_point(c)
    with np.errstate(all="ignore"):
        e = Xp - prv["p"]
        assert e.dtype == F32
        zf = rc.dot3(e, prv["fwd"])
        a = rc.dot3(e, prv["right"]) / zf
        b = rc.dot3(e, prv["up"]) / zf
        u = a / prv["sw"]
        v = b / prv["sh"]
        xf = (u / prv["aspect"] + F32(0.5)) * prv["wf"]
        yf = (F32(0.5) - v) * prv["hf"]
        l = np.sqrt(rc.dot3(e, e))
    assert xf.dtype == F32 and yf.dtype == F32 and l.dtype == F32
    return xf, yf, zf, l, ok, sp


def restate(c, params):
    """reproject_cases.restate with the motion of c: (hist_out, out, out_rgb, info)."""
    max_history, taps, tol = params
    w, h = c["width"], c["height"]
    col = c["rgba"][..., :3].astype(F32) / F32(255.0)
    s = c["sphere"]
    hit = s >= 0
    xf, yf, zf, l, ok, sp = project(c)
    nvalid = np.zeros((h, w), np.int32)
    with np.errstate(all="ignore"):
        front = zf > F32(0.0)
        bound = F32(tol) * l
        sw = np.zeros((h, w), F32)
        sc = np.zeros((h, w, 3), F32)
        nmin = np.full((h, w), 1 << 40, np.int64)
        for tx, ty, wt in rc.taps_of(xf, yf, taps):
            inside = (tx >= F32(0.0)) & (tx < F32(w)) & (ty >= F32(0.0)) & (ty < F32(h))
            qx = np.where(inside, tx, F32(0.0)).astype(np.int64)
            qy = np.where(inside, ty, F32(0.0)).astype(np.int64)
            hq = c["hist"][qy, qx]
            valid = (hit & ok & front & inside & (wt > F32(0.0)) & (c["sphere_prev"][qy, qx] == sp) & (hq["n"] >= 1) &
                     (np.abs(l - c["t_prev"][qy, qx]) <= bound))
            sw = np.where(valid, sw + wt, sw)
            for ch, f in enumerate("rgb"):
                sc[..., ch] = np.where(valid, sc[..., ch] + hq[f] * wt, sc[..., ch])
            nmin = np.where(valid, np.minimum(nmin, hq["n"].astype(np.int64)), nmin)
            nvalid += valid
        took = nvalid > 0
        m = sc / sw[..., None]
        nn = np.minimum(nmin + 1, max_history)
        upd = m + (col - m) / nn.astype(F32)[..., None]
        assert upd.dtype == F32
    mean = np.where(took[..., None], upd, col)
    n_new = np.where(took, nn, 1).astype(np.int32)
    why = np.where(~hit, SKY, np.where(~ok, NO_SPHERE, np.where(~front, BEHIND, np.where(took, REUSED, NO_TAP))))
    hist = np.zeros((h, w), abi.HISTORY)
    hist["r"], hist["g"], hist["b"], hist["n"] = mean[..., 0], mean[..., 1], mean[..., 2], n_new
    return hist, rc.display(mean), np.ascontiguousarray(mean), dict(why=why, valid=nvalid)


# ---- moved scenes, from the oracle

def moved(s, sigma, seed):
    """test_update_device.moved"""
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(F32)
    out["radius"] *= r.uniform(0.5, 1.5, len(s)).astype(F32)
    return out


def diffused(s, sigma, seed):
    """The centres' part of `moved` alone."""
    out = s.copy()
    out["center"] += np.random.default_rng(seed).normal(0.0, sigma, (len(s), 3)).astype(F32)
    return out


def shifted_ids():
    return np.arange(0, N, SHIFT_EVERY)


@functools.lru_cache(maxsize=None)
def spheres_of(kind):
    """The scene `kind` holds: scene(N)'s spheres, in their order, moved. "walkK": K diffusion steps."""
    base = cases.scene(N)[0]
    if kind == "still":
        out = base.copy()
    elif kind in ("diffused", "permuted"):
        out = moved(base, SIGMA, 11)
    elif kind == "shifted":
        out = base.copy()
        out["center"][shifted_ids()] += SHIFT
    elif kind == "radii":
        out = base.copy()
        out["radius"] *= np.random.default_rng(12).uniform(0.5, 1.5, N).astype(F32)
    elif kind.startswith("walk"):
        k = int(kind[4:])
        out = base.copy() if k == 0 else diffused(spheres_of(f"walk{k - 1}"), SIGMA, 100 + k)
    else:
        raise KeyError(kind)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tree_of(kind):
    """The oracle's tree handle of scene(N)'s tree refit to spheres_of(kind) (kept for the session)."""
    nodes = mirt.refit_bvh(cases.scene(N)[2], spheres_of(kind), N).nodes
    return cases._oracle().tree_from_flat(nodes)


@functools.lru_cache(maxsize=None)
def oracle_frame(kind, cam, sample):
    out = cases._oracle().render(rc.camera(cam), W, H, spheres_of(kind), tree_of(kind), depth=5, seed=1, sample=sample)
    out = np.ascontiguousarray(out.reshape(H, W, 4))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _rays(cam):
    return cases._oracle().camera_rays(rc.camera(cam), W, H).reshape(-1)


@functools.lru_cache(maxsize=None)
def oracle_planes(kind, cam):
    pl = cases.planes_of(cases._oracle().intersect(tree_of(kind), spheres_of(kind), _rays(cam)), (H, W))
    for a in pl.values():
        a.setflags(write=False)
    return pl


def _case(base, geo, geo_prev, prev_index, **over):
    c = dict(base)
    c.update(over)
    c.update(geo=np.ascontiguousarray(geo, F32), geo_prev=np.ascontiguousarray(geo_prev, F32),
             prev_index=None if prev_index is None else np.ascontiguousarray(prev_index, np.int32), params=PARAMS)
    for k in ("sphere", "sphere_prev"):
        c[k] = np.ascontiguousarray(c[k], np.int32)
    return rc._frozen(c)


def _real(kind, cam):
    hist, t_prev, sphere_prev = rc._previous("A")
    pl = oracle_planes(kind, cam)
    base = rc._case(W, H, rc.camera(cam), rc.camera("A"), oracle_frame(kind, cam, 1), pl["t"], pl["sphere"], hist,
                    t_prev, sphere_prev)
    geo, geo_prev, idx = geo_of(spheres_of(kind)), geo_of(cases.scene(N)[0]), None
    if kind == "permuted":
        order = np.random.default_rng(13).permutation(N)     # the previous scene held sphere order[j] at j
        idx = np.empty(N, np.int32)
        idx[order] = np.arange(N, dtype=np.int32)
        geo_prev = geo_prev[order]
        sphere_prev = np.where(sphere_prev >= 0, idx[np.maximum(sphere_prev, 0)], sphere_prev)
    return _case(base, geo, geo_prev, idx, sphere_prev=sphere_prev)


def _centre_point(c):
    """The point the middle pixel of a synthetic case sees."""
    w, h = c["width"], c["height"]
    _, d = lc.pinhole(c["cam"], None, w, h)
    return rc.cam_consts(c["cam"], w, h)["p"] + d[h // 2, w // 2] * c["t"][h // 2, w // 2]


def _synthetic(w, h, seed, kind="syn", fov=1.0):
    """reproject_cases' synthetic frame with spheres around its surface, each moved by about a pixel. "rigid": the
    radii stay (on a wide image the points are far from the centres, and a rescaling would carry them out of view).
    fov: of both cameras, narrow: a pixel is then a small part of the t tolerance (0.25 at distance 16), so that
    motions of a pixel change the taps and not the distance test (a quarter of the previous distances are a tenth
    off, as in reproject_cases)."""
    base = dict(rc._synthetic(w, h, seed))
    # a pixel at the surface's distance, in units, along y and along x (the frame's horizontal extent grows with the
    # aspect squared: a wide image needs a narrow field, at 60 degrees by 14 its outer rays graze the image plane)
    py = 2.0 * 16.0 * np.tan(np.radians(fov) / 2.0) / h
    px_x = py * h * (w / h) ** 2 / w
    px = F32(min(px_x, py))
    # the previous camera stands a part of a pixel away along both axes
    base["cam"] = rc._syn_camera(fov=fov)
    prev = rc.copy_camera(base["cam"])
    p = rc._vec(prev.position) + rc._vec(prev.right) * F32(0.4 * px_x) + rc._vec(prev.up) * F32(0.3 * py)
    prev.position = abi.Vec3(*[float(v) for v in p])
    base["cam_prev"] = prev
    rng = np.random.default_rng(seed + 1000)
    n = 4
    centre = _centre_point(base)
    geo = np.zeros((n, 4), F32)
    geo[:, :3] = centre + rng.uniform(-0.65, 0.65, (n, 3)).astype(F32) * px
    geo[:, 3] = rng.uniform(0.5, 0.8, n).astype(F32) * px
    geo_prev = geo.copy()
    geo_prev[:, :3] += rng.normal(0.0, 0.5, (n, 3)).astype(F32) * px
    if kind != "rigid":
        geo_prev[:, 3] *= rng.uniform(0.8, 1.2, n).astype(F32)
    geo_prev[0] = geo[0]   # one sphere that did not move
    # both frames see the spheres in square patches (the motion is about a pixel: most taps land on the same sphere),
    # a tenth of the current pixels see the sky
    yy, xx = np.mgrid[0:h, 0:w]
    side = 2 if w <= 16 else 8
    patch = ((xx // side + yy // side) % n).astype(np.int32)
    sphere = np.where(rng.random((h, w)) < 0.1, -1, patch).astype(np.int32)
    sphere_prev = patch
    idx = None
    if kind == "range":
        idx = np.array([0, -1, n, 1], np.int32)
        sphere.reshape(-1)[:4] = [n, 2 ** 31 - 1, -5, -(2 ** 31)]
        sphere_prev = np.array([0, 0, 0, 1], np.int32)[patch]
    elif kind == "radius":
        geo[1, 3] = 0.0
        geo[2, 3] = np.nan
        geo_prev[3, 3] = 0.0
        geo_prev = np.concatenate([geo_prev, geo_prev[:1]])
        geo_prev[4, 3] = np.nan
        idx = np.array([4, 1, 2, 3], np.int32)
        sphere_prev = idx[patch]
    elif kind == "counts":
        geo = geo[:3]
        geo_prev = np.concatenate([geo_prev, geo_prev[:1] + F32(1.0)])
        idx = np.array([4, 0, 2], np.int32)
        # (mostly sphere 0, which was entry 4 and has hardly moved: some taps are valid)
        sphere = rng.choice(np.array([-1, 0, 0, 0, 1, 2], np.int32), (h, w))
        sphere_prev = rng.choice(np.array([4, 4, 4, 0, 2], np.int32), (h, w))
    elif kind == "index":
        idx = np.array([2, 0, 3, 1], np.int32)
        geo_prev = geo_prev[np.argsort(idx)]
        geo_prev[2] = geo[0]
        sphere_prev = idx[patch]
    return _case(base, geo, geo_prev, idx, sphere=sphere, sphere_prev=sphere_prev)


KINDS = ["still", "diffused", "shifted", "radii", "permuted"]
REAL = [f"{k}_{cam}" for k in KINDS for cam in ("A", "right")]
SYNTHETIC = {
    "m_5_3": lambda: _synthetic(5, 3, 53), "m_1_1": lambda: _synthetic(1, 1, 11), "m_7_1": lambda: _synthetic(7, 1, 71, fov=0.5),
    "m_1_7": lambda: _synthetic(1, 7, 17), "m_70_5": lambda: _synthetic(70, 5, 705, "rigid", fov=0.3),
    "index_5_3": lambda: _synthetic(5, 3, 57, "index"), "range_9_3": lambda: _synthetic(9, 3, 58, "range"),
    "radius_9_3": lambda: _synthetic(9, 3, 59, "radius"), "counts_5_3": lambda: _synthetic(5, 3, 60, "counts"),
}
CASES = REAL + list(SYNTHETIC)


@functools.lru_cache(maxsize=None)
def case(name):
    """reproject_cases.case's fields plus "geo", "geo_prev" and "prev_index" (None: the identity)."""
    if name in SYNTHETIC:
        return SYNTHETIC[name]()
    kind, cam = name.rsplit("_", 1)
    return _real(kind, cam)


@functools.lru_cache(maxsize=None)
def expected(name, params):
    hist, out, rgb, info = restate(case(name), params)
    for a in (hist, out, rgb, info["why"], info["valid"]):
        a.setflags(write=False)
    return hist, out, rgb, info


def runs():
    return [(name, p) for name in CASES for p in PARAMS]


def motion_struct(c):
    """abi.SphereMotion of a case's (host) arrays; the arrays stay the case's."""
    idx = c["prev_index"]
    return abi.SphereMotion(c["geo"].ctypes.data, c["geo_prev"].ctypes.data, idx.ctypes.data if idx is not None else None,
                            len(c["geo"]), len(c["geo_prev"]))


def host(lib, c, params, want_out=True, want_rgb=True, motion=True):
    """mirt_reproject_motion_host on a case (motion=False: mirt_reproject_host on its frame):
    (hist_out, out, out_rgb), None for an output not asked for."""
    if not motion:
        return rc.host(lib, c, params, want_out, want_rgb)
    h_, w_ = c["height"], c["width"]
    hist = np.zeros((h_, w_), abi.HISTORY)
    out = np.zeros((h_, w_, 4), np.uint8) if want_out else None
    rgb = np.zeros((h_, w_, 3), F32) if want_rgb else None
    p, mo = rc.params_struct(params), motion_struct(c)
    r = lib.mirt_reproject_motion_host(w_, h_, rc._ref(c["cam"]), rc._ref(c["cam_prev"]), rc._p(c["rgba"]),
                                       rc._p(c["t"]), rc._p(c["sphere"]), rc._p(c["hist"]), rc._p(c["t_prev"]),
                                       rc._p(c["sphere_prev"]), C.byref(p), rc._p(hist), rc._p(out), rc._p(rgb),
                                       C.byref(mo))
    assert r == 0, lib.mirt_last_error().decode()
    return hist, out, rgb


def host_step(lib, cam, rgba, t, sphere, prev, params, motion=None):
    """reproject_cases.host_step; motion: None or (geo, geo_prev, prev_index) for a frame with a previous one."""
    if motion is None or prev is None:
        return rc.host_step(lib, cam, rgba, t, sphere, prev, params)
    cam_prev, hist, t_prev, sphere_prev = prev
    h_, w_ = sphere.shape
    geo, geo_prev, idx = motion
    c = dict(width=w_, height=h_, cam=cam, cam_prev=cam_prev, rgba=np.ascontiguousarray(rgba),
             t=np.ascontiguousarray(t, F32), sphere=np.ascontiguousarray(sphere, np.int32), hist=hist, t_prev=t_prev,
             sphere_prev=sphere_prev, geo=np.ascontiguousarray(geo, F32), geo_prev=np.ascontiguousarray(geo_prev, F32),
             prev_index=None if idx is None else np.ascontiguousarray(idx, np.int32))
    hist_out, out, _ = host(lib, c, params, want_rgb=False)
    return hist_out, out

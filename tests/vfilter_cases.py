"""The moments reprojection and the variance-guided filter (csrc/reproject.h
MOMENTS, csrc/vfilter.h, mirt.h mirt_denoise_var_params) restated in numpy, one
float32 operation per operation of the definition and in its order, and the
cases their tests run, from the oracle and a seeded generator alone (no GPU).

lum(c): L = 0.2126 c0; L = L + 0.7152 c1; L = L + 0.0722 c2.

MOMENTS, on top of reproject_cases / reproject_motion_cases: q2 = lum(c)^2;
over the valid taps in order s2 = s2 + m2_prev[q] * w; M2 = s2 / sw;
m2_out = M2 + (q2 - M2) / n_new; no history: m2_out = q2. The cases are every
case of reproject_cases.CASES and reproject_motion_cases.CASES with a seeded
m2_prev: lum(record)^2 where the record's n is 1 (and wherever n is not a count
or the square is not finite), up to one and a half times that elsewhere.

FILTER: V1 n >= min_history: var = fmax(m2 - Lp Lp, 0) / n; V2 else over the
7 x 7 window (dy outermost, dx innermost, centre included) the taps inside the
image on the pixel's sphere give k, S1, S2; mu = S1 / k; var = fmax(S2 / k -
mu mu, 0). V3 pass i has spacing 2^i and denoise_cases' taps, B, same-sphere
rule, normal weight and centre; with sigma_lum > 0 off the centre also
dl = Lp - Lq; g = dl dl; den = sl2 var_p; den = den + 1e-6;
w = w * (1 / (1 + g / den)); sw = sw + w; sc = sc + c_q w; sv = sv + var_q (w w);
colour sc / sw, variance sv / (sw sw).

Filter cases (FILTER_CASES): "loop" -- the records and m2 after the five frames
path0 .. path4 over reproject_cases' 44 x 26 case (the oracle's colours and
planes, the restated moments reprojection at its defaults), with the last
camera's normals; "syn_W_H" at denoise_cases.SIZES and "miss", "one", "checker"
at 33 x 65 -- denoise_cases' spheres and normals, random colours in [0, 1), n in
1 .. 8 (so that both variance branches are taken at min_history 4), m2 between
lum^2 and twice it; "n_*": n of 0, negative and 2^31 - 1; "m2_*": m2 of NaN,
+-inf and below lum^2; "nan_*": NaN colours.

Non-finite data gives unspecified VALUES (mirt.h): where the restatement holds
a NaN the forms must hold one too, whatever its sign and payload
(same_values); every other byte is compared.
"""
import ctypes as C
import functools
import itertools

import numpy as np

import denoise_cases as dc
import reproject_cases as rc
import reproject_motion_cases as mc

abi = rc.abi
F32 = np.float32
B = dc.B
W, H = rc.W, rc.H
same_bytes = dc.same_bytes


def display(rgb):
    """denoise_display: (u8)(int)fminf(c * 255, 255) per channel (255 for a NaN, 0 below int's range), alpha 255."""
    with np.errstate(all="ignore"):
        v = np.fmin(rgb * F32(255.0), F32(255.0))
        v = np.where(v >= F32(-2147483648.0), v, F32(0.0)).astype(np.int32)
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = (v & 0xFF).astype(np.uint8)
    return out


def lum(c):
    L = F32(0.2126) * c[..., 0]
    L = L + F32(0.7152) * c[..., 1]
    return L + F32(0.0722) * c[..., 2]


def same_values(got, want, what):
    """same_bytes, but a NaN in `want` only asks for a NaN in `got`."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (what, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: NaNs at other pixels"
    same_bytes(np.where(nan, F32(0), got), np.where(nan, F32(0), want), what)


def rgb_of(hist):
    return np.stack([hist["r"], hist["g"], hist["b"]], axis=-1)


# ---- moments

def moment_case(name):
    """(the reprojection case, whether it has a motion)"""
    if name.startswith("motion:"):
        return mc.case(name[7:]), True
    return rc.case(name), False


MOMENT_CASES = list(rc.CASES) + ["motion:" + n for n in mc.CASES]


@functools.lru_cache(maxsize=None)
def m2_prev_of(name):
    c, _ = moment_case(name)
    if c["hist"] is None:
        return None
    rng = np.random.default_rng(len(name) * 131 + c["width"])
    with np.errstate(all="ignore"):
        L = lum(rgb_of(c["hist"]))
        sq = L * L
        more = sq * (F32(1.0) + rng.random(sq.shape).astype(F32) * F32(0.5))
        out = np.where((c["hist"]["n"] > 1) & np.isfinite(more), more, sq).astype(F32)
    out.setflags(write=False)
    return out


def restate_moments(c, params, m2_prev, motion):
    """(hist_out, out, out_rgb, m2_out) of the definition, in numpy."""
    hist, out, rgb, _ = (mc.restate if motion else rc.restate)(c, params)
    max_history, taps, tol = params
    w, h = c["width"], c["height"]
    col = c["rgba"][..., :3].astype(F32) / F32(255.0)
    Lc = lum(col)
    q2 = Lc * Lc
    assert q2.dtype == F32
    if c["cam_prev"] is None:
        return hist, out, rgb, q2
    s = c["sphere"]
    hit = s >= 0
    if motion:
        xf, yf, zf, l, ok, sp = mc.project(c)
    else:
        xf, yf, zf, l = rc.project(c)
        ok, sp = np.ones((h, w), bool), s
    with np.errstate(all="ignore"):
        front = zf > F32(0.0)
        bound = F32(tol) * l
        sw = np.zeros((h, w), F32)
        s2 = np.zeros((h, w), F32)
        nmin = np.full((h, w), 1 << 40, np.int64)
        took = np.zeros((h, w), bool)
        for tx, ty, wt in rc.taps_of(xf, yf, taps):
            inside = (tx >= F32(0.0)) & (tx < F32(w)) & (ty >= F32(0.0)) & (ty < F32(h))
            qx = np.where(inside, tx, F32(0.0)).astype(np.int64)
            qy = np.where(inside, ty, F32(0.0)).astype(np.int64)
            hq = c["hist"][qy, qx]
            valid = (hit & ok & front & inside & (wt > F32(0.0)) & (c["sphere_prev"][qy, qx] == sp) & (hq["n"] >= 1) &
                     (np.abs(l - c["t_prev"][qy, qx]) <= bound))
            sw = np.where(valid, sw + wt, sw)
            s2 = np.where(valid, s2 + m2_prev[qy, qx] * wt, s2)
            nmin = np.where(valid, np.minimum(nmin, hq["n"].astype(np.int64)), nmin)
            took |= valid
        M2 = s2 / sw
        nn = np.minimum(nmin + 1, max_history).astype(F32)
        upd = M2 + (q2 - M2) / nn
        assert upd.dtype == F32
    assert (np.where(took, np.minimum(nmin + 1, max_history), 1) == hist["n"]).all()   # the same taps as the records'
    return hist, out, rgb, np.where(took, upd, q2)


@functools.lru_cache(maxsize=None)
def expected_moments(name, params):
    c, motion = moment_case(name)
    got = restate_moments(c, params, m2_prev_of(name), motion)
    for a in got:
        a.setflags(write=False)
    return got


def moment_runs():
    return [(name, p) for name in MOMENT_CASES for p in moment_case(name)[0]["params"]]


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host_moments(lib, c, params, m2_prev, motion, want_out=True, want_rgb=True):
    """mirt_reproject_moments_host: (hist_out, out, out_rgb, m2_out), None for an output not asked for."""
    h_, w_ = c["height"], c["width"]
    hist = np.zeros((h_, w_), abi.HISTORY)
    out = np.zeros((h_, w_, 4), np.uint8) if want_out else None
    rgb = np.zeros((h_, w_, 3), F32) if want_rgb else None
    m2 = np.zeros((h_, w_), F32)
    p = rc.params_struct(params)
    mo = mc.motion_struct(c) if motion else None
    r = lib.mirt_reproject_moments_host(w_, h_, rc._ref(c["cam"]), rc._ref(c["cam_prev"]), _p(c["rgba"]), _p(c["t"]),
                                        _p(c["sphere"]), _p(c["hist"]), _p(c["t_prev"]), _p(c["sphere_prev"]),
                                        C.byref(p), _p(hist), _p(out), _p(rgb), rc._ref(mo), _p(m2_prev), _p(m2))
    assert r == 0, lib.mirt_last_error().decode()
    return hist, out, rgb, m2


def host_moments_step(lib, cam, rgba, t, sphere, prev, params, motion=None):
    """One frame of the loop on the host: prev is None or (cam_prev, hist, t_prev, sphere_prev, m2_prev); motion None
    or (geo, geo_prev, prev_index). Returns (hist_out, out, m2_out)."""
    cam_prev, hist, t_prev, sphere_prev, m2_prev = prev if prev is not None else (None,) * 5
    h_, w_ = sphere.shape
    c = dict(width=w_, height=h_, cam=cam, cam_prev=cam_prev, rgba=np.ascontiguousarray(rgba),
             t=np.ascontiguousarray(t, F32), sphere=np.ascontiguousarray(sphere, np.int32), hist=hist, t_prev=t_prev,
             sphere_prev=sphere_prev)
    if motion is not None and prev is not None:
        geo, geo_prev, idx = motion
        c.update(geo=np.ascontiguousarray(geo, F32), geo_prev=np.ascontiguousarray(geo_prev, F32),
                 prev_index=None if idx is None else np.ascontiguousarray(idx, np.int32))
    hist_out, out, _, m2 = host_moments(lib, c, params, m2_prev, motion is not None and prev is not None,
                                        want_rgb=False)
    return hist_out, out, m2


# ---- the filter

# (passes, normal_sharpness, sigma_lum, min_history, with the normal plane)
PARAMS = list(itertools.product((1, 2, 3, 4, 5), (3,), (0.0, 0.5, 4.0), (4,), (True, False))) + \
    [(3, 0, 4.0, 1, True), (3, 7, 0.5, 65536, True), (2, 3, 4.0, 1, False), (2, 0, 0.5, 65536, False),
     (5, 7, 0.0, 1, True), (1, 0, 0.0, 65536, False)]
DEFAULT = (3, 3, 4.0, 4, True)
SIGMAS = (1.0, 2.0, 4.0, 8.0)   # mirt_denoise_var_params_default takes the best of these (test_vfilter_host)
PATH = [f"path{k}" for k in range(5)]


def variance(hist, m2, sphere, min_history):
    """V1, V2: (H, W) float32."""
    h_, w_ = sphere.shape
    L = lum(rgb_of(hist))
    n = hist["n"]
    ys, xs = np.arange(h_), np.arange(w_)
    with np.errstate(all="ignore"):
        vt = np.fmax(m2 - L * L, F32(0.0))
        temporal = vt / n.astype(F32)
        k = np.zeros((h_, w_), F32)
        S1 = np.zeros((h_, w_), F32)
        S2 = np.zeros((h_, w_), F32)
        for dy in range(-3, 4):
            qy = ys + dy
            in_y = (qy >= 0) & (qy < h_)
            qy = np.clip(qy, 0, h_ - 1)
            for dx in range(-3, 4):
                qx = xs + dx
                in_x = (qx >= 0) & (qx < w_)
                qx = np.clip(qx, 0, w_ - 1)
                q = np.ix_(qy, qx)
                take = in_y[:, None] & in_x[None, :] & (sphere[q] == sphere)
                Lq = L[q]
                k = np.where(take, k + F32(1.0), k)
                S1 = np.where(take, S1 + Lq, S1)
                S2 = np.where(take, S2 + Lq * Lq, S2)
        mu = S1 / k
        spatial = np.fmax(S2 / k - mu * mu, F32(0.0))
        out = np.where(n >= min_history, temporal, spatial)
    assert out.dtype == F32
    return out


def restate(c, passes, k, sigma, min_history, with_normal):
    """(out (H, W, 4) u8, out_rgb (H, W, 3) f32, var_out (H, W) f32) of the definition, in numpy."""
    w_, h_ = c["width"], c["height"]
    sphere = c["sphere"]
    normal = c["normal"] if with_normal else None
    col = np.ascontiguousarray(rgb_of(c["hist"]))
    var0 = variance(c["hist"], c["m2"], sphere, min_history)
    var = var0
    sl2 = F32(sigma) * F32(sigma) if sigma > 0 else None
    ys, xs = np.arange(h_), np.arange(w_)
    use_n = sphere >= 0
    with np.errstate(all="ignore"):
        for i in range(passes):
            s = 1 << i
            sw = np.zeros((h_, w_), F32)
            sc = np.zeros((h_, w_, 3), F32)
            sv = np.zeros((h_, w_), F32)
            if sl2 is not None:
                L = lum(col)
                den = sl2 * var
                den = den + F32(1e-6)
            for dy in range(-2, 3):
                qy = ys + dy * s
                in_y = (qy >= 0) & (qy < h_)
                qy = np.clip(qy, 0, h_ - 1)
                for dx in range(-2, 3):
                    qx = xs + dx * s
                    in_x = (qx >= 0) & (qx < w_)
                    qx = np.clip(qx, 0, w_ - 1)
                    q = np.ix_(qy, qx)
                    take = in_y[:, None] & in_x[None, :] & (sphere[q] == sphere)
                    cq = col[q]
                    wt = np.full((h_, w_), B[dy + 2] * B[dx + 2], F32)
                    if dx or dy:
                        if normal is not None:
                            nq = normal[q]
                            d = normal[..., 0] * nq[..., 0]
                            d = d + normal[..., 1] * nq[..., 1]
                            d = d + normal[..., 2] * nq[..., 2]
                            m = np.fmax(d, F32(0.0))
                            for _ in range(k):
                                m = m * m
                            wt = np.where(use_n, wt * m, wt)
                        if sl2 is not None:
                            dl = L - L[q]
                            g = dl * dl
                            wt = wt * (F32(1.0) / (F32(1.0) + g / den))
                    assert wt.dtype == F32
                    sw = np.where(take, sw + wt, sw)
                    sc = np.where(take[..., None], sc + cq * wt[..., None], sc)
                    sv = np.where(take, sv + var[q] * (wt * wt), sv)
            col = sc / sw[..., None]
            var = sv / (sw * sw)
            assert col.dtype == F32 and var.dtype == F32
    return display(col), col, var0


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def loop_steps(path=tuple(PATH), params=rc.DEFAULT):
    """The restated moments loop along `path` over reproject_cases' scene: [(hist, m2)] after each frame."""
    prev, m2_prev, steps = None, None, []
    for k, name in enumerate(path):
        pl = rc.oracle_planes(name)
        c = dict(width=W, height=H, cam=rc.camera(name), cam_prev=None, rgba=rc.oracle_frame(name, k), t=pl["t"],
                 sphere=pl["sphere"], hist=None, t_prev=None, sphere_prev=None)
        if prev is not None:
            c.update(cam_prev=prev[0], hist=prev[1], t_prev=prev[2], sphere_prev=prev[3])
        hist, _, _, m2 = restate_moments(c, params, m2_prev, False)
        prev, m2_prev = (rc.camera(name), hist, pl["t"], pl["sphere"]), m2
        hist.setflags(write=False)
        m2.setflags(write=False)
        steps.append((hist, m2))
    return steps


def _synthetic(width, height, pattern, kind):
    base = dc.case(f"{pattern}_{width}_{height}")
    rng = np.random.default_rng(7000 * width + height + len(kind))
    shape = (height, width)
    rgb = rng.random(shape + (3,)).astype(F32)
    n = rng.integers(1, 9, shape).astype(np.int32)
    L = lum(rgb)
    m2 = (L * L * (F32(1.0) + rng.random(shape).astype(F32))).astype(F32)
    flat = np.arange(width * height).reshape(shape)
    if kind == "n":     # hostile counts: nothing, negative, and the largest
        n = np.choose(flat % 5, [n, 0, -1, -(2 ** 31), 2 ** 31 - 1]).astype(np.int32)
    elif kind == "m2":  # hostile moments: NaN, both infinities, below lum^2 and negative
        m2 = np.choose(flat % 6, [m2, F32(np.nan), F32(np.inf), F32(-np.inf), L * L * F32(0.5), F32(-1.0)]).astype(F32)
    elif kind == "nan":
        rgb[(flat % 7 == 3)] = np.nan
        rgb[..., 1][flat % 11 == 5] = np.nan
    return _frozen(dict(width=width, height=height, hist=rc.records(rgb, n), m2=m2, sphere=base["sphere"],
                        normal=base["normal"]))


HOSTILE = ["n_5_3", "n_33_65", "m2_5_3", "m2_33_65", "nan_5_3", "nan_33_65"]
FILTER_CASES = ["loop"] + [f"syn_{w}_{h}" for w, h in dc.SIZES] + ["miss_33_65", "one_33_65", "checker_33_65"] + HOSTILE


@functools.lru_cache(maxsize=None)
def case(name):
    """{"width", "height", "hist", "m2", "sphere", "normal"}; read-only."""
    if name == "loop":
        hist, m2 = loop_steps()[-1]
        pl = rc.oracle_planes(PATH[-1])
        return _frozen(dict(width=W, height=H, hist=hist, m2=m2, sphere=pl["sphere"], normal=pl["normal"]))
    kind, w, h = name.split("_")
    pattern = kind if kind in ("miss", "one", "checker") else "syn"
    return _synthetic(int(w), int(h), pattern, kind)


@functools.lru_cache(maxsize=None)
def expected(name, params):
    got = restate(case(name), *params)
    for a in got:
        a.setflags(write=False)
    return got


def params_struct(params):
    passes, k, sigma, min_history = params[:4]
    return abi.DenoiseVarParams(passes, k, sigma, min_history)


def host(lib, c, params, want_out=True, want_rgb=True, want_var=True):
    """mirt_denoise_var_host on a case: (out, out_rgb, var_out), None for an output not asked for."""
    h_, w_ = c["height"], c["width"]
    out = np.zeros((h_, w_, 4), np.uint8) if want_out else None
    rgb = np.zeros((h_, w_, 3), F32) if want_rgb else None
    var = np.zeros((h_, w_), F32) if want_var else None
    p = params_struct(params)
    r = lib.mirt_denoise_var_host(w_, h_, _p(c["hist"]), _p(c["m2"]), _p(c["sphere"]),
                                  _p(c["normal"]) if params[4] else None, C.byref(p), _p(out), _p(rgb), _p(var))
    assert r == 0, lib.mirt_last_error().decode()
    return out, rgb, var


def check(got, want, what, hostile):
    """(out, out_rgb, var_out) against the same of the restatement or of the host form; None: not asked for."""
    out, rgb, var = got
    if out is not None:
        same_bytes(out, want[0], what + " out")
    for g, w, n in ((rgb, want[1], " out_rgb"), (var, want[2], " var_out")):
        if g is not None:
            (same_values if hostile else same_bytes)(g, w, what + n)

"""The C surface of the moments reprojection and the variance-guided filter, as
far as it can be seen without a GPU: the entry points exist, the header and
abi.py agree on them, the parameter struct and its defaults, the version string
is unchanged, and every MIRT_E_INVALID of the device, blocking and frame forms
is returned before any HIP call (on a machine without a GPU a HIP call would be
MIRT_E_DEVICE) and before the context is looked at."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

E_INVALID = -1
I, P = C.c_int, C.c_void_p
F32 = np.float32
# name -> (restype, the ctypes argument list)
FORMS = {"mirt_denoise_var_params_default": (None, [P]),
         "mirt_reproject_moments_host": (I, [I, I] + [P] * 15),
         "mirt_reproject_moments_device": (I, [P, I, I] + [P] * 16),
         "mirt_reproject_moments": (I, [P, I, I] + [P] * 15),
         "mirt_denoise_var_host": (I, [I, I] + [P] * 8),
         "mirt_denoise_var_device": (I, [P, I, I] + [P] * 9),
         "mirt_denoise_var": (I, [P, I, I] + [P] * 8),
         "mirt_render_frame_reprojected_denoised": (I, [P] * 8),
         "mirt_history_moments_read": (I, [P, P, C.c_size_t])}
HOST = ("mirt_denoise_var_params_default", "mirt_reproject_moments_host", "mirt_denoise_var_host")


def header():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_exported_declared_and_bound(mirt):
    L = mirt.load()
    bound = {n: (r, a) for n, r, a in mirt.abi.SIGNATURES}
    for name, (res, args) in FORMS.items():
        assert hasattr(L, name), name
        m = re.search(r"\b(int|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
        assert m, name
        assert (m.group(1) == "int") == (res is I), name
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(params) == len(args), (name, params)
        assert [("*" in p) for p in params] == [a in (P,) for a in args], (name, params)
        assert bound[name] == (res, args), name
        if name not in HOST:
            assert params[0].startswith("mirt_ctx *"), params
    for name in ("reproject_moments", "denoise_var", "render_frame_reprojected_denoised", "history_moments_read"):
        assert callable(getattr(mirt.Renderer, name)), name
    assert L.mirt_version() == b"mirt 0.7 (gfx950)"


def test_the_parameter_struct_and_its_defaults(mirt):
    assert re.search(r"typedef\s+struct\s+mirt_denoise_var_params\s*\{\s*int32_t\s+passes;\s*int32_t\s+normal_sharpness;"
                     r"\s*float\s+sigma_lum;\s*int32_t\s+min_history;\s*\}\s*mirt_denoise_var_params;", header())
    V = mirt.abi.DenoiseVarParams
    assert C.sizeof(V) == 16
    assert [(f, t) for f, t in V._fields_] == [("passes", C.c_int32), ("normal_sharpness", C.c_int32),
                                               ("sigma_lum", C.c_float), ("min_history", C.c_int32)]
    p = V(9, 9, 9.0, 9)
    mirt.load().mirt_denoise_var_params_default(C.byref(p))
    assert (p.passes, p.normal_sharpness, p.min_history) == (3, 3, 4) and p.sigma_lum in (1.0, 2.0, 4.0, 8.0)
    mirt.load().mirt_denoise_var_params_default(None)   # ignored
    q = mirt.Renderer._denoise_var_params(None)
    assert (q.passes, q.normal_sharpness, q.sigma_lum, q.min_history) == (3, 3, p.sigma_lum, 4)
    q = mirt.Renderer._denoise_var_params((5, 0, 0.5, 1))
    assert (q.passes, q.normal_sharpness, q.sigma_lum, q.min_history) == (5, 0, 0.5, 1)


def bad_params(V):
    nan, inf = float("nan"), float("inf")
    return [("passes 0", V(0, 3, 4.0, 4)), ("passes 6", V(6, 3, 4.0, 4)), ("passes -1", V(-1, 3, 4.0, 4)),
            ("sharpness -1", V(3, -1, 4.0, 4)), ("sharpness 8", V(3, 8, 4.0, 4)), ("sigma -0.5", V(3, 3, -0.5, 4)),
            ("sigma nan", V(3, 3, nan, 4)), ("sigma inf", V(3, 3, inf, 4)), ("sigma -inf", V(3, 3, -inf, 4)),
            ("min_history 0", V(3, 3, 4.0, 0)), ("min_history -1", V(3, 3, 4.0, -1)),
            ("min_history 65537", V(3, 3, 4.0, 65537))]


p_ = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731


def test_filter_forms_invalid_before_any_hip_call(mirt):
    """A block of zero bytes stands in for a context: the checks come before
    the context is looked at, and nothing is written."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    V = mirt.abi.DenoiseVarParams
    good = V(3, 3, 4.0, 4)
    hist, m2 = np.zeros((4, 4), mirt.abi.HISTORY), np.zeros((4, 4), F32)
    sph, nrm = np.zeros((4, 4), np.int32), np.zeros((4, 4, 3), F32)
    out, rgb, var = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), F32), np.zeros((4, 4), F32)
    # (width, height, hist, m2, sphere, params, out, out_rgb)
    cases = [("NULL params", (4, 4, hist, m2, sph, None, out, None)),
             ("NULL hist", (4, 4, None, m2, sph, good, out, None)),
             ("NULL m2", (4, 4, hist, None, sph, good, out, None)),
             ("NULL sphere plane", (4, 4, hist, m2, None, good, out, None)),
             ("no output", (4, 4, hist, m2, sph, good, None, None)),
             ("width 0", (0, 4, hist, m2, sph, good, out, None)),
             ("height 0", (4, 0, hist, m2, sph, good, None, rgb)),
             ("width -4", (-4, 4, hist, m2, sph, good, out, None)),
             ("height -4", (4, -4, hist, m2, sph, good, out, None)),
             ("beyond 2^31 pixels", (65536, 32769, hist, m2, sph, good, out, None))]
    cases += [(what, (4, 4, hist, m2, sph, bad, out, rgb)) for what, bad in bad_params(V)]

    def call(name, c, a):
        w, h, hh, m, s, prm, o, f = a
        args = (w, h, p_(hh), p_(m), p_(s), p_(nrm), ref(prm), p_(o), p_(f), p_(var))
        if name == "mirt_denoise_var_host":
            return L.mirt_denoise_var_host(*args)
        if name == "mirt_denoise_var":
            return L.mirt_denoise_var(c, *args)
        return L.mirt_denoise_var_device(c, *args, None)

    fine = (4, 4, hist, m2, sph, good, out, rgb)
    for name in ("mirt_denoise_var_host", "mirt_denoise_var", "mirt_denoise_var_device"):
        if name != "mirt_denoise_var_host":
            assert call(name, None, fine) == E_INVALID
            assert L.mirt_last_error().decode() == name + ": null context", name
        for what, a in cases:
            rc = call(name, ctx, a)
            assert rc == E_INVALID, (name, what, rc)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, what)
            assert not out.any() and not rgb.any() and not var.any()
    assert bytes(fake) == bytes(16384)


def test_moments_forms_invalid_before_any_hip_call(mirt):
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    R = mirt.abi.ReprojectParams
    cam, good = mirt.default_camera(), R(64, 4, 0.015625)
    rgba, t, sph = np.zeros((4, 4, 4), np.uint8), np.ones((4, 4), F32), np.zeros((4, 4), np.int32)
    hist, m2 = np.zeros((4, 4), mirt.abi.HISTORY), np.zeros((4, 4), F32)
    hist_out, m2_out = np.zeros((4, 4), mirt.abi.HISTORY), np.zeros((4, 4), F32)
    out, rgb = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), F32)
    geo = np.ones((2, 4), F32)
    M = mirt.abi.SphereMotion
    mo = M(geo.ctypes.data, geo.ctypes.data, None, 2, 2)
    base = dict(w=4, h=4, cam=cam, cam_prev=cam, rgba=rgba, t=t, sph=sph, hist=hist, t_prev=t, sph_prev=sph, prm=good,
                hist_out=hist_out, mo=None, m2_prev=m2, m2_out=m2_out)
    first = dict(cam_prev=None, hist=None, t_prev=None, sph_prev=None, m2_prev=None)
    nan = float("nan")
    cases = [dict(prm=None), dict(cam=None), dict(rgba=None), dict(t=None), dict(sph=None), dict(hist_out=None),
             dict(cam_prev=None), dict(hist=None), dict(t_prev=None), dict(sph_prev=None), dict(hist_out=hist),
             dict(m2_prev=None), dict(first, m2_prev=m2), dict(m2_out=None), dict(m2_out=m2), dict(w=0), dict(h=-4),
             dict(w=65536, h=32769), dict(prm=R(0, 4, 0.0)), dict(prm=R(65537, 4, 0.0)), dict(prm=R(64, 2, 0.0)),
             dict(prm=R(64, 4, nan)), dict(prm=R(64, 4, -1.0)), dict(first, mo=mo),
             dict(mo=M(None, geo.ctypes.data, None, 2, 2)), dict(mo=M(geo.ctypes.data, None, None, 2, 2)),
             dict(mo=M(geo.ctypes.data, geo.ctypes.data, None, 2, 1)), dict(mo=M(geo.ctypes.data, geo.ctypes.data, None, 0, 0))]

    def call(name, c, **kw):
        a = dict(base, **kw)
        args = (a["w"], a["h"], ref(a["cam"]), ref(a["cam_prev"]), p_(a["rgba"]), p_(a["t"]), p_(a["sph"]),
                p_(a["hist"]), p_(a["t_prev"]), p_(a["sph_prev"]), ref(a["prm"]), p_(a["hist_out"]), p_(out), p_(rgb))
        tail = (ref(a["mo"]), p_(a["m2_prev"]), p_(a["m2_out"]))
        if name == "mirt_reproject_moments_host":
            return L.mirt_reproject_moments_host(*args, *tail)
        if name == "mirt_reproject_moments":
            return L.mirt_reproject_moments(c, *args, *tail)
        return L.mirt_reproject_moments_device(c, *args, None, *tail)

    for name in ("mirt_reproject_moments_host", "mirt_reproject_moments", "mirt_reproject_moments_device"):
        if name != "mirt_reproject_moments_host":
            assert call(name, None) == E_INVALID
            assert L.mirt_last_error().decode() == name + ": null context", name
        for kw in cases:
            rc = call(name, ctx, **kw)
            assert rc == E_INVALID, (name, kw, rc)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, kw)
            assert not out.any() and not rgb.any() and not hist_out.view(np.uint8).any() and not m2_out.any()
    assert bytes(fake) == bytes(16384)


def test_frame_form_invalid_before_any_hip_call(mirt):
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    R, V = mirt.abi.ReprojectParams, mirt.abi.DenoiseVarParams
    cam, good, vgood = mirt.default_camera(), R(64, 4, 0.015625), V(3, 3, 4.0, 4)
    fd = mirt.frame_desc(8, 8, depth=5)
    out, rep, raw = (np.zeros((8, 8, 4), np.uint8) for _ in range(3))
    name = "mirt_render_frame_reprojected_denoised"

    def call(c, cam_, fd_, prm, vprm, o):
        return L.mirt_render_frame_reprojected_denoised(c, ref(cam_), ref(fd_), ref(prm), ref(vprm), p_(o), p_(rep),
                                                        p_(raw))

    assert call(None, cam, fd, good, vgood, out) == E_INVALID
    assert L.mirt_last_error().decode() == name + ": null context"
    fdk = lambda **kw: mirt.frame_desc(8, 8, **dict(dict(depth=5), **kw))   # noqa: E731
    cases = [("NULL camera", (None, fd, good, vgood, out)), ("NULL descriptor", (cam, None, good, vgood, out)),
             ("NULL params", (cam, fd, None, vgood, out)), ("NULL var params", (cam, fd, good, None, out)),
             ("NULL out", (cam, fd, good, vgood, None)),
             ("accumulating", (cam, fdk(accumulate=True, frames=2), good, vgood, out)),
             ("two samples", (cam, fdk(samples=2), good, vgood, out)),
             ("two shards", (cam, fdk(shard=0, num_shards=2), good, vgood, out)),
             ("jitter", (cam, fdk(jitter=True), good, vgood, out)), ("max_depth 0", (cam, fdk(depth=0), good, vgood, out)),
             ("zero width", (cam, mirt.frame_desc(0, 8, depth=5), good, vgood, out)),
             ("taps 2", (cam, fd, R(64, 2, 0.0), vgood, out)), ("max_history 0", (cam, fd, R(0, 4, 0.0), vgood, out))]
    cases += [(what, (cam, fd, good, bad, out)) for what, bad in bad_params(V)]
    for what, a in cases:
        rc = call(ctx, *a)
        assert rc == E_INVALID, (what, rc)
        assert L.mirt_last_error().decode() == name + ": invalid arguments", what
        assert not out.any() and not rep.any() and not raw.any()
    assert L.mirt_history_moments_read(None, p_(np.zeros(4, F32)), 4) == E_INVALID
    assert bytes(fake) == bytes(16384)

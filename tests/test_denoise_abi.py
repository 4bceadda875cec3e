"""The C surface of the denoiser (mirt_denoise_params_default, mirt_denoise_host,
mirt_denoise_device, mirt_denoise, mirt_render_frame_denoised), as far as it can
be seen without a GPU: the entry points exist, the headers and abi.py agree on
them, the parameter struct and its defaults, and every MIRT_E_INVALID is
returned before any HIP call (on a machine without a GPU a HIP call would be
MIRT_E_DEVICE) and before the context is looked at."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

E_INVALID = -1
I, P = C.c_int, C.c_void_p
# name -> (restype, the ctypes argument list)
FORMS = {"mirt_denoise_params_default": (None, [P]),
         "mirt_denoise_host": (I, [I, I, P, P, I, P, P, P, P, P]),
         "mirt_denoise_device": (I, [P, I, I, P, P, I, P, P, P, P, P, P]),
         "mirt_denoise": (I, [P, I, I, P, P, I, P, P, P, P, P]),
         "mirt_render_frame_denoised": (I, [P] * 7)}


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
        assert [("*" in p) for p in params] == [a is not I for a in args], (name, params)
        assert bound[name] == (res, args), name
        if name not in ("mirt_denoise_params_default", "mirt_denoise_host"):
            assert params[0].startswith("mirt_ctx *"), params
        assert sum("const mirt_denoise_params *" in p for p in params) == (name != "mirt_denoise_params_default")
    for name in ("denoise", "render_frame_denoised"):
        assert callable(getattr(mirt.Renderer, name)), name
    assert L.mirt_version() == b"mirt 0.7 (gfx950)"
    assert re.search(r"\bMIRT_OPT_DENOISE_TILE\s*=\s*26\b", header()) and mirt.abi.OPT_DENOISE_TILE == 26


def test_the_parameter_struct_and_its_defaults(mirt):
    assert re.search(r"typedef\s+struct\s+mirt_denoise_params\s*\{\s*int32_t\s+passes;\s*int32_t\s+normal_sharpness;"
                     r"\s*float\s+sigma_colour;\s*\}\s*mirt_denoise_params;", header())
    D = mirt.abi.DenoiseParams
    assert C.sizeof(D) == 12
    assert [(f, t) for f, t in D._fields_] == [("passes", C.c_int32), ("normal_sharpness", C.c_int32),
                                               ("sigma_colour", C.c_float)]
    p = D(9, 9, 9.0)
    mirt.load().mirt_denoise_params_default(C.byref(p))
    assert (p.passes, p.normal_sharpness, p.sigma_colour) == (3, 3, 0.0)
    mirt.load().mirt_denoise_params_default(None)   # ignored
    q = mirt.Renderer._denoise_params(None)
    assert (q.passes, q.normal_sharpness, q.sigma_colour) == (3, 3, 0.0)
    q = mirt.Renderer._denoise_params((5, 0, 0.5))
    assert (q.passes, q.normal_sharpness, q.sigma_colour) == (5, 0, 0.5)


def bad_params(D):
    nan, inf = float("nan"), float("inf")
    return [("passes 0", D(0, 3, 0.0)), ("passes 6", D(6, 3, 0.0)), ("passes -1", D(-1, 3, 0.0)),
            ("sharpness -1", D(3, -1, 0.0)), ("sharpness 8", D(3, 8, 0.0)), ("sigma -0.5", D(3, 3, -0.5)),
            ("sigma nan", D(3, 3, nan)), ("sigma inf", D(3, 3, inf)), ("sigma -inf", D(3, 3, -inf))]


def test_filter_forms_invalid_before_any_hip_call(mirt):
    """A block of zero bytes stands in for a context: the checks come before
    the context is looked at, and nothing is written."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    D = mirt.abi.DenoiseParams
    good = D(3, 3, 0.0)
    rgba, acc = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32)
    sph, nrm = np.zeros((4, 4), np.int32), np.zeros((4, 4, 3), np.float32)
    out, rgb = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    # (width, height, rgba, accum, frames, sphere, params, out, out_rgb)
    cases = [("NULL params", (4, 4, rgba, None, 1, sph, None, out, None)),
             ("NULL sphere plane", (4, 4, rgba, None, 1, None, good, out, None)),
             ("both sources", (4, 4, rgba, acc, 1, sph, good, out, None)),
             ("neither source", (4, 4, None, None, 1, sph, good, out, None)),
             ("frames 0 with accum", (4, 4, None, acc, 0, sph, good, out, None)),
             ("frames -1 with accum", (4, 4, None, acc, -1, sph, good, None, rgb)),
             ("no output", (4, 4, rgba, None, 1, sph, good, None, None)),
             ("width 0", (0, 4, rgba, None, 1, sph, good, out, None)),
             ("height 0", (4, 0, rgba, None, 1, sph, good, out, None)),
             ("width -4", (-4, 4, rgba, None, 1, sph, good, out, None)),
             ("height -4", (4, -4, rgba, None, 1, sph, good, out, None)),
             ("beyond 2^31 pixels", (65536, 32769, rgba, None, 1, sph, good, out, None))]
    cases += [(what, (4, 4, rgba, None, 1, sph, bad, out, rgb)) for what, bad in bad_params(D)]

    def call(name, c, a):
        w, h, r, ac, fr, s, prm, o, f = a
        args = (w, h, p(r), p(ac), fr, p(s), p(nrm), ref(prm), p(o), p(f))
        if name == "mirt_denoise_host":
            return L.mirt_denoise_host(*args)
        if name == "mirt_denoise":
            return L.mirt_denoise(c, *args)
        return L.mirt_denoise_device(c, *args, None)

    fine = (4, 4, rgba, None, 1, sph, good, out, rgb)
    for name in ("mirt_denoise_host", "mirt_denoise", "mirt_denoise_device"):
        if name != "mirt_denoise_host":
            assert call(name, None, fine) == E_INVALID
            assert L.mirt_last_error().decode() == name + ": null context", name
        for what, a in cases:
            rc = call(name, ctx, a)
            assert rc == E_INVALID, (name, what, rc)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, what)
            assert not out.any() and not rgb.any()
    assert bytes(fake) == bytes(16384)


def test_frame_form_invalid_before_any_hip_call(mirt):
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    D, Lens = mirt.abi.DenoiseParams, mirt.abi.Lens
    cam, good, lens = mirt.default_camera(), D(3, 3, 0.0), Lens(0.5, 50.0)
    fd = mirt.frame_desc(8, 8, depth=5)
    out, raw = np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 4), np.uint8)
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
    name = "mirt_render_frame_denoised"

    def call(c, cam_, lens_, fd_, prm, o, r):
        return L.mirt_render_frame_denoised(c, ref(cam_), ref(lens_), ref(fd_), ref(prm), p(o), p(r))

    for ln in (None, lens):
        assert call(None, cam, ln, fd, good, out, raw) == E_INVALID
        assert L.mirt_last_error().decode() == name + ": null context"
    nan = float("nan")
    cases = [("NULL camera", (None, None, fd, good, out, raw)),
             ("NULL descriptor", (cam, None, None, good, out, raw)),
             ("NULL params", (cam, None, fd, None, out, raw)),
             ("NULL out", (cam, None, fd, good, None, raw)),
             ("two shards", (cam, None, mirt.frame_desc(8, 8, depth=5, shard=0, num_shards=2), good, out, raw)),
             ("second of two shards", (cam, None, mirt.frame_desc(8, 8, depth=5, shard=1, num_shards=2), good, out,
                                       None)),
             ("invalid descriptor", (cam, None, mirt.frame_desc(8, 8, depth=5, shard=2, num_shards=2), good, out, raw)),
             ("zero width", (cam, None, mirt.frame_desc(0, 8, depth=5), good, out, raw)),
             ("max_depth 0", (cam, None, mirt.frame_desc(8, 8, depth=0), good, out, raw)),
             ("max_depth 0, lens", (cam, lens, mirt.frame_desc(8, 8, depth=0), good, out, raw)),
             ("aperture -1", (cam, Lens(-1.0, 50.0), fd, good, out, raw)),
             ("aperture nan", (cam, Lens(nan, 50.0), fd, good, out, raw)),
             ("focus 0", (cam, Lens(0.5, 0.0), fd, good, out, raw)),
             ("aperture 0, focus nan", (cam, Lens(0.0, nan), fd, good, out, raw))]
    cases += [(what, (cam, None, fd, bad, out, raw)) for what, bad in bad_params(D)]
    for what, a in cases:
        rc = call(ctx, *a)
        assert rc == E_INVALID, (what, rc)
        assert L.mirt_last_error().decode() == name + ": invalid arguments", what
        assert not out.any() and not raw.any()
    assert bytes(fake) == bytes(16384)

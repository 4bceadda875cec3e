"""The C surface of the reprojection with a motion and of the carried history
(mirt_reproject_motion_host, mirt_reproject_motion_device,
mirt_reproject_motion, mirt_history_motion_get, MIRT_OPT_HISTORY_MOTION), as
far as it can be seen without a GPU: the entry points exist, the header and
abi.py agree on them, the structs' layouts, the option's values, and NULL
arguments come back before any HIP call. (tests/test_reproject_motion_host.py
has the argument table and the structs' sizes as the compiler sees them.)"""
import ctypes as C
import re

import numpy as np

from test_reproject_abi import header

I, P = C.c_int, C.c_void_p
E_INVALID = -1
FORMS = {"mirt_reproject_motion_host": (I, [I, I] + [P] * 13),
         "mirt_reproject_motion_device": (I, [P, I, I] + [P] * 14),
         "mirt_reproject_motion": (I, [P, I, I] + [P] * 13),
         "mirt_history_motion_get": (I, [P, P])}


def test_exported_declared_and_bound(mirt):
    L = mirt.load()
    hdr = header()
    bound = {n: (r, a) for n, r, a in mirt.abi.SIGNATURES}
    for name, (res, args) in FORMS.items():
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",")]
        assert len(params) == len(args), (name, params)
        assert [("*" in p) for p in params] == [a is P for a in args], (name, params)
        assert bound[name] == (res, args), name
        if name != "mirt_reproject_motion_host":
            assert params[0].startswith("mirt_ctx *"), params
        if name != "mirt_history_motion_get":
            assert params[-1] == "const mirt_sphere_motion *motion", params
            # the plain form's parameters, in its order, then the motion
            plain = re.search(name.replace("_motion", "") + r"\s*\(([^)]*)\)\s*;", hdr).group(1)
            assert [a.strip() for a in plain.split(",")] == params[:-1], name
    for name in ("reproject", "history_motion"):
        assert callable(getattr(mirt.Renderer, name)), name
    assert "motion" in mirt.Renderer.reproject.__code__.co_varnames


def test_the_structs_and_the_option(mirt):
    hdr = header()
    assert re.search(r"typedef\s+struct\s+mirt_sphere_motion\s*\{\s*const\s+float\s+\*geo,\s*\*geo_prev;"
                     r"\s*const\s+int32_t\s+\*prev_index;\s*int32_t\s+num_spheres,\s*num_prev;\s*\}"
                     r"\s*mirt_sphere_motion;", hdr)
    assert re.search(r"typedef\s+struct\s+mirt_history_motion\s*\{\s*uint64_t\s+from_scene_id,\s*to_scene_id,\s*bytes;"
                     r"\s*int32_t\s+rebuilt,\s*carried;\s*\}\s*mirt_history_motion;", hdr)
    M, H = mirt.abi.SphereMotion, mirt.abi.HistoryMotion
    assert C.sizeof(M) == 32 and C.sizeof(H) == 32
    assert list(M._fields_) == [("geo", P), ("geo_prev", P), ("prev_index", P), ("num_spheres", C.c_int32),
                                ("num_prev", C.c_int32)]
    assert list(H._fields_) == [("from_scene_id", C.c_uint64), ("to_scene_id", C.c_uint64), ("bytes", C.c_uint64),
                                ("rebuilt", C.c_int32), ("carried", C.c_int32)]
    assert re.search(r"\bMIRT_OPT_HISTORY_MOTION\s*=\s*27\b", hdr) and mirt.abi.OPT_HISTORY_MOTION == 27
    # the structs callers already pass by pointer have not grown
    assert C.sizeof(mirt.abi.ReprojectParams) == 12 and C.sizeof(mirt.abi.HistoryStats) == 56


def test_the_option_values(mirt):
    """0 and 1 are stored and read back, every other value is MIRT_E_INVALID
    and leaves the stored one; a block of zero bytes stands in for the ctx (the
    option is host state: no HIP call)."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    opt = mirt.abi.OPT_HISTORY_MOTION
    assert L.mirt_get_option(ctx, opt) == 0
    for bad in (2, -1, 3, 27, 2 ** 31 - 1):
        assert L.mirt_set_option(ctx, opt, bad) == E_INVALID, bad
        assert L.mirt_get_option(ctx, opt) == 0
    assert bytes(fake) == bytes(16384)
    assert L.mirt_set_option(ctx, opt, 1) == 0 and L.mirt_get_option(ctx, opt) == 1
    assert L.mirt_set_option(ctx, opt, 2) == E_INVALID and L.mirt_get_option(ctx, opt) == 1
    assert L.mirt_set_option(ctx, opt, 0) == 0 and L.mirt_get_option(ctx, opt) == 0
    assert bytes(fake) == bytes(16384)
    assert L.mirt_set_option(None, opt, 1) == E_INVALID


def test_null_arguments_before_any_hip_call(mirt):
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    out = mirt.abi.HistoryMotion(1, 2, 3, 4, 5)
    assert L.mirt_history_motion_get(None, C.byref(out)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_history_motion_get: invalid arguments"
    assert L.mirt_history_motion_get(ctx, None) == E_INVALID
    assert (out.from_scene_id, out.to_scene_id, out.bytes, out.rebuilt, out.carried) == (1, 2, 3, 4, 5)
    cam, good = mirt.default_camera(), mirt.abi.ReprojectParams(64, 4, 0.015625)
    n = 16
    rgba, t, sph = np.zeros((4, 4, 4), np.uint8), np.ones((4, 4), np.float32), np.zeros((4, 4), np.int32)
    hist, ho = np.zeros(n, mirt.abi.HISTORY), np.zeros(n, mirt.abi.HISTORY)
    geo = np.ones((1, 4), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    mo = mirt.abi.SphereMotion(geo.ctypes.data, geo.ctypes.data, None, 1, 1)
    args = (4, 4, C.byref(cam), C.byref(cam), p(rgba), p(t), p(sph), p(hist), p(t), p(sph), C.byref(good), p(ho), None,
            None)
    for name, call in (("mirt_reproject_motion", lambda c, m: L.mirt_reproject_motion(c, *args, m)),
                       ("mirt_reproject_motion_device", lambda c, m: L.mirt_reproject_motion_device(c, *args, None, m))):
        assert call(None, C.byref(mo)) == E_INVALID
        assert L.mirt_last_error().decode() == name + ": null context"
        assert call(ctx, None) == E_INVALID
        assert L.mirt_last_error().decode() == name + ": invalid arguments"
    assert L.mirt_reproject_motion_host(*args, None) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_reproject_motion_host: invalid arguments"
    assert bytes(fake) == bytes(16384) and not ho.view(np.uint8).any()

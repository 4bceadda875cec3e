"""The C surface of the reprojection (mirt_reproject_params_default,
mirt_reproject_host, mirt_reproject_device, mirt_reproject,
mirt_render_frame_reprojected, mirt_history_reset, mirt_history_stats_get,
mirt_history_read), as far as it can be seen without a GPU: the entry points
exist, the header and abi.py agree on them, the structs' sizes and layouts, and
the defaults. (tests/test_reproject_host.py has the argument table.)"""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

I, P = C.c_int, C.c_void_p
# name -> (restype, the ctypes argument list)
FORMS = {"mirt_reproject_params_default": (None, [P]),
         "mirt_reproject_host": (I, [I, I] + [P] * 12),
         "mirt_reproject_device": (I, [P, I, I] + [P] * 13),
         "mirt_reproject": (I, [P, I, I] + [P] * 12),
         "mirt_render_frame_reprojected": (I, [P] * 6),
         "mirt_history_reset": (I, [P]),
         "mirt_history_stats_get": (I, [P, P]),
         "mirt_history_read": (I, [P, P, C.c_size_t])}


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
        assert [("*" in p) for p in params] == [a is P for a in args], (name, params)
        assert bound[name] == (res, args), name
        if name not in ("mirt_reproject_params_default", "mirt_reproject_host"):
            assert params[0].startswith("mirt_ctx *"), params
    for name in ("mirt_reproject_host", "mirt_reproject_device", "mirt_reproject", "mirt_render_frame_reprojected"):
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", header()).group(1)
        assert params.count("const mirt_reproject_params *") == 1, name
    for name in ("reproject", "render_frame_reprojected", "history_reset", "history_stats", "history_read"):
        assert callable(getattr(mirt.Renderer, name)), name


def test_the_structs(mirt):
    hdr = header()
    assert re.search(r"typedef\s+struct\s+mirt_history_px\s*\{\s*float\s+r,\s*g,\s*b;\s*int32_t\s+n;\s*\}"
                     r"\s*mirt_history_px;", hdr)
    assert re.search(r"typedef\s+struct\s+mirt_reproject_params\s*\{\s*int32_t\s+max_history;\s*int32_t\s+taps;"
                     r"\s*float\s+t_tolerance;\s*\}\s*mirt_reproject_params;", hdr)
    assert re.search(r"typedef\s+struct\s+mirt_history_stats\s*\{\s*uint64_t\s+frames;\s*uint64_t\s+scene_id;"
                     r"\s*uint64_t\s+bytes;\s*uint64_t\s+reused;\s*uint64_t\s+fresh;\s*uint64_t\s+sky;"
                     r"\s*int32_t\s+width,\s*height;\s*\}\s*mirt_history_stats;", hdr)
    H = mirt.abi.HISTORY
    assert H.itemsize == 16 and H.names == ("r", "g", "b", "n")
    assert [H.fields[f][1] for f in H.names] == [0, 4, 8, 12]
    assert [H.fields[f][0] for f in H.names] == [np.dtype(np.float32)] * 3 + [np.dtype(np.int32)]
    R, S = mirt.abi.ReprojectParams, mirt.abi.HistoryStats
    assert C.sizeof(R) == 12
    assert list(R._fields_) == [("max_history", C.c_int32), ("taps", C.c_int32), ("t_tolerance", C.c_float)]
    assert C.sizeof(S) == 56
    assert list(S._fields_) == [(f, C.c_uint64) for f in ("frames", "scene_id", "bytes", "reused", "fresh", "sky")] + \
        [("width", C.c_int32), ("height", C.c_int32)]


def test_the_defaults(mirt):
    R = mirt.abi.ReprojectParams
    p = R(9, 9, 9.0)
    mirt.load().mirt_reproject_params_default(C.byref(p))
    assert (p.max_history, p.taps, p.t_tolerance) == (64, 4, 1.0 / 64.0)
    mirt.load().mirt_reproject_params_default(None)   # ignored
    q = mirt.Renderer._reproject_params(None)
    assert (q.max_history, q.taps, q.t_tolerance) == (64, 4, 1.0 / 64.0)
    q = mirt.Renderer._reproject_params((8, 1, 0.5))
    assert (q.max_history, q.taps, q.t_tolerance) == (8, 1, 0.5)
    assert mirt.Renderer._reproject_params(q) is q

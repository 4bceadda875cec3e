"""The C surface of frames with primary-hit planes (mirt_render_frame_planes,
_device, _async), as far as it can be seen without a GPU: the entry points
exist, the header and abi.py agree on them and on mirt_primary_planes, and a
NULL context, NULL planes, planes without a member and max_depth == 0 are
MIRT_E_INVALID before any HIP call (on a machine without a GPU a HIP call
would be MIRT_E_DEVICE)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

E_INVALID = -1
FORMS = {"mirt_render_frame_planes": 5, "mirt_render_frame_planes_device": 7, "mirt_render_frame_planes_async": 5}


def header():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_exported_declared_and_bound(mirt):
    L, hdr = mirt.load(), header()
    bound = {n: (r, a) for n, r, a in mirt.abi.SIGNATURES}
    for name, nargs in FORMS.items():
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",")]
        assert len(params) == nargs and all("*" in p for p in params), (name, params)   # every argument a pointer
        assert bound[name] == (C.c_int, [C.c_void_p] * nargs), name
        assert sum("const mirt_primary_planes *" in p for p in params) == 1, name
    assert re.search(r"typedef struct mirt_primary_planes\s*\{\s*float\s*\*t;\s*int32_t\s*\*sphere;\s*float\s*\*normal;"
                     r"\s*\}\s*mirt_primary_planes\s*;", hdr)
    P = mirt.abi.PrimaryPlanes
    assert [(f, t) for f, t in P._fields_] == [("t", C.c_void_p), ("sphere", C.c_void_p), ("normal", C.c_void_p)]
    assert C.sizeof(P) == 24 and bytes(P()) == bytes(24)
    assert L.mirt_version().startswith(b"mirt 0.7")
    for name in ("render_frame_planes", "render_frame_planes_device", "render_frame_planes_async"):
        assert callable(getattr(mirt.Renderer, name)), name


def call(L, mirt, name, ctx, fd, planes):
    """One of the three forms with valid camera, output and accumulation
    pointers, so that only ctx, fd and planes decide."""
    cam = mirt.default_camera()
    out = np.zeros(8 * 8, np.uint32)
    pl = C.byref(planes) if planes is not None else None
    if name == "mirt_render_frame_planes_device":
        return getattr(L, name)(ctx, C.byref(cam), C.byref(fd), mirt.abi.ptr(out), None, pl, None), out
    return getattr(L, name)(ctx, C.byref(cam), C.byref(fd), mirt.abi.ptr(out), pl), out


def test_invalid_before_any_hip_call(mirt):
    """A block of zero bytes stands in for a context: the planes' checks come
    before the context is looked at, and nothing is written."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    t, s, n = np.zeros(64, np.float32), np.zeros(64, np.int32), np.zeros(192, np.float32)
    full = mirt.abi.PrimaryPlanes(t.ctypes.data, s.ctypes.data, n.ctypes.data)
    fd = mirt.frame_desc(8, 8, depth=5)
    fd0 = mirt.frame_desc(8, 8, depth=0)
    for name in FORMS:
        rc, out = call(L, mirt, name, None, fd, full)
        assert rc == E_INVALID and L.mirt_last_error().decode() == name + ": null context", name
        for what, args in [("NULL planes", (fd, None)), ("no member", (fd, mirt.abi.PrimaryPlanes())),
                           ("max_depth 0", (fd0, full)),
                           ("max_depth 0, one member", (fd0, mirt.abi.PrimaryPlanes(None, s.ctypes.data, None)))]:
            rc, out = call(L, mirt, name, ctx, *args)
            assert rc == E_INVALID, (name, what, rc)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, what)
            assert not out.any()
    assert bytes(fake) == bytes(16384) and not t.any() and not s.any() and not n.any()

"""The C surface of ray frames (mirt_render_rays, mirt_render_rays_device), as
far as it can be seen without a GPU: the entry points exist, the header and
abi.py agree on them, MIRT_PCACHE_RAYS is 9, and a NULL context, NULL rays, an
invalid descriptor, a jittered descriptor, planes without a member and planes
at max_depth 0 are MIRT_E_INVALID before any HIP call (on a machine without a
GPU a HIP call would be MIRT_E_DEVICE)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

E_INVALID = -1
FORMS = {"mirt_render_rays": 5, "mirt_render_rays_device": 7}


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
        assert params[0].startswith("mirt_ctx *") and params[1].startswith("const mirt_ray *"), params
        assert params[2].startswith("const mirt_frame_desc *"), params
        assert sum("const mirt_primary_planes *" in p for p in params) == 1, name
    for name in ("render_rays", "render_rays_device"):
        assert callable(getattr(mirt.Renderer, name)), name


def test_the_cache_reason_and_the_version(mirt):
    enums = dict(re.findall(r"\b(MIRT_PCACHE_\w+)\s*=\s*(\d+)", header()))
    assert int(enums["MIRT_PCACHE_RAYS"]) == 9 and mirt.abi.PCACHE_REASON[9] == "RAYS"
    # the existing values did not move
    assert {k: int(v) for k, v in enums.items() if k != "MIRT_PCACHE_RAYS"} == {
        "MIRT_PCACHE_BYPASS": 0, "MIRT_PCACHE_FILL": 1, "MIRT_PCACHE_HIT": 2, "MIRT_PCACHE_EMPTY": 1,
        "MIRT_PCACHE_SCENE": 2, "MIRT_PCACHE_CAMERA": 3, "MIRT_PCACHE_GEOMETRY": 4, "MIRT_PCACHE_OFF": 5,
        "MIRT_PCACHE_SCHEDULE": 6, "MIRT_PCACHE_JITTER": 7, "MIRT_PCACHE_PLANES": 8}
    assert mirt.load().mirt_version() == b"mirt 0.7 (gfx950)"


def call(L, mirt, name, ctx, rays, fd, planes, out):
    pl = C.byref(planes) if planes is not None else None
    r = mirt.abi.ptr(rays) if rays is not None else None
    if name == "mirt_render_rays_device":
        return getattr(L, name)(ctx, r, C.byref(fd) if fd is not None else None, mirt.abi.ptr(out), None, pl, None)
    return getattr(L, name)(ctx, r, C.byref(fd) if fd is not None else None, mirt.abi.ptr(out), pl)


def test_invalid_before_any_hip_call(mirt):
    """A block of zero bytes stands in for a context: the checks come before
    the context is looked at, and nothing is written."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    rays = np.zeros(64, mirt.abi.RAY)
    rays["direction"][:, 2] = -1.0
    t, s, n = np.zeros(64, np.float32), np.zeros(64, np.int32), np.zeros(192, np.float32)
    full = mirt.abi.PrimaryPlanes(t.ctypes.data, s.ctypes.data, n.ctypes.data)
    fd = mirt.frame_desc(8, 8, depth=5)
    bad_fd = mirt.frame_desc(8, 8, depth=5, shard=2, num_shards=2)
    cases = [("NULL rays", (None, fd, None)), ("NULL rays, planes", (None, fd, full)),
             ("NULL descriptor", (rays, None, None)),
             ("invalid descriptor", (rays, bad_fd, None)),
             ("zero width", (rays, mirt.frame_desc(0, 8, depth=5), None)),
             ("jitter", (rays, mirt.frame_desc(8, 8, depth=5, jitter=True), None)),
             ("jitter, planes", (rays, mirt.frame_desc(8, 8, depth=5, jitter=True), full)),
             ("no member", (rays, fd, mirt.abi.PrimaryPlanes())),
             ("max_depth 0, planes", (rays, mirt.frame_desc(8, 8, depth=0), full)),
             ("max_depth 0, one member", (rays, mirt.frame_desc(8, 8, depth=0),
                                          mirt.abi.PrimaryPlanes(None, s.ctypes.data, None)))]
    for name in FORMS:
        out = np.zeros(8 * 8, np.uint32)
        assert call(L, mirt, name, None, rays, fd, full, out) == E_INVALID
        assert L.mirt_last_error().decode() == name + ": null context", name
        assert call(L, mirt, name, None, rays, fd, None, out) == E_INVALID
        assert L.mirt_last_error().decode() == name + ": null context", name
        for what, args in cases:
            rc = call(L, mirt, name, ctx, *args, out)
            assert rc == E_INVALID, (name, what, rc)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, what)
            assert not out.any()
    assert bytes(fake) == bytes(16384) and not t.any() and not s.any() and not n.any()

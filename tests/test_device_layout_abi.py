"""The device layout path's C surface, as far as it can be seen without a GPU:
the entry points exist, the header and abi.py agree on them, and bad
arguments are rejected before any HIP call (on a machine without a GPU a HIP
call would be MIRT_E_DEVICE)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

NEW = ("mirt_scene_build_device", "mirt_scene_upload_flat_device", "mirt_scene_resident_layout",
       "mirt_last_scene_build_stats")
E_INVALID = -1


def header():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_exported_declared_and_bound(mirt):
    L = mirt.load()
    hdr = header()
    declared = set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", hdr))
    bound = {n: (r, a) for n, r, a in mirt.abi.SIGNATURES}
    for name in NEW:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in bound, name
    # the prototypes: return type and parameter count, header against abi.py
    P, I = C.c_void_p, C.c_int
    want = {"mirt_scene_build_device": ("int", [P, P, I, I, I, I, P]),
            "mirt_scene_upload_flat_device": ("int", [P, P, I, P, I]),
            "mirt_scene_resident_layout": ("int64_t", [P, I, P, C.c_size_t, P]),
            "mirt_last_scene_build_stats": ("int", [P, P])}
    for name, (ret, args) in want.items():
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert m.group(1) == ret, name
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(params) == len(args), name
        for prm, ty in zip(params, args):
            assert ("*" in prm) == (ty is P), (name, prm)
            if ty is C.c_size_t:
                assert prm.startswith("size_t"), (name, prm)
        assert bound[name] == (C.c_int64 if ret == "int64_t" else I, args), name
    assert re.search(r"typedef struct mirt_scene_build_stats\s*\{[^}]*int32_t\s+on_device[^}]*int32_t\s+levels"
                     r"[^}]*int32_t\s+nodes[^}]*float\s+build_ms[^}]*float\s+layout_ms[^}]*float\s+total_ms[^}]*\}"
                     r"\s*mirt_scene_build_stats\s*;", hdr)
    assert C.sizeof(mirt.abi.SceneBuildStats) == 24
    assert [f for f, _ in mirt.abi.SceneBuildStats._fields_] == ["on_device", "levels", "nodes", "build_ms",
                                                                  "layout_ms", "total_ms"]
    assert C.sizeof(mirt.abi.BuildStats) == 20          # mirt_build_stats keeps its size
    for name in ("build_scene", "upload_device", "resident_layout", "last_scene_build_stats"):
        assert callable(getattr(mirt.Renderer, name)), name


def test_null_context_is_invalid(mirt):
    L, p = mirt.load(), mirt.abi.ptr
    s = mirt.create_random_spheres(8, 1)
    before = s.copy()
    out = np.zeros(8, mirt.abi.SPHERE)
    assert L.mirt_scene_build_device(None, p(s), 8, 0, 8, 0, p(out)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_build_device: null context"
    assert s.tobytes() == before.tobytes() and not out.view(np.uint8).any()
    assert L.mirt_scene_upload_flat_device(None, p(s), 8, None, 0) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_upload_flat_device: null context"
    raw = mirt.abi.SceneLayoutInfo()
    assert L.mirt_scene_resident_layout(None, 0, None, 0, C.byref(raw)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_resident_layout: null context"
    st = mirt.abi.SceneBuildStats()
    assert L.mirt_last_scene_build_stats(None, C.byref(st)) == E_INVALID
    assert b"mirt_last_scene_build_stats" in L.mirt_last_error()


def test_bad_arguments_are_invalid_before_the_context_is_used(mirt):
    """Ranges are checked as mirt_bvh_build_flat_device checks them, plus
    end <= num_spheres, and a tree is validated on the host, before the context
    is looked at: a block of zero bytes stands in for one."""
    L, p = mirt.load(), mirt.abi.ptr
    fake = C.create_string_buffer(8192)
    ctx = C.cast(fake, C.c_void_p)
    s = mirt.create_random_spheres(8, 1)
    before = s.copy()
    out = np.zeros(8, mirt.abi.SPHERE)
    for args in [(p(s), 8, -1, 8, 0), (p(s), 8, 5, 4, 0), (p(s), 8, 0, 9, 0), (None, 8, 0, 8, 0), (p(s), -1, 0, 0, 0)]:
        assert L.mirt_scene_build_device(ctx, *args, p(out)) == E_INVALID, args[1:]
        assert L.mirt_last_error().decode() == "mirt_scene_build_device: invalid arguments"
    assert s.tobytes() == before.tobytes() and not out.view(np.uint8).any()
    bad = np.zeros(3, mirt.abi.NODE)
    bad["sphere"] = [-1, 0, 7]
    bad["skip"] = [3, 2, 3]
    bad["bmax"] = 1.0
    assert L.mirt_scene_upload_flat_device(ctx, p(s), 3, p(bad), 3) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_upload_flat_device: malformed node 2 (sphere 7, skip 3)"
    assert L.mirt_scene_upload_flat_device(ctx, None, 3, None, 0) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_upload_flat_device: invalid arguments"
    assert bytes(fake) == bytes(8192)

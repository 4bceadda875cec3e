"""The refit's C surface, as far as it can be seen without a GPU: the entry
points exist, the header and abi.py agree on them, bad arguments are rejected
before any HIP call (on a machine without a GPU a HIP call would be
MIRT_E_DEVICE), and the host refit runs clean under ASan + UBSan in a
stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

NEW = ("mirt_bvh_refit_flat", "mirt_scene_refit_device", "mirt_scene_refit_device_ptr", "mirt_last_refit_stats")
E_INVALID = -1


def header():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_exported_declared_and_bound(mirt):
    L = mirt.load()
    hdr = header()
    declared = set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", hdr))
    bound = {n: (r, a) for n, r, a in mirt.abi.SIGNATURES}
    P, I = C.c_void_p, C.c_int
    want = {"mirt_bvh_refit_flat": [P, I, P, I, I],
            "mirt_scene_refit_device": [P, P, I, I, P],
            "mirt_scene_refit_device_ptr": [P, P, I, I, P],
            "mirt_last_refit_stats": [P, P]}
    assert set(want) == set(NEW)
    for name, args in want.items():
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in bound, name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",")]
        assert len(params) == len(args), name
        for prm, ty in zip(params, args):
            assert ("*" in prm) == (ty is P), (name, prm)
        assert bound[name] == (I, args), name
    assert re.search(r"typedef struct mirt_refit_stats\s*\{[^}]*int32_t\s+on_device[^}]*int32_t\s+nodes"
                     r"[^}]*float\s+refit_ms[^}]*float\s+layout_ms[^}]*float\s+total_ms[^}]*\}"
                     r"\s*mirt_refit_stats\s*;", hdr)
    assert C.sizeof(mirt.abi.RefitStats) == 20
    assert [f for f, _ in mirt.abi.RefitStats._fields_] == ["on_device", "nodes", "refit_ms", "layout_ms",
                                                           "total_ms"]
    assert C.sizeof(mirt.abi.SceneBuildStats) == 24      # the 0.8 structs keep their sizes
    assert C.sizeof(mirt.abi.BuildStats) == 20
    assert mirt.load().mirt_version().startswith(b"mirt 0.7")
    for name in ("refit_scene", "last_refit_stats"):
        assert callable(getattr(mirt.Renderer, name)), name
    assert callable(mirt.refit_bvh) and "refit_bvh" in mirt.__all__


def test_null_context_is_invalid(mirt):
    L, p = mirt.load(), mirt.abi.ptr
    s = mirt.create_random_spheres(8, 1)
    before = s.copy()
    out = np.zeros(15, mirt.abi.NODE)
    assert L.mirt_scene_refit_device(None, p(s), 8, 8, p(out)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_refit_device: null context"
    assert L.mirt_scene_refit_device_ptr(None, p(s), 8, 8, p(out)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_refit_device_ptr: null context"
    assert s.tobytes() == before.tobytes() and not out.view(np.uint8).any()
    st = mirt.abi.RefitStats()
    assert L.mirt_last_refit_stats(None, C.byref(st)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_last_refit_stats: null context or output"


def test_bad_arguments_are_invalid_before_the_context_is_used(mirt):
    """num_spheres, the sphere pointer and 0 <= end <= num_spheres are checked
    before the context is looked at: a block of zero bytes stands in for one."""
    L, p = mirt.load(), mirt.abi.ptr
    fake = C.create_string_buffer(8192)
    ctx = C.cast(fake, C.c_void_p)
    s = mirt.create_random_spheres(8, 1)
    out = np.zeros(15, mirt.abi.NODE)
    for fn in ("mirt_scene_refit_device", "mirt_scene_refit_device_ptr"):
        for args in [(p(s), -1, 0), (None, 8, 8), (p(s), 8, 9), (p(s), 8, -1)]:
            assert getattr(L, fn)(ctx, *args, p(out)) == E_INVALID, (fn, args[1:])
            assert L.mirt_last_error().decode() == fn + ": invalid arguments"
    assert L.mirt_last_refit_stats(ctx, None) == E_INVALID
    assert bytes(fake) == bytes(8192) and not out.view(np.uint8).any()


def test_host_refit_under_the_sanitizers():
    """tests/c/san_refit.cpp via `make -C csrc san_refit`: mirt_bvh_refit_flat on
    identity, moved and invalid inputs under ASan + UBSan, a program of its own
    (nothing is loaded into Python): every check holds and no sanitizer reports."""
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "san_refit"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(csrc, "build", "san_refit")], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "san_refit: ok" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])

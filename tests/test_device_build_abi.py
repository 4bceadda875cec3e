"""The device BVH builder's C surface, as far as it can be seen without a GPU:
the three entry points exist, are declared, and reject bad arguments before
any HIP call (on a machine without a GPU a HIP call would be MIRT_E_DEVICE)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

NEW = ("mirt_bvh_build_flat_device", "mirt_last_build_stats", "mirt_build_partition_probe")
E_INVALID = -1


def test_exported_and_declared(mirt):
    L = mirt.load()
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", hdr))
    bound = {n for n, _, _ in mirt.abi.SIGNATURES}
    for name in NEW:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in bound, name
    assert re.search(r"typedef struct mirt_build_stats\s*\{[^}]*on_device[^}]*levels[^}]*nodes[^}]*device_ms"
                     r"[^}]*total_ms[^}]*\}\s*mirt_build_stats\s*;", hdr)
    assert C.sizeof(mirt.abi.BuildStats) == 20
    for name in ("build_bvh", "last_build_stats", "partition_probe"):
        assert callable(getattr(mirt.Renderer, name)), name


def test_null_context_is_invalid(mirt):
    L = mirt.load()
    s = mirt.create_random_spheres(8, 1)
    before = s.copy()
    out, cnt = C.c_void_p(), C.c_int(-7)
    rc = L.mirt_bvh_build_flat_device(None, mirt.abi.ptr(s), 0, 8, 0, C.byref(out), C.byref(cnt))
    assert rc == E_INVALID
    assert b"mirt_bvh_build_flat_device" in L.mirt_last_error()
    assert out.value is None and cnt.value == -7 and s.tobytes() == before.tobytes()
    st = mirt.abi.BuildStats()
    assert L.mirt_last_build_stats(None, C.byref(st)) == E_INVALID
    assert b"mirt_last_build_stats" in L.mirt_last_error()
    key = np.zeros(4, np.float32)
    seg = np.array([0, 4], np.int32)
    split = np.zeros(1, np.float32)
    perm = np.zeros(4, np.int32)
    p = mirt.abi.ptr
    assert L.mirt_build_partition_probe(None, p(key), 4, p(seg), 1, p(split), p(perm)) == E_INVALID
    assert b"mirt_build_partition_probe" in L.mirt_last_error()


def test_bad_range_is_invalid_before_the_context_is_used(mirt):
    """Arguments are checked as mirt_bvh_build_flat checks them, before the
    context is looked at: a block of zero bytes stands in for one."""
    L = mirt.load()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)
    s = mirt.create_random_spheres(8, 1)
    before = s.copy()
    out, cnt = C.c_void_p(), C.c_int()
    p = mirt.abi.ptr(s)
    for args in [(p, -1, 8, 0, C.byref(out), C.byref(cnt)), (p, 5, 4, 0, C.byref(out), C.byref(cnt)),
                 (None, 0, 8, 0, C.byref(out), C.byref(cnt)), (p, 0, 8, 0, None, C.byref(cnt)),
                 (p, 0, 8, 0, C.byref(out), None)]:
        assert L.mirt_bvh_build_flat_device(ctx, *args) == E_INVALID
        assert b"mirt_bvh_build_flat_device: invalid arguments" in L.mirt_last_error()
    assert out.value is None and s.tobytes() == before.tobytes()
    assert bytes(fake) == bytes(4096)


def test_version_is_0_7(mirt):
    assert mirt.load().mirt_version().decode().startswith("mirt 0.7")

"""The C surface of the shared scene slot, the scene calls of mirt_multi and
mirt_scene_update_device_ptr, as far as it can be seen without a GPU: the
entry points exist, the headers and abi.py agree on them, NULL handles and bad
counts are rejected before any HIP call (on a machine without a GPU a HIP call
would be MIRT_E_DEVICE), and mirt_multi.h is C."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

E_INVALID = -1
P, I, D, U64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
NAMES = {
    "mirt_ctx_share_scene": ("mirt.h", I, [P, P]),
    "mirt_ctx_scene_id": ("mirt.h", U64, [P]),
    "mirt_scene_update_device_ptr": ("mirt.h", I, [P, P, I, I, I, D, P, P, P]),
    "mirt_multi_scene_build_device": ("mirt_multi.h", I, [P, P, I, I, I, I, P]),
    "mirt_multi_scene_refit_device": ("mirt_multi.h", I, [P, P, I, I]),
    "mirt_multi_scene_update_device": ("mirt_multi.h", I, [P, P, I, I, I, D, P, P, P]),
}


def header(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_exported_declared_and_bound(mirt):
    L = mirt.load()
    bound = {n: (r, a) for n, r, a in mirt.abi.SIGNATURES}
    for name, (hdr_name, ret, args) in NAMES.items():
        assert hasattr(L, name), name
        hdr = header(hdr_name)
        m = re.search(r"\b(int|uint64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert (m.group(1) == "uint64_t") == (ret is U64), name
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(params) == len(args), name
        for prm, ty in zip(params, args):
            assert ("*" in prm) == (ty is P), (name, prm)
            assert prm.startswith("double") == (ty is D), (name, prm)
        assert bound[name] == (ret, args), name
    for name in ("share_scene", "scene_id", "update_scene"):
        assert callable(getattr(mirt.Renderer, name)), name
    for name in ("build_scene", "refit_scene", "update_scene", "scene_ids"):
        assert callable(getattr(mirt.MultiRenderer, name)), name
    # nothing existing moved
    assert C.sizeof(mirt.abi.TreeQuality) == 56 and C.sizeof(mirt.abi.UpdateResult) == 96
    assert C.sizeof(mirt.abi.RefitStats) == 20 and C.sizeof(mirt.abi.SceneBuildStats) == 24
    assert L.mirt_version().startswith(b"mirt 0.7")


def test_null_handles_are_invalid(mirt):
    L, p = mirt.load(), mirt.abi.ptr
    s = mirt.create_random_spheres(8, 1)
    out, perm, res = np.zeros(8, mirt.abi.SPHERE), np.zeros(8, np.int32), mirt.abi.UpdateResult()
    fake = C.create_string_buffer(8192)                   # stands in for device memory: never looked at
    d = C.cast(fake, C.c_void_p)
    assert L.mirt_ctx_share_scene(None, None) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_ctx_share_scene: null context"
    assert L.mirt_ctx_scene_id(None) == 0
    assert L.mirt_scene_update_device_ptr(None, d, 8, 0, 8, 1.1, None, None, C.byref(res)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_update_device_ptr: null context"
    assert L.mirt_multi_scene_build_device(None, p(s), 8, 0, 8, 0, p(out)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_multi_scene_build_device: null mirt_multi"
    assert L.mirt_multi_scene_refit_device(None, p(s), 8, 8) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_multi_scene_refit_device: null mirt_multi"
    assert L.mirt_multi_scene_update_device(None, p(s), 8, 0, 8, 1.1, p(out), p(perm), C.byref(res)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_multi_scene_update_device: null mirt_multi"
    assert not out.view(np.uint8).any() and not perm.any() and bytes(res) == bytes(C.sizeof(res))
    assert bytes(fake) == bytes(8192)


def test_bad_arguments_are_invalid_before_the_handle_is_used(mirt):
    """Counts, pointers and 0 <= start <= end <= num_spheres are checked before
    the handle is looked at: a block of zero bytes stands in for one."""
    L, p = mirt.load(), mirt.abi.ptr
    fake = C.create_string_buffer(8192)
    h = C.cast(fake, C.c_void_p)
    dev = C.create_string_buffer(256)                     # stands in for device memory: never looked at
    d = C.cast(dev, C.c_void_p)
    s = mirt.create_random_spheres(8, 1)
    out, perm, res = np.zeros(8, mirt.abi.SPHERE), np.zeros(8, np.int32), mirt.abi.UpdateResult()
    ranges = [(-1, 0, 0), (8, 0, 9), (8, -1, 8), (8, 5, 4), (8, 0, -1)]
    for ns, start, end in ranges:
        assert L.mirt_scene_update_device_ptr(h, d, ns, start, end, 1.1, None, None, C.byref(res)) == E_INVALID
        assert L.mirt_last_error().decode() == "mirt_scene_update_device_ptr: invalid arguments"
        assert L.mirt_multi_scene_update_device(h, p(s), ns, start, end, 1.1, p(out), p(perm),
                                                C.byref(res)) == E_INVALID
        assert L.mirt_last_error().decode() == "mirt_multi_scene_update_device: invalid arguments"
        assert L.mirt_multi_scene_build_device(h, p(s), ns, start, end, 0, p(out)) == E_INVALID
        assert L.mirt_last_error().decode() == "mirt_multi_scene_build_device: invalid arguments"
    assert L.mirt_scene_update_device_ptr(h, None, 8, 0, 8, 1.1, None, None, None) == E_INVALID
    assert L.mirt_scene_update_device_ptr(h, d, 8, 0, 8, 1.1, d, None, None) == E_INVALID   # output == input
    assert L.mirt_multi_scene_update_device(h, None, 8, 0, 8, 1.1, None, None, None) == E_INVALID
    assert L.mirt_multi_scene_build_device(h, None, 8, 0, 8, 0, None) == E_INVALID
    for ns, end in [(-1, 0), (8, 9), (8, -1)]:
        assert L.mirt_multi_scene_refit_device(h, p(s), ns, end) == E_INVALID
        assert L.mirt_last_error().decode() == "mirt_multi_scene_refit_device: invalid arguments"
    assert L.mirt_multi_scene_refit_device(h, None, 8, 8) == E_INVALID
    assert bytes(fake) == bytes(8192) and bytes(dev) == bytes(256)
    assert not out.view(np.uint8).any() and not perm.any() and bytes(res) == bytes(C.sizeof(res))


def test_the_multi_header_is_c(tmp_path):
    src = tmp_path / "use_multi.c"
    src.write_text('#include "mirt_multi.h"\n'
                   "int use(mirt_multi *m, const mirt_sphere *s, int n, mirt_update_result *out)\n"
                   "{\n"
                   "    if (mirt_multi_scene_build_device(m, s, n, 0, n, 0, 0)) return 1;\n"
                   "    if (mirt_multi_scene_refit_device(m, s, n, n)) return 2;\n"
                   "    if (mirt_ctx_share_scene(mirt_multi_ctx(m, 0, 0), 0)) return 3;\n"
                   "    if (mirt_scene_update_device_ptr(mirt_multi_ctx(m, 0, 0), 0, 0, 0, 0, 0.0, 0, 0, out)) return 4;\n"
                   "    return mirt_multi_scene_update_device(m, s, n, 0, n, 1.15, 0, 0, out)\n"
                   "           + (int)mirt_ctx_scene_id(mirt_multi_ctx(m, 0, 0));\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)

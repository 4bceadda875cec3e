"""mirt_scene_update_device_ptr (csrc/refit_device.hip, the tagging kernel and
the device-source build entry of csrc/bvh_device.hip): the update with the
spheres read from device memory and reordered / perm written there gives the
bytes the host functions define, on both branches. Every comparison is exact."""
import ctypes as C
import importlib.util
import math
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_layouts", os.path.join(GOLDEN, "make_golden_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

F4 = np.float32
E_INVALID, E_NOSCENE = -1, -3
SIZES = [1, 2, 63, 64, 65, 257, 4097]      # both sides of a wave, a block and a grid of several blocks
QFLOATS = ("inner_area", "leaf_area", "overhead", "cost")


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def dbits(x):
    return struct.pack("<d", x)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_same_quality(got, want, what=""):
    assert set(got) == set(want), what
    for k, v in want.items():
        g = got[k]
        ok = dbits(g) == dbits(v) if k in QFLOATS else fbits(g) == fbits(v) if k == "root_area" else g == v
        assert ok, f"{what}: {k} is {g!r}, the host has {v!r}"


def assert_same_layout(mirt, got, want, what=""):
    ginfo, gparts = got
    winfo, wparts = want
    for k, v in winfo.items():
        g = ginfo[k]
        ok = fbits(g) == fbits(v) if k in gen.FLOATS else int(g) == int(v)
        assert ok, f"{what}: info.{k} is {g!r}, the host has {v!r}"
    for name, _ in mirt.abi.LAYOUT_PARTS:
        assert gparts[name].tobytes() == wparts[name].tobytes(), f"{what}: part {name} differs"


def moved(s, sigma, seed):
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(F4)
    out["radius"] *= r.uniform(0.5, 1.5, len(s)).astype(F4)
    return out


def duplicates(mirt):
    s = mirt.create_random_spheres(64, 5)
    s[8:40] = s[8]
    return s


def decay_of(cost, base):
    ok = all(x > 0.0 and math.isfinite(x) for x in (cost, base))
    return cost / base if ok else 1.0


def host_update(mirt, nodes, s2, start, end, max_decay, base):
    """What the update is defined to do, from the host functions alone."""
    ns = len(s2)
    refit = mirt.refit_bvh(nodes, s2, end).nodes
    q = mirt.bvh_quality(refit, ns)
    decay = decay_of(q["cost"], base)
    out = dict(cost=q["cost"], decay=decay, base_cost=base, rebuilt=int(max_decay > 0 and decay > max_decay))
    if not out["rebuilt"]:
        out.update(tree=refit, spheres=s2.copy(), perm=np.arange(ns, dtype=np.int32), installed=q)
        return out
    tagged = s2.copy()                                   # the colour word holds the sphere's index
    tagged["color"] = np.arange(ns, dtype="<u4").view(np.uint8).reshape(ns, 4)
    tree = mirt.build_bvh(tagged, start, end, 0).nodes
    perm = np.ascontiguousarray(tagged["color"]).view("<u4").reshape(ns).astype(np.int32)
    out.update(tree=tree, spheres=s2[perm].copy(), perm=perm, installed=mirt.bvh_quality(tree, ns))
    return out


def on_gpu(s):
    """The spheres as a (n, 20) uint8 tensor on cuda:0."""
    return torch.from_numpy(np.ascontiguousarray(s).view(np.uint8).reshape(len(s), 20).copy()).to("cuda:0")


def check_update(mirt, gpu, got, want, what, on_device=1):
    reordered, perm, res = got
    assert reordered.is_cuda and perm.is_cuda
    assert res["on_device"] == on_device, what
    assert res["rebuilt"] == want["rebuilt"], (what, res, want["decay"])
    for k in ("base_cost", "cost", "decay"):
        assert dbits(res[k]) == dbits(want[k]), f"{what}: {k} is {res[k]!r}, the host has {want[k]!r}"
    assert_same_quality(res["installed"], want["installed"], what + ", installed")
    assert same(perm.cpu().numpy(), want["perm"]), what
    assert same(reordered.cpu().numpy(), want["spheres"]), what
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(want["spheres"], want["tree"]), what)


@pytest.mark.parametrize("n", SIZES + ["duplicates"])
def test_both_branches(gpu, mirt, n):
    if n == "duplicates":
        s, n = duplicates(mirt), 64                      # the stuck group: 32 identical spheres
    else:
        s = mirt.create_random_spheres(n, 11)
    b = mirt.build_bvh(s)
    base = mirt.bvh_quality(b, n)["cost"]
    s2 = moved(s, 3.0, n)
    for max_decay in (0.0, 1e-9):                        # never rebuild; any tree is past 1e-9
        gpu.upload_device(s, b)                          # a fresh install: the update measures the base itself
        want = host_update(mirt, b.nodes, s2, 0, n, max_decay, base)
        assert want["rebuilt"] == int(max_decay > 0)
        d = on_gpu(s2)
        check_update(mirt, gpu, gpu.update_scene(d, 0, n, max_decay), want, f"{n} max {max_decay}")
        assert same(d.cpu().numpy(), s2), "the input tensor was written"


def test_null_outputs_and_a_following_host_update(gpu, mirt):
    L, p = mirt.load(), mirt.abi.ptr
    n = 257
    s = mirt.create_random_spheres(n, 11)
    b = mirt.build_bvh(s)
    base = mirt.bvh_quality(b, n)["cost"]
    gpu.upload_device(s, b)
    s2 = moved(s, 3.0, 1)
    d = on_gpu(s2)
    torch.cuda.synchronize()
    want = host_update(mirt, b.nodes, s2, 0, n, 1e-9, base)
    assert L.mirt_scene_update_device_ptr(gpu.h, C.c_void_p(d.data_ptr()), n, 0, n, 1e-9, None, None, None) == 0
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(want["spheres"], want["tree"]), "NULL outputs")
    # the host form continues from the base the device form left: the rebuilt tree's cost
    s3 = moved(want["spheres"], 0.5, 2)
    want3 = host_update(mirt, want["tree"], s3, 0, n, 0.0, want["installed"]["cost"])
    _, _, res = gpu.update_scene(s3, 0, n, 0.0)
    assert dbits(res["base_cost"]) == dbits(want["installed"]["cost"])
    assert dbits(res["cost"]) == dbits(want3["cost"]) and res["rebuilt"] == 0
    # the outputs may not be the input; without a scene there is nothing to update
    assert L.mirt_scene_update_device_ptr(gpu.h, C.c_void_p(d.data_ptr()), n, 0, n, 0.0, C.c_void_p(d.data_ptr()),
                                          None, None) == E_INVALID
    with mirt.Renderer(0) as fresh:
        assert L.mirt_scene_update_device_ptr(fresh.h, C.c_void_p(d.data_ptr()), n, 0, n, 0.0, None, None,
                                              None) == E_NOSCENE


@pytest.mark.parametrize("bad", ["nan", "negzero"])
@pytest.mark.parametrize("max_decay", [0.0, 1e-9])
def test_declined_inputs_take_the_host_path(gpu, mirt, bad, max_decay):
    n = 65
    s = mirt.create_random_spheres(n, 11)
    b = mirt.build_bvh(s)
    base = mirt.bvh_quality(b, n)["cost"]
    s2 = moved(s, 3.0, 4)
    if bad == "nan":
        s2["radius"][5] = np.nan
    else:
        s2["center"][5] = [-0.0, 1.0, 2.0]
        s2["radius"][5] = 0.0
    gpu.upload_device(s, b)
    want = host_update(mirt, b.nodes, s2, 0, n, max_decay, base)
    d = on_gpu(s2)
    check_update(mirt, gpu, gpu.update_scene(d, 0, n, max_decay), want, f"{bad} {max_decay}", on_device=0)
    assert same(d.cpu().numpy(), s2)

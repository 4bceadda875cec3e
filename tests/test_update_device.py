"""mirt_scene_quality and mirt_scene_update_device (csrc/quality_device.hip,
csrc/refit_device.hip): the quality kernel returns the bytes
mirt_bvh_quality_flat returns for the host's tree, and an update leaves the
context holding, byte for byte, what the host refit or the host build followed
by mirt_scene_upload_flat would -- whichever the measured decay decides. Every
comparison is exact."""
import ctypes as C
import importlib.util
import math
import os
import struct

import numpy as np
import pytest

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
    """(info, parts) against (info, parts): every scalar (floats as bits) and
    every part's bytes; names the part and the first differing element."""
    ginfo, gparts = got
    winfo, wparts = want
    for k, v in winfo.items():
        g = ginfo[k]
        ok = fbits(g) == fbits(v) if k in gen.FLOATS else int(g) == int(v)
        assert ok, f"{what}: info.{k} is {g!r}, the host has {v!r}"
    for name, _ in mirt.abi.LAYOUT_PARTS:
        g, w = gparts[name], wparts[name]
        assert len(g) == len(w), f"{what}: part {name} has {len(g)} elements, the host has {len(w)}"
        if g.tobytes() == w.tobytes():
            continue
        gb = np.frombuffer(g.tobytes(), np.uint8).reshape(len(g), -1)
        wb = np.frombuffer(w.tobytes(), np.uint8).reshape(len(w), -1)
        first = int(np.nonzero((gb != wb).any(axis=1))[0][0])
        raise AssertionError(f"{what}: part {name} differs first at element {first}: {g[first]!r} != {w[first]!r}")


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
    """What the update is defined to do, from the host functions alone: the
    decision, the tree and spheres it installs, and the permutation."""
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
    plain = s2.copy()
    assert same(mirt.build_bvh(plain, start, end, 0).nodes, tree) and same(plain, s2[perm])   # the colour is never read
    out.update(tree=tree, spheres=plain, perm=perm, installed=mirt.bvh_quality(tree, ns))
    return out


def check_update(mirt, gpu, got, want, what, on_device=1):
    reordered, perm, res = got
    assert res["on_device"] == on_device, what
    assert res["rebuilt"] == want["rebuilt"], (what, res, want["decay"])
    for k in ("base_cost", "cost", "decay"):
        assert dbits(res[k]) == dbits(want[k]), f"{what}: {k} is {res[k]!r}, the host has {want[k]!r}"
    assert_same_quality(res["installed"], want["installed"], what + ", installed")
    assert same(perm, want["perm"]), what
    assert same(reordered, want["spheres"]), what
    assert res["total_ms"] > 0.0
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(want["spheres"], want["tree"]), what)
    assert_same_quality(gpu.scene_quality(), want["installed"], what + ", resident")


@pytest.fixture(scope="module")
def scene10k(mirt):
    s = mirt.create_random_spheres(10000, 1)
    return s, mirt.build_bvh(s).nodes


@pytest.fixture(scope="module")
def catalogue(mirt, small):
    return gen.scenes(mirt, small)


# ------------------------------------------------- quality of the resident tree

@pytest.mark.parametrize("n", SIZES)
def test_quality_after_every_install(gpu, mirt, n):
    pre = mirt.create_random_spheres(n, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    want = mirt.bvh_quality(b, n)
    assert want["inner_nodes"] + want["leaves"] + want["dead_leaves"] == len(b)
    gpu.upload(s, b)
    assert_same_quality(gpu.scene_quality(), want, f"upload {n}")
    gpu.upload_device(s, b)
    assert_same_quality(gpu.scene_quality(), want, f"upload_device {n}")
    assert same(gpu.build_scene(pre), s)
    assert_same_quality(gpu.scene_quality(), want, f"build_scene {n}")
    for sigma in (0.05, 3.0):
        s2 = moved(s, sigma, n)
        gpu.refit_scene(s2)
        assert_same_quality(gpu.scene_quality(), mirt.bvh_quality(mirt.refit_bvh(b, s2), n), f"refit_scene {n} {sigma}")


def test_quality_of_the_catalogue(gpu, mirt, catalogue):
    """Every scene of the golden catalogue, the hand trees and those that do not
    admit ordered walks included; a scene without a tree gives all zeros."""
    unordered = []
    for name, (s, nodes) in catalogue.items():
        gpu.upload_device(s, nodes)
        got = gpu.scene_quality()
        assert_same_quality(got, mirt.bvh_quality(nodes, len(s)), name)
        if len(nodes) and not gpu.resident_layout()[0]["ordered"]:
            unordered.append(name)
        if not len(nodes):
            assert not any(got.values()), name
    for name in ("hand_falling", "hand_chain70", "hand_chain300"):
        assert name in unordered, name
    assert "bench_100000_1" in catalogue and "no_tree" in catalogue and "hand_sticks_out" in catalogue


def test_quality_10k_and_a_clamped_leaf(gpu, mirt, scene10k):
    s, nodes = scene10k
    gpu.upload(s, mirt.Bvh(nodes))
    got = gpu.scene_quality()
    assert_same_quality(got, mirt.bvh_quality(nodes, len(s)), "render 10000")
    assert (got["inner_nodes"], got["leaves"], got["clamped"]) == (14699, 9811, 0)
    live = np.nonzero((nodes["sphere"] >= 0) & ((nodes["skip"] & mirt.abi.NODE_EMPTY) == 0) & (nodes["sphere"] < len(s)))[0]
    big = nodes.copy()
    leaf = int(live[len(live) // 2])
    big["bmin"][leaf] = nodes["bmin"][0] - F4(1.0)
    big["bmax"][leaf] = nodes["bmax"][0] + F4(1.0)
    big["bmax"][int(live[3])][1] = np.nan
    gpu.upload(s, mirt.Bvh(big))
    got = gpu.scene_quality()
    assert got["clamped"] == 2
    assert_same_quality(got, mirt.bvh_quality(big, len(s)), "clamped")


def test_quality_without_a_scene(mirt):
    L = mirt.load()
    with mirt.Renderer(0) as fresh:
        q = mirt.abi.TreeQuality()
        assert L.mirt_scene_quality(fresh.h, C.byref(q)) == E_NOSCENE
        assert L.mirt_scene_quality(fresh.h, None) == E_INVALID
        fresh.upload(mirt.create_random_spheres(5, 1))
        assert not any(fresh.scene_quality().values())


# ------------------------------------------------------ update, both branches

@pytest.mark.parametrize("n", SIZES + ["duplicates"])
def test_update_both_branches(gpu, mirt, n):
    if n == "duplicates":
        s, n = duplicates(mirt), 64
    else:
        s = mirt.create_random_spheres(n, 11)
    b = mirt.build_bvh(s)
    base = mirt.bvh_quality(b, n)["cost"]
    seen = set()
    for sigma in (0.05, 3.0, 10.0):
        s2 = moved(s, sigma, n)
        for max_decay in (0.0, 1.1, 1e9):
            gpu.upload_device(s, b)                      # a fresh install: the update measures the base itself
            want = host_update(mirt, b.nodes, s2, 0, n, max_decay, base)
            check_update(mirt, gpu, gpu.update_scene(s2, 0, n, max_decay), want, f"{n} sigma {sigma} max {max_decay}")
            assert want["rebuilt"] == 0 or max_decay == 1.1
            seen.add((sigma, max_decay, want["rebuilt"]))
    if n >= 257:                                         # not vacuous: both branches were taken
        assert (10.0, 1.1, 1) in seen and (0.05, 1.1, 0) in seen, seen


def test_update_over_a_part_of_the_spheres(gpu, mirt, small):
    """benchmark.c:317 builds over [0, n - 1): the last sphere stays where it is."""
    pre = small["bench_1000_1_pre"].copy()
    s = gpu.build_scene(pre, 0, 999, 20)
    nodes = mirt.build_bvh(pre.copy(), 0, 999, 20).nodes
    base = mirt.bvh_quality(nodes, 1000)["cost"]
    s2 = moved(s, 30.0, 4)
    want = host_update(mirt, nodes, s2, 0, 999, 1.01, base)
    assert want["rebuilt"] == 1 and want["perm"][999] == 999
    check_update(mirt, gpu, gpu.update_scene(s2, 0, 999, 1.01), want, "bench 1000 over [0, 999)")


# ----------------------------------------------------------------- a sequence

def test_sequence_keeps_and_drops_the_base(gpu, mirt, small):
    s = small["render_1000_1_post"].copy()
    nodes = small["render_1000_1_tree"].copy()
    n = len(s)
    gpu.upload(s, mirt.Bvh(nodes))
    b0 = mirt.bvh_quality(nodes, n)["cost"]
    # refit, refit: the base stays the built tree's
    for k, sigma in enumerate((0.5, 3.0)):
        s2 = moved(s, sigma, 20 + k)
        want = host_update(mirt, nodes, s2, 0, n, 0.0, b0)
        check_update(mirt, gpu, gpu.update_scene(s2, 0, n, 0.0), want, f"refit {k}")
        assert want["rebuilt"] == 0 and want["installed"]["cost"] != b0
    # rebuild: decided against the old base, the new tree's cost becomes the base
    s3 = moved(s, 10.0, 22)
    want = host_update(mirt, nodes, s3, 0, n, 1.1, b0)
    assert want["rebuilt"] == 1
    check_update(mirt, gpu, gpu.update_scene(s3, 0, n, 1.1), want, "rebuild")
    s, nodes, b1 = want["spheres"], want["tree"], want["installed"]["cost"]
    assert b1 != b0
    # refit: against the rebuilt tree's cost
    s4 = moved(s, 0.5, 23)
    want = host_update(mirt, nodes, s4, 0, n, 1.1, b1)
    assert want["rebuilt"] == 0
    check_update(mirt, gpu, gpu.update_scene(s4, 0, n, 1.1), want, "refit after the rebuild")
    # a plain refit drops the base: the next update measures the resident (refit) tree
    s5 = moved(s, 3.0, 24)
    gpu.refit_scene(s5)
    resident = mirt.refit_bvh(nodes, s5).nodes
    b2 = mirt.bvh_quality(resident, n)["cost"]
    assert b2 != b1
    s6 = moved(s, 3.0, 25)
    want = host_update(mirt, resident, s6, 0, n, 1.1, b2)
    check_update(mirt, gpu, gpu.update_scene(s6, 0, n, 1.1), want, "after a plain refit")
    # so does a plain build
    pre = small["render_1000_1_pre"].copy()
    s = gpu.build_scene(pre)
    nodes = mirt.build_bvh(pre.copy()).nodes
    b3 = mirt.bvh_quality(nodes, n)["cost"]
    s7 = moved(s, 3.0, 26)
    want = host_update(mirt, nodes, s7, 0, n, 0.0, b3)
    check_update(mirt, gpu, gpu.update_scene(s7, 0, n, 0.0), want, "after a plain build")
    # and so does a host upload, which installs without ctx_install_scene: rebuild first, so that the
    # base on the context is a cost the uploaded tree does not have
    want = host_update(mirt, want["tree"], moved(s, 10.0, 27), 0, n, 1.1, b3)
    assert want["rebuilt"] == 1 and want["installed"]["cost"] != b3
    check_update(mirt, gpu, gpu.update_scene(moved(s, 10.0, 27), 0, n, 1.1), want, "a second rebuild")
    gpu.upload(s, mirt.Bvh(nodes))
    s8 = moved(s, 3.0, 28)
    want = host_update(mirt, nodes, s8, 0, n, 0.0, b3)
    check_update(mirt, gpu, gpu.update_scene(s8, 0, n, 0.0), want, "after a host upload")


# ------------------------------------------------- declined inputs and failures

@pytest.mark.parametrize("max_decay", [0.0, 1.0001])
def test_negative_zero_takes_the_host_path(gpu, mirt, small, max_decay):
    s, nodes = small["render_100_1_post"], small["render_100_1_tree"]
    gpu.upload_device(s, nodes)
    s2 = moved(s, 5.0, 4)
    s2["center"][5] = [-0.0, 1.0, 2.0]
    s2["radius"][5] = 0.0
    want = host_update(mirt, nodes, s2, 0, 100, max_decay, mirt.bvh_quality(nodes, 100)["cost"])
    assert want["rebuilt"] == int(max_decay > 0)
    check_update(mirt, gpu, gpu.update_scene(s2, 0, 100, max_decay), want, "negative zero", on_device=0)
    # the next ordinary spheres are updated on the device again, against the base this call left
    s3 = moved(want["spheres"], 0.5, 5)
    base = want["installed"]["cost"] if want["rebuilt"] else want["base_cost"]
    want3 = host_update(mirt, want["tree"], s3, 0, 100, 0.0, base)
    check_update(mirt, gpu, gpu.update_scene(s3, 0, 100, 0.0), want3, "then finite")


def test_deep_chain_takes_the_host_path(gpu, mirt):
    s, nodes = gen.hand_trees(mirt)["hand_chain70"]
    gpu.upload(s, mirt.Bvh(nodes))
    assert gpu.resident_layout()[0]["ordered"] == 0
    base = mirt.bvh_quality(nodes, len(s))["cost"]
    s2 = moved(s, 0.5, 2)
    want = host_update(mirt, nodes, s2, 0, len(s), 0.0, base)
    check_update(mirt, gpu, gpu.update_scene(s2, 0, len(s), 0.0), want, "hand_chain70", on_device=0)
    want = host_update(mirt, want["tree"], s, 0, len(s), 1e-3, base)      # any decay is past this bound: a rebuild
    assert want["rebuilt"] == 1
    check_update(mirt, gpu, gpu.update_scene(s, 0, len(s), 1e-3), want, "hand_chain70 rebuilt", on_device=0)


def test_failures_leave_the_scene_and_the_base(gpu, mirt, small):
    L, p = mirt.load(), mirt.abi.ptr
    s, nodes = small["render_100_1_post"], small["render_100_1_tree"]
    gpu.upload(s, mirt.Bvh(nodes.copy()))
    b0 = mirt.bvh_quality(nodes, 100)["cost"]
    s1 = moved(s, 3.0, 1)
    want = host_update(mirt, nodes, s1, 0, 100, 0.0, b0)
    check_update(mirt, gpu, gpu.update_scene(s1, 0, 100, 0.0), want, "refit")      # resident cost != base now
    assert want["installed"]["cost"] != b0
    before = gpu.resident_layout()
    s2 = moved(s, 3.0, 2)
    with pytest.raises(mirt.MirtError, match="invalid arguments"):
        gpu.update_scene(s2, 0, 101, 1.1)
    with pytest.raises(mirt.MirtError, match="end 99 does not lie behind the last leaf's sphere 99"):
        gpu.update_scene(s2, 0, 99, 1.1)
    with pytest.raises(mirt.MirtError, match="99 spheres for a resident scene of 100"):
        gpu.update_scene(s2[:99], 0, 99, 1.1)
    assert L.mirt_scene_update_device(gpu.h, None, 100, 0, 100, 1.1, None, None, None) == E_INVALID
    assert_same_layout(mirt, gpu.resident_layout(), before, "after the refused calls")
    # the base is still the built tree's, not the resident refit tree's; NULL outputs are allowed
    assert L.mirt_scene_update_device(gpu.h, p(s2), 100, 0, 100, 0.0, None, None, None) == 0
    s3 = moved(s, 3.0, 3)
    want = host_update(mirt, nodes, s3, 0, 100, 0.0, b0)
    check_update(mirt, gpu, gpu.update_scene(s3, 0, 100, 0.0), want, "after the refused calls")
    with mirt.Renderer(0) as fresh:
        res = mirt.abi.UpdateResult()
        assert L.mirt_scene_update_device(fresh.h, p(s2), 100, 0, 100, 1.1, None, None, C.byref(res)) == E_NOSCENE
        assert bytes(res) == bytes(C.sizeof(res))


# ---------------------------------------------------------------------- frames

def test_frames_after_each_branch(gpu, mirt, small):
    s = small["render_1000_1_pre"].copy()
    b = mirt.build_bvh(s)
    base = mirt.bvh_quality(b, len(s))["cost"]
    cam = mirt.default_camera()
    s2 = moved(s, 10.0, 6)
    with mirt.Renderer(0) as host:
        for max_decay in (0.0, 1.1):
            gpu.upload(s, b)
            want = host_update(mirt, b.nodes, s2, 0, len(s), max_decay, base)
            assert want["rebuilt"] == int(max_decay > 0)
            _, _, res = gpu.update_scene(s2, 0, len(s), max_decay)
            assert res["rebuilt"] == want["rebuilt"] and res["on_device"] == 1
            host.upload(want["spheres"], mirt.Bvh(want["tree"]))
            got = gpu.render_frame(cam, 160, 90, depth=5, seed=1)
            assert same(got, host.render_frame(cam, 160, 90, depth=5, seed=1)), max_decay
            assert (got[..., :3] != got[0, 0, :3]).any()

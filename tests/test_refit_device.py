"""mirt_scene_refit_device[_ptr] (csrc/refit_device.hip): the resident scene
refit to moved spheres on the device leaves the context holding, byte for byte,
what mirt_bvh_refit_flat on the resident tree followed by
mirt_scene_upload_flat would -- read back through mirt_scene_resident_layout
and compared part by part with mirt_scene_layout of the host refit. Every
comparison is exact."""
import ctypes as C
import importlib.util
import os

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
# scenes of the golden catalogue whose tree was not built over all their spheres: one past the last sphere it covers
CATALOGUE_END = {"bench_1000_1": 999, "orphan_phantom": 3}


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


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


def host_layout(mirt, nodes, s2, end):
    return mirt.scene_layout(s2, mirt.refit_bvh(nodes, s2, end))


@pytest.fixture(scope="module")
def scene10k(mirt):
    s = mirt.create_random_spheres(10000, 1)
    return s, mirt.build_bvh(s).nodes


@pytest.fixture(scope="module")
def catalogue(mirt, small):
    return gen.scenes(mirt, small)


# --------------------------------------------------------------- identity

@pytest.mark.parametrize("name", ["render_1000", "duplicates_64", "bench_1000"])
def test_identity(gpu, mirt, small, name):
    """build_scene, then a refit with the spheres it returned: nothing moves."""
    if name == "render_1000":
        pre, start, end, depth = small["render_1000_1_pre"].copy(), 0, 1000, 0
    elif name == "duplicates_64":
        pre, start, end, depth = duplicates(mirt), 0, 64, 0
    else:
        pre, start, end, depth = small["bench_1000_1_pre"].copy(), 0, 999, 20     # benchmark.c:317
    reordered = gpu.build_scene(pre, start, end, depth)
    assert gpu.last_scene_build_stats()["on_device"] == 1
    before = gpu.resident_layout()
    host = pre.copy()
    want = mirt.build_bvh(host, start, end, depth).nodes
    assert same(host, reordered)
    keep = reordered.copy()
    got = gpu.refit_scene(reordered, end, return_nodes=True)
    assert same(reordered, keep)
    st = gpu.last_refit_stats()
    assert st["on_device"] == 1 and st["nodes"] == len(want), st
    assert same(got.nodes, want)
    assert_same_layout(mirt, gpu.resident_layout(), before, name)
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(reordered, want), name)


# ------------------------------------------------------- moved, part by part

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4097])
def test_moved_random_scenes(gpu, mirt, n):
    """A single-leaf root, and both sides of a wave, a block and a scan tile;
    the scene installed by each of the three calls that can install one."""
    pre = mirt.create_random_spheres(n, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    if n % 3 == 2:
        assert same(gpu.build_scene(pre), s)
    else:
        (gpu.upload, gpu.upload_device)[n % 3](s, b)
    for sigma in (0.05, 3.0):
        s2 = moved(s, sigma, n)
        got = gpu.refit_scene(s2, return_nodes=True)
        assert gpu.last_refit_stats()["on_device"] == 1
        assert same(got.nodes, mirt.refit_bvh(b, s2).nodes), (n, sigma)
        assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, b.nodes, s2, n), f"render {n} sigma {sigma}")


def test_moved_render_10000(gpu, mirt, scene10k):
    s, nodes = scene10k
    gpu.upload(s, mirt.Bvh(nodes))
    s2 = moved(s, 3.0, 1)
    gpu.refit_scene(s2)
    st = gpu.last_refit_stats()
    assert st["on_device"] == 1 and st["nodes"] == len(nodes), st
    assert st["refit_ms"] >= 0.0 and st["layout_ms"] > 0.0 and st["total_ms"] >= st["refit_ms"], st
    assert st["total_ms"] >= st["refit_ms"] + st["layout_ms"], st
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s2, len(s)), "render 10000")


def test_moved_duplicates(gpu, mirt):
    """One stuck group of 32 spheres; then 200 of 256 identical: a range longer
    than a lane folds alone, handed to a wave."""
    for n, lo, hi in ((64, 8, 40), (256, 20, 220)):
        s = mirt.create_random_spheres(n, 5)
        s[lo:hi] = s[lo]
        b = mirt.build_bvh(s)
        gpu.upload(s, b)
        r = np.random.default_rng(n)
        s2 = moved(s, 0.5, 3)
        s2["center"][lo:hi] += r.normal(0.0, 2.0, (hi - lo, 3)).astype(F4)     # the group spreads out
        gpu.refit_scene(s2)
        assert gpu.last_refit_stats()["on_device"] == 1
        assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, b.nodes, s2, n), f"duplicates {n}")


def test_moved_catalogue(gpu, mirt, catalogue):
    """Every `ordered` scene of the golden catalogue (tests/golden/make_golden_layouts.py)."""
    done = []
    for name, (s, nodes) in catalogue.items():
        if not len(nodes) or not mirt.scene_layout(s, nodes)[0]["ordered"]:
            continue
        end = CATALOGUE_END.get(name, len(s))
        gpu.upload_device(s, nodes)
        s2 = moved(s, 0.05 * float(np.abs(s["radius"]).max()), 9)
        gpu.refit_scene(s2, end)
        finite = np.isfinite(s2["center"][:end]).all() and np.isfinite(s2["radius"][:end]).all()
        assert gpu.last_refit_stats()["on_device"] == int(finite), name       # hand_nan_centre is declined
        assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s2, end), name)
        done.append(name)
    for name in ("render_20_1", "bench_1000_1", "render_10000_1", "bench_100000_1", "cluster", "single_leaf",
                 "edge_tiny_far", "edge_huge", "edge_offset"):
        assert name in done, name


def test_no_tree_gets_its_spheres_replaced(gpu, mirt):
    s = mirt.create_random_spheres(5, 1)
    gpu.upload(s)
    s2 = moved(s, 3.0, 2)
    got = gpu.refit_scene(s2, return_nodes=True)
    assert len(got) == 0 and gpu.last_refit_stats()["nodes"] == 0
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(s2), "no tree")


# ------------------------------------------------------------- declined inputs

@pytest.mark.parametrize("case", ["negzero", "nan_centre", "inf_radius"])
def test_declined_spheres_take_the_host_path(gpu, mirt, small, case):
    s, nodes = small["render_100_1_post"], small["render_100_1_tree"]
    gpu.upload_device(s, nodes)
    s2 = moved(s, 0.5, 4)
    if case == "negzero":
        s2["center"][5] = [-0.0, 1.0, 2.0]
        s2["radius"][5] = 0.0
    elif case == "nan_centre":
        s2["center"][17, 1] = np.nan
    else:
        s2["radius"][40] = np.inf
    got = gpu.refit_scene(s2, return_nodes=True)
    st = gpu.last_refit_stats()
    assert st["on_device"] == 0 and st["refit_ms"] == 0.0 and st["layout_ms"] == 0.0 and st["nodes"] == len(nodes), st
    assert same(got.nodes, mirt.refit_bvh(nodes, s2).nodes)
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s2, len(s)), case)
    # the next ordinary spheres are refit on the device again
    s3 = moved(s, 0.5, 5)
    gpu.refit_scene(s3)
    assert gpu.last_refit_stats()["on_device"] == 1
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s3, len(s)), case + ", then finite")


def test_deep_chain_takes_the_host_path(gpu, mirt):
    s, nodes = gen.hand_trees(mirt)["hand_chain70"]
    gpu.upload(s, mirt.Bvh(nodes))
    assert gpu.resident_layout()[0]["ordered"] == 0
    s2 = moved(s, 0.5, 2)
    gpu.refit_scene(s2)
    assert gpu.last_refit_stats()["on_device"] == 0
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s2, len(s)), "hand_chain70")


# --------------------------------------------------------------- invalid input

def test_invalid_inputs_leave_the_scene(gpu, mirt, small):
    L, p = mirt.load(), mirt.abi.ptr
    s, nodes = gen.hand_trees(mirt)["hand_falling"]
    gpu.upload(s, mirt.Bvh(nodes))
    before = gpu.resident_layout()
    with pytest.raises(mirt.MirtError, match="do not increase"):
        gpu.refit_scene(moved(s, 0.5, 1))
    assert_same_layout(mirt, gpu.resident_layout(), before, "hand_falling")
    s, nodes = small["render_100_1_post"], small["render_100_1_tree"]
    gpu.upload(s, mirt.Bvh(nodes.copy()))
    before = gpu.resident_layout()
    s2 = moved(s, 0.5, 1)
    live = (nodes["sphere"] >= 0) & ((nodes["skip"] & mirt.abi.NODE_EMPTY) == 0) & (nodes["sphere"] < 100)
    assert int(nodes["sphere"][live].max()) == 99
    with pytest.raises(mirt.MirtError, match="end 99 does not lie behind the last leaf's sphere 99"):
        gpu.refit_scene(s2, 99)
    with pytest.raises(mirt.MirtError, match="invalid arguments"):
        gpu.refit_scene(s2, 101)
    with pytest.raises(mirt.MirtError, match="99 spheres for a resident scene of 100"):
        gpu.refit_scene(s2[:99])
    assert L.mirt_scene_refit_device(gpu.h, None, 100, 100, None) == E_INVALID
    assert_same_layout(mirt, gpu.resident_layout(), before, "after the refused calls")
    with mirt.Renderer(0) as fresh:
        assert L.mirt_scene_refit_device(fresh.h, p(s2), 100, 100, None) == E_NOSCENE
        st = mirt.abi.RefitStats()
        assert L.mirt_last_refit_stats(fresh.h, C.byref(st)) == E_INVALID


# -------------------------------------------------------------- frames and hits

def test_frames_and_hits_after_a_refit(gpu, mirt, small, oracle):
    s = small["render_1000_1_pre"].copy()
    b = mirt.build_bvh(s)
    s2 = moved(s, 3.0, 6)
    b2 = mirt.refit_bvh(b, s2)
    cam = mirt.default_camera()
    gpu.upload(s, b)
    gpu.refit_scene(s2)
    assert gpu.last_refit_stats()["on_device"] == 1
    with mirt.Renderer(0) as host:
        host.upload(s2, b2)
        for W, H, depth in ((160, 90, 5), (77, 45, 1)):
            got = gpu.render_frame(cam, W, H, depth=depth, seed=1)
            assert same(got, host.render_frame(cam, W, H, depth=depth, seed=1)), (W, H, depth)
            assert (got[..., :3] != got[0, 0, :3]).any()
    rays = gpu.get_camera_rays(cam, 160, 90).reshape(-1)
    got = gpu.closest_hit(rays)
    want = oracle.intersect_flat(b2.nodes, s2, rays)
    assert want["hit"].any()
    assert same(got["hit"], want["hit"]) and same(got["t"], want["t"]) and same(got["sphere"], want["sphere"])
    frames = []
    try:
        for once in (0, 1):
            gpu.set_option(mirt.abi.OPT_CONFIRM_ONCE, once)
            frames.append(gpu.render_frame(cam, 160, 90, depth=5, seed=3))
    finally:
        gpu.set_option(mirt.abi.OPT_CONFIRM_ONCE, 2)
    assert same(frames[0], frames[1])


def test_enqueued_frame_finishes_on_the_old_scene(mirt, small):
    """render_frame_async(A), refit to B, render: the first buffer holds A's
    frame, the second B's. The first frame starts behind a bounded 30 ms wait
    (the MIRT_OPT_DEBUG_STALL_MS hook), so it is still queued when the refit is called."""
    s = small["render_1000_1_pre"].copy()
    b = mirt.build_bvh(s)
    s2 = moved(s, 3.0, 8)
    cam = mirt.default_camera()
    fd = mirt.frame_desc(160, 90, depth=5, seed=1)
    with mirt.Renderer(0) as host:
        host.upload(s, b)
        want_a = host.render_frame(cam, 160, 90, depth=5, seed=1)
        host.upload(s2, mirt.refit_bvh(b, s2))
        want_b = host.render_frame(cam, 160, 90, depth=5, seed=1)
    assert not same(want_a, want_b)
    bufs = [mirt.HostBuffer((90, 160, 4)) for _ in range(2)]
    try:
        with mirt.Renderer(0) as r:
            r.upload(s, b)
            r.set_option(mirt.abi.OPT_DEBUG_STALL_MS, 30)
            r.render_frame_async(cam, fd, bufs[0])
            r.set_option(mirt.abi.OPT_DEBUG_STALL_MS, 0)
            r.refit_scene(s2)
            r.render_frame_async(cam, fd, bufs[1])
            r.wait()
            assert same(bufs[0].array, want_a)
            assert same(bufs[1].array, want_b)
    finally:
        for x in bufs:
            x.close()


# ---------------------------------------------------------------- determinism

def test_sixteen_refits_alternate_exactly(gpu, mirt, scene10k):
    s, nodes = scene10k
    a, b = moved(s, 3.0, 1), moved(s, 0.05, 2)
    want = [host_layout(mirt, nodes, a, len(s)), host_layout(mirt, nodes, b, len(s))]
    gpu.upload(s, mirt.Bvh(nodes))
    for k in range(16):
        gpu.refit_scene((a, b)[k % 2])
        assert gpu.last_refit_stats()["on_device"] == 1
        assert_same_layout(mirt, gpu.resident_layout(), want[k % 2], f"refit {k}")


# ------------------------------------------------------------ pointer variant

def test_pointer_variant_equals_the_host_pointer_call(gpu, mirt, scene10k):
    s, nodes = scene10k
    gpu.upload(s, mirt.Bvh(nodes))
    s2 = moved(s, 3.0, 12)
    want_nodes = gpu.refit_scene(s2, return_nodes=True)
    want = gpu.resident_layout()
    gpu.refit_scene(moved(s, 0.05, 13))                       # something else in between
    t = torch.from_numpy(s2.view(np.uint8).reshape(-1, 20).copy()).to("cuda:0")
    got_nodes = gpu.refit_scene(t, return_nodes=True)
    st = gpu.last_refit_stats()
    assert st["on_device"] == 1 and st["nodes"] == len(nodes), st
    assert same(got_nodes.nodes, want_nodes.nodes)
    assert_same_layout(mirt, gpu.resident_layout(), want, "device pointer")
    assert same(t.cpu().numpy(), s2.view(np.uint8).reshape(-1, 20))      # read, not written
    # a declined sphere arriving through the device pointer: the host refit on a downloaded copy
    s3 = s2.copy()
    s3["center"][7] = [np.nan, 0.0, 0.0]
    t3 = torch.from_numpy(s3.view(np.uint8).reshape(-1, 20).copy()).to("cuda:0")
    gpu.refit_scene(t3)
    assert gpu.last_refit_stats()["on_device"] == 0
    assert_same_layout(mirt, gpu.resident_layout(), host_layout(mirt, nodes, s3, len(s)), "device pointer, NaN")
    with pytest.raises(mirt.MirtError, match="contiguous"):
        gpu.refit_scene(torch.zeros(20 * len(s), dtype=torch.uint8))    # a host tensor


# ---------------------------------------------------------------------- stats

def test_stats(gpu, mirt, small):
    s, nodes = small["render_1000_1_post"], small["render_1000_1_tree"]
    gpu.upload(s, mirt.Bvh(nodes.copy()))
    gpu.refit_scene(moved(s, 0.5, 1))
    st = gpu.last_refit_stats()
    assert st["nodes"] == len(nodes) and st["on_device"] == 1, st
    assert st["total_ms"] >= st["refit_ms"] >= 0.0 and st["layout_ms"] >= 0.0, st

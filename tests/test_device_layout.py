"""The device layouts derived ON the device (csrc/scene_device.hip):
mirt_scene_upload_flat_device and mirt_scene_build_device leave the context
holding, byte for byte, what mirt_scene_upload_flat's host builders derive --
read back through mirt_scene_resident_layout and compared with the goldens of
tests/golden/layouts.json (made by the commit before the host builders moved,
not by any code under test here) and with mirt_scene_layout part by part."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, sha

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_layouts", os.path.join(GOLDEN, "make_golden_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "layouts.json")) as _f:
    LAYOUTS = json.load(_f)["scenes"]

E_INVALID, E_NOSCENE = -1, -3


@pytest.fixture(scope="module")
def scenes(mirt, small):
    return gen.scenes(mirt, small)


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def assert_same_layout(mirt, got, want, what=""):
    """(info, parts) against (info, parts): every scalar (floats as bits) and
    every part's bytes; names the part and the first differing element."""
    ginfo, gparts = got
    winfo, wparts = want
    for k, v in winfo.items():
        g = ginfo[k]
        same = fbits(g) == fbits(v) if k in gen.FLOATS else int(g) == int(v)
        assert same, f"{what}: info.{k} is {g!r}, the host has {v!r}"
    for name, _ in mirt.abi.LAYOUT_PARTS:
        g, w = gparts[name], wparts[name]
        assert len(g) == len(w), f"{what}: part {name} has {len(g)} elements, the host has {len(w)}"
        if g.tobytes() == w.tobytes():
            continue
        gb = np.frombuffer(g.tobytes(), np.uint8).reshape(len(g), -1)
        wb = np.frombuffer(w.tobytes(), np.uint8).reshape(len(w), -1)
        first = int(np.nonzero((gb != wb).any(axis=1))[0][0])
        raise AssertionError(f"{what}: part {name} differs first at element {first}: {g[first]!r} != {w[first]!r}")


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------- goldens

def test_golden_covers_the_scenes(scenes):
    assert list(LAYOUTS) == list(scenes)
    for name in ("no_tree", "empty", "single_leaf", "hand_falling", "hand_chain70", "hand_chain300",
                 "hand_sticks_out", "hand_nan_centre", "orphan_phantom", "edge_tiny_far", "edge_huge", "edge_offset",
                 "cluster", "render_10000_1", "bench_100000_1"):
        assert name in scenes, name


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_golden_layouts(gpu, scenes, name):
    """upload_device, then the resident layout: the parent commit's bytes."""
    s, nodes = scenes[name]
    gpu.upload_device(s, nodes)
    info, parts = gpu.resident_layout()
    got, want = gen.record(info, parts), LAYOUTS[name]
    assert got["info"] == want["info"]
    for part, digest in want["sha"].items():
        assert got["sha"][part] == digest, part
    assert got == want


# ------------------------------------------------------------ part by part

@pytest.mark.parametrize("n", [2, 3, 7, 64, 65, 300, 1025])
def test_parts_random_scenes(gpu, mirt, n):
    s = mirt.create_random_spheres(n, 11)
    b = mirt.build_bvh(s)
    gpu.upload_device(s, b)
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(s, b), f"render {n}")


def quantised_scene(mirt, seed):
    """test_device_build.py's quantised_scene: coordinates and radii on
    multiples of 1/8, few distinct values, one axis constant -- zero-extent
    boxes, tied areas, groups of equal centres stuck down to depth 40."""
    r = np.random.default_rng(seed)
    n = 4096 if seed == 0 else int(r.integers(2, 4097))
    span = int(r.integers(1, 33))
    s = np.zeros(n, mirt.abi.SPHERE)
    s["center"] = r.integers(-span, span + 1, (n, 3)) / 8.0
    s["center"][:, seed % 3] = r.integers(-4, 5) / 8.0
    s["radius"] = r.integers(0, 4, n) / 8.0
    s["color"] = r.integers(0, 256, (n, 4))
    return s


def test_parts_tie_heavy_scenes(gpu, mirt):
    for seed in range(12):
        s = quantised_scene(mirt, seed)
        b = mirt.build_bvh(s)
        gpu.upload_device(s, b)
        assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(s, b), f"quantised seed {seed}")


def test_host_upload_reads_back_the_same(gpu, mirt, small):
    """mirt_scene_resident_layout reads whichever call installed the scene."""
    s, t = small["render_100_1_post"], small["render_100_1_tree"]
    gpu.upload(s, mirt.Bvh(t.copy()))
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(s, t), "host upload")


# --------------------------------- build_scene against host build + host upload

def check_build_scene(gpu, mirt, pre, start, end, depth, post=None, tree=None, what=""):
    ref = pre.copy()
    want_tree = mirt.build_bvh(ref, start, end, depth).nodes
    if post is not None:
        assert same(ref, post) and same(want_tree, tree)
    before = pre.copy()
    out = gpu.build_scene(pre, start, end, depth)
    assert same(pre, before), f"{what}: the caller's spheres were written"
    assert same(out, ref), f"{what}: reordered spheres"
    st = gpu.last_scene_build_stats()
    assert st["on_device"] == 1, st
    assert st["nodes"] == len(want_tree) and 1 <= st["levels"] <= max(1, 41 - depth), st
    assert st["build_ms"] > 0.0 and st["layout_ms"] > 0.0, st
    assert st["total_ms"] >= st["build_ms"] + st["layout_ms"], st
    got = gpu.resident_layout()
    d = got[1]["dnodes"]
    for k in ("bmin", "bmax", "sphere", "skip"):
        assert same(d[k], want_tree[k]), f"{what}: resident node field {k}"
    assert_same_layout(mirt, got, mirt.scene_layout(ref, want_tree), what)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [20, 100, 1000])
def test_build_scene_reference_fixtures(gpu, mirt, small, n, seed):
    key = f"render_{n}_{seed}"
    check_build_scene(gpu, mirt, small[key + "_pre"].copy(), 0, n, 0, small[key + "_post"], small[key + "_tree"], key)


def test_build_scene_benchmark_fixture(gpu, mirt, small):
    check_build_scene(gpu, mirt, small["bench_1000_1_pre"].copy(), 0, 999, 20, small["bench_1000_1_post"],
                      small["bench_1000_1_tree"], "bench_1000_1")     # benchmark.c:317


def test_build_scene_sub_range(gpu, mirt):
    check_build_scene(gpu, mirt, mirt.create_random_spheres(300, 4), 5, 297, 33, what="sub range")


@pytest.mark.parametrize("n", [0, 1])
def test_build_scene_tiny(gpu, mirt, n):
    check_build_scene(gpu, mirt, mirt.create_random_spheres(n, 3), 0, n, 0, what=f"n = {n}")


def test_build_scene_declined_inputs(gpu, mirt, small):
    """A NaN radius, and a sphere box with a -0.0 coordinate: host build and
    host upload, same resident scene; the next ordinary scene is built on the
    device."""
    for case in ("nan", "negzero"):
        s = small["render_100_1_pre"].copy()
        if case == "nan":
            s["radius"][17] = np.nan
        else:
            s["center"][5] = [-0.0, 1.0, 2.0]
            s["radius"][5] = 0.0
        ref = s.copy()
        want = mirt.build_bvh(ref).nodes
        before = s.copy()
        out = gpu.build_scene(s)
        st = gpu.last_scene_build_stats()
        assert st["on_device"] == 0 and st["build_ms"] == 0.0 and st["layout_ms"] == 0.0, (case, st)
        assert st["nodes"] == len(want), case
        assert same(s, before) and same(out, ref), case
        assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(ref, want), case)
    check_build_scene(gpu, mirt, small["render_100_1_pre"].copy(), 0, 100, 0, small["render_100_1_post"],
                      small["render_100_1_tree"], "after the declined inputs")


# ------------------------------------------------------------------ in use

def test_build_scene_renders_the_golden_frame(gpu, mirt, golden, small):
    gpu.build_scene(small["render_100_1_pre"].copy())
    assert gpu.last_scene_build_stats()["on_device"] == 1
    cam = mirt.abi.Camera.from_numpy(small["cameras"][0])
    img = gpu.render_frame(cam, 160, 90, depth=5, seed=1)
    assert sha(img) == golden["frames"]["160x90_render100_d5_m1_b1_s1_c0_step1"]["sha"]


def test_build_scene_batches_and_overlay_equal_the_host_path(gpu, mirt, small):
    """The benchmark-shaped scene (built over [0, n - 1) from depth 20): closest
    hits, any hits and the BVH overlay equal a second context's that took the
    host build and the host upload."""
    pre = small["bench_1000_1_pre"]
    n = len(pre)
    rays = mirt.create_bench_rays(256, mirt.RandState(7))
    cam = mirt.default_camera()
    out = gpu.build_scene(pre.copy(), 0, n - 1, 20)
    assert gpu.last_scene_build_stats()["on_device"] == 1
    got = (gpu.closest_hit(rays), gpu.any_hit(rays, use_bvh=True), gpu.bvh_overlay(cam, 160, 90))
    with mirt.Renderer(0) as host:
        s = pre.copy()
        b = mirt.build_bvh(s, 0, n - 1, 20)
        host.upload(s, b)
        want = (host.closest_hit(rays), host.any_hit(rays, use_bvh=True), host.bvh_overlay(cam, 160, 90))
    assert same(out, s)
    assert want[0]["hit"].any() and want[2].any()
    for g, w, what in zip(got, want, ("closest_hit", "any_hit", "bvh_overlay")):
        assert same(g, w), what


def test_installed_arrays_belong_to_the_context(mirt, small):
    """A device-built scene, then a host upload of another, then close: the
    arrays the kernels made are released as an upload's are, with no error."""
    r = mirt.Renderer(0)
    try:
        r.build_scene(small["render_100_1_pre"].copy())
        s = small["render_20_1_post"]
        r.upload(s, mirt.Bvh(small["render_20_1_tree"].copy()))
        assert_same_layout(mirt, r.resident_layout(), mirt.scene_layout(s, small["render_20_1_tree"]), "re-upload")
        r.upload_device(s, small["render_20_1_tree"])
        r.build_scene(small["render_100_2_pre"].copy())
        cam = mirt.abi.Camera.from_numpy(small["cameras"][0])
        assert r.render_frame(cam, 64, 32, depth=2, seed=1).shape == (32, 64, 4)
    finally:
        r.close()
    with mirt.Renderer(0) as again:       # the device is in order: a new context works
        again.upload_device(s, small["render_20_1_tree"])
        assert again.resident_layout()[0]["num_pnodes"] >= 1


# ------------------------------------------------------------------ errors

def test_build_scene_argument_errors(gpu, mirt):
    L, p = mirt.load(), mirt.abi.ptr
    s = mirt.create_random_spheres(8, 1)
    out = np.zeros(8, mirt.abi.SPHERE)
    assert L.mirt_scene_build_device(None, p(s), 8, 0, 8, 0, p(out)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_build_device: null context"
    for args in [(p(s), 8, 0, 9, 0), (p(s), 8, -1, 8, 0), (p(s), 8, 5, 4, 0), (None, 8, 0, 8, 0), (p(s), -1, 0, 0, 0)]:
        assert L.mirt_scene_build_device(gpu.h, *args, p(out)) == E_INVALID, args[1:]
        assert L.mirt_last_error().decode() == "mirt_scene_build_device: invalid arguments"
    assert not out.view(np.uint8).any()
    with pytest.raises(mirt.MirtError, match="mirt_scene_build_device: invalid arguments"):
        gpu.build_scene(s, 0, 9)


def test_upload_device_rejects_malformed_trees(gpu, mirt):
    """test_probe_rejects_malformed_tree's trees: same messages, own prefix."""
    abi = mirt.abi
    L, p = mirt.load(), abi.ptr
    s = mirt.create_random_spheres(3, 1)
    bad = np.array([gen._node(-1, 3), gen._node(0, 2), gen._node(7, 3)], abi.NODE)   # sphere 7 of 3
    assert L.mirt_scene_upload_flat_device(gpu.h, p(s), 3, p(bad), 3) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_upload_flat_device: malformed node 2 (sphere 7, skip 3)"
    assert L.mirt_scene_layout(p(s), 3, p(bad), 3, 0, None, 0, None) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_layout: malformed node 2 (sphere 7, skip 3)"
    with pytest.raises(mirt.MirtError, match="mirt_scene_upload_flat_device: malformed node 2"):
        gpu.upload_device(s, bad)
    one_child = np.array([gen._node(-1, 2), gen._node(0, 2)], abi.NODE)
    assert L.mirt_scene_upload_flat_device(gpu.h, p(s), 3, p(one_child), 2) == E_INVALID
    msg = L.mirt_last_error().decode()
    assert L.mirt_scene_layout(p(s), 3, p(one_child), 2, 0, None, 0, None) == E_INVALID
    assert msg == L.mirt_last_error().decode().replace("mirt_scene_layout", "mirt_scene_upload_flat_device")
    assert L.mirt_scene_upload_flat_device(gpu.h, None, 3, None, 0) == E_INVALID        # spheres missing
    assert L.mirt_scene_upload_flat_device(None, p(s), 3, None, 0) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_upload_flat_device: null context"


def test_resident_layout_errors(gpu, mirt, small):
    abi = mirt.abi
    L = mirt.load()
    raw = abi.SceneLayoutInfo()
    with mirt.Renderer(0) as fresh:
        assert L.mirt_scene_resident_layout(fresh.h, 0, None, 0, C.byref(raw)) == E_NOSCENE
    assert L.mirt_scene_resident_layout(None, 0, None, 0, None) == E_INVALID
    s, t = small["render_100_1_post"], small["render_100_1_tree"]
    gpu.upload_device(s, t)
    assert L.mirt_scene_resident_layout(gpu.h, 99, None, 0, None) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_resident_layout: unknown part 99"
    info, parts = mirt.scene_layout(s, t)
    for part, (name, dtype) in enumerate(abi.LAYOUT_PARTS):
        want = parts[name]
        buf = np.full(want.nbytes + 16, 0xAB, np.uint8)
        raw = abi.SceneLayoutInfo()
        assert L.mirt_scene_resident_layout(gpu.h, part, abi.ptr(buf), want.nbytes - 1, C.byref(raw)) == want.nbytes
        assert (buf == 0xAB).all(), name
        assert raw.num_pnodes == info["num_pnodes"] and raw.leaf_box_off == info["leaf_box_off"]
        assert L.mirt_scene_resident_layout(gpu.h, part, abi.ptr(buf), want.nbytes, None) == want.nbytes
        assert buf[:want.nbytes].tobytes() == want.tobytes() and (buf[want.nbytes:] == 0xAB).all(), name

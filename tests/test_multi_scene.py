"""mirt_multi_scene_build_device / _refit_device / _update_device
(csrc/multi.hip): the single-context calls run once per device
on the scene all the object's contexts of that device share, without waiting
for the launches in flight. Every comparison is exact. One device here: the
loop over distinct devices is not exercised."""
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
W, H = 160, 90
E_INVALID, E_NOSCENE = -1, -3
QFLOATS = ("inner_area", "leaf_area", "overhead", "cost")
# devices, lanes, flags -> owned contexts
OBJECTS = {
    "1x1": dict(devices=[0], lanes=1),
    "1x3": dict(devices=[0], lanes=3),
    "3x2": dict(devices=[0, 0, 0], lanes=2),
    "ahead": dict(devices=[0], lanes=2, queue_ahead=True),
    "direct": dict(devices=[0, 0], host_direct=True),
}


def owned(kw):
    return len(kw["devices"]) * kw.get("lanes", 1)


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def dbits(x):
    return struct.pack("<d", x)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def moved(s, sigma, seed):
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(F4)
    out["radius"] *= r.uniform(0.5, 1.5, len(s)).astype(F4)
    return out


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


def check_update(mirt, m, got, want, what, on_device=1):
    reordered, perm, res = got
    assert res["on_device"] == on_device, what
    assert res["rebuilt"] == want["rebuilt"], (what, res, want["decay"])
    for k in ("base_cost", "cost", "decay"):
        assert dbits(res[k]) == dbits(want[k]), f"{what}: {k} is {res[k]!r}, the host has {want[k]!r}"
    assert_same_quality(res["installed"], want["installed"], what + ", installed")
    assert same(perm, want["perm"]), what
    assert same(reordered, want["spheres"]), what
    contexts = m.lanes // 2 if m.queue_ahead else m.lanes
    assert_same_layout(mirt, m.resident_layout(contexts - 1, m.size - 1),
                       mirt.scene_layout(want["spheres"], want["tree"]), what)


@pytest.fixture(scope="module")
def host(mirt):
    """One private context that renders the host's uploads: the reference frames."""
    r = mirt.Renderer(0)
    yield r
    r.close()


def host_frame(mirt, host, s, tree):
    host.upload(s, tree if isinstance(tree, mirt.Bvh) else mirt.Bvh(tree))
    return host.render_frame(mirt.default_camera(), W, H, depth=5, seed=1)


def frame(m, mirt):
    return m.render_frame(mirt.default_camera(), W, H, depth=5, seed=1)


@pytest.mark.parametrize("name", list(OBJECTS))
@pytest.mark.parametrize("n", [1, 65, 257])
def test_build_refit_update(mirt, host, name, n):
    kw = OBJECTS[name]
    pre = mirt.create_random_spheres(n, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    with mirt.MultiRenderer(**kw) as m:
        # build
        assert same(m.build_scene(pre), s)
        ids = m.scene_ids()
        assert len(ids) == 1 and ids[0] != 0
        want = host_frame(mirt, host, s, b)
        assert same(frame(m, mirt), want)
        with mirt.Renderer(0) as single:
            single.build_scene(pre)
            assert same(single.render_frame(mirt.default_camera(), W, H, depth=5, seed=1), want)
        # refit
        s2 = moved(s, 0.5, n)
        tree2 = mirt.refit_bvh(b, s2)
        m.refit_scene(s2)
        assert len(m.scene_ids()) == 1 and m.scene_ids() != ids
        assert same(frame(m, mirt), host_frame(mirt, host, s2, tree2))
        # update, both branches (max_decay 1e-9: any tree is past it)
        nodes, cur = tree2.nodes, s2
        base = mirt.bvh_quality(nodes, n)["cost"]       # a plain refit left no base: the resident tree's cost
        for k, max_decay in enumerate((0.0, 1e-9)):
            s3 = moved(cur, 0.5, 100 + k)
            want = host_update(mirt, nodes, s3, 0, n, max_decay, base)
            assert want["rebuilt"] == int(max_decay > 0 and want["decay"] > max_decay)
            check_update(mirt, m, m.update_scene(s3, 0, n, max_decay), want, f"{name} {n} max {max_decay}")
            assert same(frame(m, mirt), host_frame(mirt, host, want["spheres"], want["tree"]))
            nodes, cur = want["tree"], want["spheres"]
            base = want["installed"]["cost"] if want["rebuilt"] else base
            assert len(m.scene_ids()) == 1


def test_the_rebuild_branch_is_taken(mirt):
    """Not vacuous: at 257 spheres max_decay 1e-9 rebuilds (cost / base > 1e-9)."""
    s = mirt.create_random_spheres(257, 11)
    b = mirt.build_bvh(s)
    base = mirt.bvh_quality(b, 257)["cost"]
    assert host_update(mirt, b.nodes, moved(s, 0.5, 1), 0, 257, 1e-9, base)["rebuilt"] == 1


def test_4097_through_three_ranks(mirt, host):
    pre = mirt.create_random_spheres(4097, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    with mirt.MultiRenderer([0, 0, 0], lanes=2) as m:
        assert same(m.build_scene(pre), s)
        s2 = moved(s, 0.5, 7)
        base = mirt.bvh_quality(b, 4097)["cost"]
        want = host_update(mirt, b.nodes, s2, 0, 4097, 1e-9, base)
        assert want["rebuilt"] == 1
        check_update(mirt, m, m.update_scene(s2, 0, 4097, 1e-9), want, "4097")
        assert same(frame(m, mirt), host_frame(mirt, host, want["spheres"], want["tree"]))


def test_launches_in_flight_across_a_refit(mirt, host):
    """Three launches wait behind bounded 150 ms stalls of lane 0's context
    while the scene is refit: they deliver the old scene, the next three the
    new one. (The refit's own kernels queue behind lane 0's launch.)"""
    s = mirt.create_random_spheres(257, 11)
    b = mirt.build_bvh(s)
    s2 = moved(s, 3.0, 8)
    want_old = host_frame(mirt, host, s, mirt.refit_bvh(b, s))
    want_new = host_frame(mirt, host, s2, mirt.refit_bvh(b, s2))
    assert not same(want_old, want_new)
    cam, fd = mirt.default_camera(), mirt.frame_desc(W, H, depth=5, seed=1)
    bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(6)]
    try:
        with mirt.MultiRenderer([0], lanes=3) as m:
            m.upload(s, b)
            m.refit_scene(s)                               # the contexts share from here on: later calls wait for no lane
            assert len(m.scene_ids()) == 1
            assert mirt.load().mirt_set_option(m.ctx(0, 0), mirt.abi.OPT_DEBUG_STALL_MS, 150) == 0
            for k in range(3):
                m.render_frame_async(cam, fd, bufs[k])
            m.refit_scene(s2)
            assert mirt.load().mirt_set_option(m.ctx(0, 0), mirt.abi.OPT_DEBUG_STALL_MS, 0) == 0
            for k in range(3, 6):
                m.render_frame_async(cam, fd, bufs[k])
            m.wait()
            for k in range(3):
                assert same(bufs[k].array, want_old), k
            for k in range(3, 6):
                assert same(bufs[k].array, want_new), k
    finally:
        for hb in bufs:
            hb.close()


@pytest.mark.parametrize("name", ["3x2", "ahead"])
def test_upload_after_sharing(mirt, host, name):
    kw = OBJECTS[name]
    pre = mirt.create_random_spheres(257, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    s2 = moved(s, 0.5, 3)
    tree2 = mirt.refit_bvh(b, s2)
    with mirt.MultiRenderer(**kw) as m:
        m.build_scene(pre)
        assert len(m.scene_ids()) == 1
        m.upload(s2, tree2)
        assert len(m.scene_ids()) == owned(kw)
        assert same(frame(m, mirt), host_frame(mirt, host, s2, tree2))
        s3 = moved(s2, 0.5, 4)
        m.refit_scene(s3)
        assert len(m.scene_ids()) == 1
        assert same(frame(m, mirt), host_frame(mirt, host, s3, mirt.refit_bvh(tree2, s3)))


@pytest.mark.parametrize("bad", ["nan", "negzero"])
def test_declined_inputs_through_the_object(mirt, host, bad):
    pre = mirt.create_random_spheres(65, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    s2 = moved(s, 0.5, 5)
    if bad == "nan":
        s2["radius"][7] = np.nan
    else:
        s2["center"][7] = [-0.0, 1.0, 2.0]
        s2["radius"][7] = 0.0                              # the box coordinate is -0.0
    b0 = mirt.refit_bvh(b, s)                              # what refit_scene(s) leaves resident
    base = mirt.bvh_quality(b0, 65)["cost"]
    with mirt.MultiRenderer([0, 0], lanes=2) as m:
        m.build_scene(pre)
        for max_decay in (0.0, 1e-9):
            m.refit_scene(s)                               # back to the first spheres, and no base
            want = host_update(mirt, b0.nodes, s2, 0, 65, max_decay, base)
            check_update(mirt, m, m.update_scene(s2, 0, 65, max_decay), want, f"{bad} {max_decay}", on_device=0)
            assert len(m.scene_ids()) == 1
            assert same(frame(m, mirt), host_frame(mirt, host, want["spheres"], want["tree"]))


def test_errors(mirt, host):
    L, p = mirt.load(), mirt.abi.ptr
    pre = mirt.create_random_spheres(65, 11)
    s = pre.copy()
    b = mirt.build_bvh(s)
    with mirt.MultiRenderer([0, 0], lanes=2) as m:
        assert L.mirt_multi_scene_refit_device(m.h, p(s), 65, 65) == E_NOSCENE
        assert L.mirt_multi_scene_update_device(m.h, p(s), 65, 0, 65, 0.0, None, None, None) == E_NOSCENE
        assert m.scene_ids() == [0] and not m.failed
        m.build_scene(pre)
        want = host_frame(mirt, host, s, b)
        ids = m.scene_ids()
        assert L.mirt_multi_scene_refit_device(m.h, p(s), 64, 64) == E_INVALID
        assert "64 spheres for a resident scene of 65" in L.mirt_last_error().decode()
        assert L.mirt_multi_scene_update_device(m.h, p(s), 64, 0, 64, 0.0, None, None, None) == E_INVALID
        assert m.scene_ids() == ids and not m.failed
        assert same(frame(m, mirt), want)

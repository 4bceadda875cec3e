"""mirt_ctx_share_scene (csrc/render.hip): the contexts of a
group render one resident scene, installs and reads through any member concern
that scene, and a frame in flight finishes on the scene it was enqueued on.
Every comparison is exact."""
import importlib.util
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


def assert_same_layout(mirt, got, want, what=""):
    ginfo, gparts = got
    winfo, wparts = want
    for k, v in winfo.items():
        g = ginfo[k]
        ok = fbits(g) == fbits(v) if k in gen.FLOATS else int(g) == int(v)
        assert ok, f"{what}: info.{k} is {g!r}, the host has {v!r}"
    for name, _ in mirt.abi.LAYOUT_PARTS:
        assert gparts[name].tobytes() == wparts[name].tobytes(), f"{what}: part {name} differs"


def frame(r, mirt):
    return r.render_frame(mirt.default_camera(), W, H, depth=5, seed=1)


def host_frame(mirt, s, tree):
    """The frame of a private context holding the host upload of (s, tree)."""
    with mirt.Renderer(0) as host:
        host.upload(s, tree if isinstance(tree, mirt.Bvh) else mirt.Bvh(tree))
        return frame(host, mirt)


@pytest.mark.parametrize("n", [1, 65, 257, 4097])
def test_shared_frames_and_ids(mirt, n):
    pre = mirt.create_random_spheres(n, 3)
    s = pre.copy()
    b = mirt.build_bvh(s)
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B, mirt.Renderer(0) as third:
        assert A.scene_id() == 0 and B.scene_id() == 0
        assert same(A.build_scene(pre), s)
        B.share_scene(A)
        third.upload(s, b)
        want = frame(third, mirt)
        assert same(frame(A, mirt), want) and same(frame(B, mirt), want)
        assert A.scene_id() == B.scene_id() != 0
        assert third.scene_id() not in (0, A.scene_id())
        B.share_scene(A)                                   # already so: nothing changes
        assert A.scene_id() == B.scene_id()


@pytest.mark.parametrize("n", [65, 257])
def test_installs_are_seen_by_all(mirt, n):
    pre = mirt.create_random_spheres(n, 4)
    s = pre.copy()
    b = mirt.build_bvh(s)
    s2 = moved(s, 0.5, n)
    want = mirt.scene_layout(s2, mirt.refit_bvh(b, s2))
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
        A.build_scene(pre)
        B.share_scene(A)
        before = A.scene_id()
        B.refit_scene(s2)                                  # through the follower
        assert A.scene_id() == B.scene_id() == before + 1  # one install, one new id (nothing else installs here)
        assert_same_layout(mirt, A.resident_layout(), want, "through the owner")
        assert_same_layout(mirt, B.resident_layout(), want, "through the follower")
        assert B.last_refit_stats()["on_device"] == 1      # statistics stay with the context that ran the call
        with pytest.raises(mirt.MirtError):
            A.last_refit_stats()


def test_frame_in_flight_keeps_its_scene(mirt):
    """B's frame waits behind a bounded 200 ms stall while A refits the group's
    scene: the frame reads the replaced arrays, which must still be there."""
    s = mirt.create_random_spheres(257, 11)
    b = mirt.build_bvh(s)
    s2 = moved(s, 3.0, 8)
    want_old = host_frame(mirt, s, b)
    want_new = host_frame(mirt, s2, mirt.refit_bvh(b, s2))
    assert not same(want_old, want_new)
    cam, fd = mirt.default_camera(), mirt.frame_desc(W, H, depth=5, seed=1)
    bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(2)]
    try:
        with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
            A.upload(s, b)
            B.share_scene(A)
            B.set_option(mirt.abi.OPT_DEBUG_STALL_MS, 200)
            B.render_frame_async(cam, fd, bufs[0])
            A.refit_scene(s2)
            B.wait()
            assert same(bufs[0].array, want_old)
            B.set_option(mirt.abi.OPT_DEBUG_STALL_MS, 0)
            B.render_frame_async(cam, fd, bufs[1])
            B.wait()
            assert same(bufs[1].array, want_new)
            A.refit_scene(s)                               # a later install looks at the retired scene
            assert same(frame(B, mirt), want_old)
    finally:
        for hb in bufs:
            hb.close()


def test_base_cost_belongs_to_the_slot(mirt):
    s = mirt.create_random_spheres(257, 11)
    nodes = mirt.build_bvh(s).nodes
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
        A.upload(s, mirt.Bvh(nodes))
        B.share_scene(A)
        s1, _, first = A.update_scene(moved(s, 10.0, 257), 0, len(s), 1.1)
        _, _, second = B.update_scene(moved(s1, 0.5, 2), 0, len(s), 0.0)
        assert first["rebuilt"] == 1 and second["rebuilt"] == 0
        assert dbits(first["installed"]["cost"]) != dbits(first["base_cost"])
        assert dbits(second["base_cost"]) == dbits(first["installed"]["cost"])


def test_leaving_and_destroying(mirt):
    s = mirt.create_random_spheres(257, 11)
    b = mirt.build_bvh(s)
    s2 = moved(s, 3.0, 9)
    want_old = host_frame(mirt, s, b)
    want_new = host_frame(mirt, s2, mirt.refit_bvh(b, s2))
    A, B, D = mirt.Renderer(0), mirt.Renderer(0), mirt.Renderer(0)
    try:
        A.upload(s, b)
        B.share_scene(A)
        D.share_scene(A)
        B.share_scene(None)                                # leaves with the scene
        assert B.scene_id() == A.scene_id()
        A.refit_scene(s2)
        assert B.scene_id() != A.scene_id() == D.scene_id()
        assert same(frame(B, mirt), want_old)
        assert same(frame(A, mirt), want_new) and same(frame(D, mirt), want_new)
        A.close()                                          # the owner goes: its follower keeps the scene
        assert same(frame(D, mirt), want_new)
        assert same(frame(B, mirt), want_old)
        D.refit_scene(s)
        assert same(frame(D, mirt), want_old)
    finally:
        for r in (A, B, D):
            r.close()


def test_options_stay_per_context(mirt):
    s = mirt.create_random_spheres(257, 11)
    b = mirt.build_bvh(s)
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
        A.upload(s, b)
        B.share_scene(A)
        B.set_option(mirt.abi.OPT_PRUNE, 0)
        assert A.get_option(mirt.abi.OPT_PRUNE) == 1 and B.get_option(mirt.abi.OPT_PRUNE) == 0
        assert same(frame(A, mirt), frame(B, mirt))


def test_sharing_without_a_scene(mirt):
    s = mirt.create_random_spheres(65, 11)
    b = mirt.build_bvh(s)
    with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
        B.share_scene(A)
        for r in (A, B):
            with pytest.raises(mirt.MirtError, match=r"\(-3\).*no scene uploaded"):
                frame(r, mirt)
        B.upload(s, b)                                     # either member installs for both
        assert A.scene_id() == B.scene_id() != 0
        assert same(frame(A, mirt), host_frame(mirt, s, b))
    assert mirt.load().mirt_ctx_share_scene(None, None) == -1
    assert mirt.load().mirt_ctx_scene_id(None) == 0


def test_other_device_is_invalid(mirt):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    with mirt.Renderer(0) as A, mirt.Renderer(1) as B:
        with pytest.raises(mirt.MirtError, match=r"\(-1\).*devices"):
            B.share_scene(A)

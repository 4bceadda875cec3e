"""The reprojection with a motion on the GPU, and the history that survives a
moved scene: mirt_reproject_motion_device and mirt_reproject_motion equal
mirt_reproject_motion_host byte for byte on every case and parameter set of
tests/reproject_motion_cases.py (which the host tests hold against the numpy
restatement), with canaries around every device output, the outputs one at a
time, d_out aliasing d_rgba and a torch stream; under MIRT_OPT_HISTORY_MOTION 1
mirt_render_frame_reprojected across refits, updates and rebuilds equals
mirt_render_frame_planes composed with mirt_reproject_motion_host, fed the
resident geo arrays before and after each install and the returned
permutation; and the history empties whenever the link does not lead from
exactly its scene to exactly the resident one."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_cases as dc
import reproject_cases as rc
import reproject_motion_cases as mc
import test_planes_cases as cases
from test_planes_gpu import upload
from test_reproject_gpu import CANARY, PAD, Device, frame_kw

pytestmark = pytest.mark.gpu

W, H, N = mc.W, mc.H, mc.N


@functools.lru_cache(maxsize=None)
def host(name, params):
    """mirt_reproject_motion_host's (hist_out, out, out_rgb) of a case, computed once."""
    hist, out, rgb = mc.host(mc.mirt.load(), mc.case(name), params)
    for a in (hist, out, rgb):
        a.setflags(write=False)
    return hist, out, rgb


def prev_of(c):
    return (c["cam_prev"], c["hist"], c["t_prev"], c["sphere_prev"])


def motion_of(c):
    return (c["geo"], c["geo_prev"], c["prev_index"])


class MotionDevice(Device):
    """A case and its motion in device memory, outputs between canaries."""

    def __init__(self, c):
        super().__init__(c)
        torch = self.torch
        up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(self.rgba.device)   # noqa: E731
        self.geo, self.geo_prev, self.idx = up(c["geo"]), up(c["geo_prev"]), up(c["prev_index"])
        torch.cuda.synchronize()

    def run(self, gpu, params, stream=None, alias=False, want_out=True, want_rgb=True):
        """mirt_reproject_motion_device; returns (hist_out, out, out_rgb) from the device (None if not asked for)."""
        c, p = self.c, rc.params_struct(params)
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None   # noqa: E731
        mo = mc.abi.SphereMotion(self.geo.data_ptr(), self.geo_prev.data_ptr(),
                                 self.idx.data_ptr() if self.idx is not None else None, len(c["geo"]),
                                 len(c["geo_prev"]))
        d_out = (dp(self.rgba) if alias else dp(self.out, PAD)) if want_out else None
        r = gpu.L.mirt_reproject_motion_device(gpu.h, c["width"], c["height"], C.byref(c["cam"]),
                                               C.byref(c["cam_prev"]), dp(self.rgba), dp(self.t), dp(self.sphere),
                                               dp(self.hist), dp(self.t_prev), dp(self.sphere_prev), C.byref(p),
                                               dp(self.ho, PAD), d_out, dp(self.rgb, PAD) if want_rgb else None,
                                               C.c_void_p(stream or 0), C.byref(mo))
        assert r == 0, gpu.L.mirt_last_error().decode()
        self.torch.cuda.synchronize()
        h, w = c["height"], c["width"]
        hist = self.ho[PAD:-PAD].cpu().numpy().view(rc.abi.HISTORY).reshape(h, w)
        out_t = (self.rgba if alias else self.out[PAD:-PAD]) if want_out else None
        out = out_t.cpu().numpy().reshape(h, w, 4) if want_out else None
        rgb = self.rgb[PAD:-PAD].cpu().numpy().view(np.float32).reshape(h, w, 3) if want_rgb else None
        for buf in (self.ho, self.out, self.rgb):
            edge = buf.cpu().numpy()
            assert (edge[:PAD] == CANARY).all() and (edge[-PAD:] == CANARY).all(), "a canary was overwritten"
        return hist, out, rgb


@pytest.mark.parametrize("name", mc.CASES)
def test_both_forms_equal_the_host_form(gpu, name):
    c = mc.case(name)
    d = MotionDevice(c)
    assert {p[1] for p in mc.PARAMS} == {1, 4}
    for params in mc.PARAMS:
        want = host(name, params)
        got = gpu.reproject(c["cam"], c["rgba"], c["t"], c["sphere"], prev=prev_of(c), params=params, rgb=True,
                            motion=motion_of(c))
        for g, w, what in zip(got, want, ("hist_out", "out", "out_rgb")):
            mc.same_bytes(g, w, f"mirt_reproject_motion {name} {params} {what}")
        got = d.run(gpu, params)
        for g, w, what in zip(got, want, ("hist_out", "out", "out_rgb")):
            mc.same_bytes(g, w, f"mirt_reproject_motion_device {name} {params} {what}")


def test_outputs_one_at_a_time_aliasing_and_a_stream(gpu):
    import torch
    s = torch.cuda.Stream()
    for name in ("diffused_right", "permuted_A", "range_9_3", "radius_9_3", "m_70_5", "m_1_7"):
        c = mc.case(name)
        for params in mc.PARAMS[:2]:
            want_hist, want_out, want_rgb = host(name, params)
            d = MotionDevice(c)
            hist, out, rgb = d.run(gpu, params, want_rgb=False)
            mc.same_bytes(hist, want_hist, f"{name} {params} hist_out, out alone")
            mc.same_bytes(out, want_out, f"{name} {params} out alone")
            assert (d.rgb.cpu().numpy() == CANARY).all()
            d = MotionDevice(c)
            hist, out, rgb = d.run(gpu, params, want_out=False)
            mc.same_bytes(rgb, want_rgb, f"{name} {params} out_rgb alone")
            assert (d.out.cpu().numpy() == CANARY).all()
            d = MotionDevice(c)
            hist, out, rgb = d.run(gpu, params, want_out=False, want_rgb=False)
            mc.same_bytes(hist, want_hist, f"{name} {params} hist_out alone")
            assert (d.out.cpu().numpy() == CANARY).all() and (d.rgb.cpu().numpy() == CANARY).all()
            d = MotionDevice(c)
            hist, out, rgb = d.run(gpu, params, stream=s.cuda_stream)
            mc.same_bytes(hist, want_hist, f"{name} {params} on a torch stream, hist_out")
            mc.same_bytes(out, want_out, f"{name} {params} on a torch stream")
            mc.same_bytes(rgb, want_rgb, f"{name} {params} on a torch stream, out_rgb")
            hist, out, _ = d.run(gpu, params)   # back on the default stream: behind the other stream's launch
            mc.same_bytes(hist, want_hist, f"{name} {params} back on the default stream, hist_out")
            mc.same_bytes(out, want_out, f"{name} {params} back on the default stream")
            d = MotionDevice(c)
            hist, out, rgb = d.run(gpu, params, alias=True)
            mc.same_bytes(hist, want_hist, f"{name} {params} d_out aliasing d_rgba, hist_out")
            mc.same_bytes(out, want_out, f"{name} {params} d_out aliasing d_rgba")
            mc.same_bytes(rgb, want_rgb, f"{name} {params} aliasing, out_rgb")
            assert (d.out.cpu().numpy() == CANARY).all()
    # the binding's device form: tensors in, tensors out
    c = mc.case("permuted_right")
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731
    records = np.array(c["hist"]).view(np.float32).reshape(H, W, 4)   # the same 16 bytes per pixel
    prev = (c["cam_prev"], up(records), up(c["t_prev"]), up(c["sphere_prev"]))
    want_hist, want_out, want_rgb = host("permuted_right", rc.DEFAULT)
    hist, out, rgb = gpu.reproject(c["cam"], up(c["rgba"]), up(c["t"]), up(c["sphere"]), prev=prev, rgb=True,
                                   motion=(up(c["geo"]), up(c["geo_prev"]), up(c["prev_index"])))
    torch.cuda.synchronize()
    mc.same_bytes(hist.cpu().numpy().view(rc.abi.HISTORY).reshape(H, W), want_hist, "Renderer.reproject on tensors")
    mc.same_bytes(out.cpu().numpy(), want_out, "Renderer.reproject on tensors, out")
    mc.same_bytes(rgb.cpu().numpy(), want_rgb, "Renderer.reproject on tensors, rgb")
    with pytest.raises(mc.mirt.MirtError, match="invalid arguments"):   # a motion without a previous frame
        gpu.reproject(c["cam"], c["rgba"], c["t"], c["sphere"], motion=motion_of(c))
    with pytest.raises(mc.mirt.MirtError, match="invalid arguments"):   # no map, other counts
        gpu.reproject(c["cam"], c["rgba"], c["t"], c["sphere"], prev=prev_of(c),
                      motion=(c["geo"], c["geo_prev"][:-1], None))


# ---- the frame form

@contextlib.contextmanager
def history_motion(mirt, *renderers, value=1):
    try:
        for r in renderers:
            r.set_option(mirt.abi.OPT_HISTORY_MOTION, value)
        yield
    finally:
        for r in renderers:
            r.set_option(mirt.abi.OPT_HISTORY_MOTION, 0)


def geo_now(r):
    """The resident scene's spheres as the geo array holds them."""
    return np.ascontiguousarray(r.resident_layout()[1]["geo"][:N])


def cam_of(k):
    return rc.camera(f"path{k % 5}")


class Loop:
    """The animate loop on a ctx beside its host restatement: each frame is
    rendered twice, once by mirt_render_frame_planes for the host form's input
    and once by mirt_render_frame_reprojected."""

    def __init__(self, gpu, mirt, params=rc.DEFAULT):
        self.gpu, self.L, self.params = gpu, mirt.load(), params
        self.prev, self.k, self.frames = None, 0, 0

    def frame(self, motion, what):
        """One frame. motion: None = the host loop starts over (no history), "plain" = the history is kept
        without a motion, else (geo, geo_prev, prev_index). Returns the ctx's stats."""
        gpu, k = self.gpu, self.k
        cam = cam_of(k)
        raw, pl = gpu.render_frame_planes(cam, W, H, planes=("t", "sphere"), **frame_kw(k))
        prev = None if motion is None else self.prev
        hist, want = mc.host_step(self.L, cam, raw, pl["t"], pl["sphere"], prev, self.params,
                                  None if motion in (None, "plain") else motion)
        out, raw2 = gpu.render_frame_reprojected(cam, W, H, params=self.params, raw=True, **frame_kw(k))
        mc.same_bytes(raw2, raw, f"{what}: the one-sample frame")
        mc.same_bytes(out, want, f"{what}: the display")
        mc.same_bytes(gpu.history_read(), hist, f"{what}: the records")
        self.prev, self.k = (cam, hist, pl["t"], pl["sphere"]), k + 1
        self.frames = 1 if prev is None else self.frames + 1
        st = gpu.history_stats()
        assert st["frames"] == self.frames and st["scene_id"] == gpu.scene_id(), (what, st)
        assert st["reused"] == int((hist["n"] > 1).sum()) and st["reused"] + st["fresh"] + st["sky"] == W * H, (what, st)
        assert (st["reused"] > 0) == (prev is not None), (what, st)
        return st


def test_the_animate_loop(gpu, mirt):
    """A frame; an update that refits; an update that rebuilds; a refit. The
    history is carried over every one of them."""
    spheres = upload(gpu, mirt, N)
    gpu.history_reset()
    with history_motion(mirt, gpu):
        assert gpu.get_option(mirt.abi.OPT_HISTORY_MOTION) == 1
        hm = gpu.history_motion()
        assert (hm["from_scene_id"], hm["to_scene_id"], hm["rebuilt"], hm["carried"]) == (0, 0, 0, 0), hm
        loop = Loop(gpu, mirt)
        loop.frame(None, "the first frame")
        loop.frame("plain", "a second frame of the same scene")
        held = spheres
        for step, (call, max_decay) in enumerate([("update", 0.0), ("update", 1e-3), ("refit", None), ("update", 1e-3),
                                                  ("update", 0.0)]):
            what = f"step {step}: {call} {max_decay}"
            before, sid = geo_now(gpu), gpu.scene_id()
            moved = mc.diffused(held, mc.SIGMA, 40 + step)
            if call == "update":
                held, perm, res = gpu.update_scene(moved, 0, N, max_decay)
                assert res["on_device"] == 1 and res["rebuilt"] == int(max_decay > 0), (what, res)
                rebuilt = res["rebuilt"]
                if rebuilt:
                    assert (perm != np.arange(N)).any()
                    mc.same_bytes(held, moved[perm], what + ": reordered")
            else:
                gpu.refit_scene(moved)
                assert gpu.last_refit_stats()["on_device"] == 1
                held, perm, rebuilt = moved, None, 0
            after = geo_now(gpu)
            mc.same_bytes(after, mc.geo_of(held), f"{what}: the resident geo array")
            hm = gpu.history_motion()
            assert (hm["from_scene_id"], hm["to_scene_id"], hm["rebuilt"]) == (sid, gpu.scene_id(), rebuilt), (what, hm)
            assert hm["bytes"] >= 2 * 20 * N, (what, hm)   # (carried still speaks of the frame before the install)
            frames = loop.frames
            st = loop.frame((after, before, perm if rebuilt else None), what)
            assert st["frames"] == frames + 1, (what, st)
            hm2 = gpu.history_motion()
            assert hm2["carried"] == 1 and dict(hm2, carried=0) == dict(hm, carried=0), (what, hm2)
            if step == 1:   # the next frame of the same scene is a plain one again
                loop.frame("plain", what + ", a second frame")
                assert gpu.history_motion()["carried"] == 0
                loop.frame("plain", what + ", a third frame")
        assert loop.frames == 9
    assert gpu.get_option(mirt.abi.OPT_HISTORY_MOTION) == 0
    # a plain frame afterwards still matches its golden bytes
    upload(gpu, mirt, N)
    rc.same_bytes(gpu.render_frame(cases.camera("A"), W, H, depth=5, seed=1, sample=1), dc.oracle_frame(1),
                  "a plain frame afterwards")
    gpu.history_reset()


def test_with_the_option_off_every_install_starts_over(mirt):
    """On a ctx of its own, which never had the option on: no link, and no memory held for one."""
    with mirt.Renderer(0) as r:
        spheres = upload(r, mirt, N)
        assert r.get_option(mirt.abi.OPT_HISTORY_MOTION) == 0
        loop = Loop(r, mirt)
        loop.frame(None, "the first frame")
        held = spheres
        for step, (call, max_decay) in enumerate([("update", 0.0), ("update", 1e-3), ("refit", None)]):
            moved = mc.diffused(held, mc.SIGMA, 50 + step)
            if call == "update":
                held, _, _ = r.update_scene(moved, 0, N, max_decay)
            else:
                r.refit_scene(moved)
                held = moved
            hm = r.history_motion()
            assert (hm["from_scene_id"], hm["to_scene_id"], hm["rebuilt"], hm["bytes"]) == (0, 0, 0, 0), hm
            st = loop.frame(None, f"option 0, step {step}")
            assert st["frames"] == 1 and st["reused"] == 0 and r.history_motion()["carried"] == 0
            loop.frame("plain", f"option 0, step {step}, a second frame")


def test_the_history_empties_when_the_link_does_not_fit(gpu, mirt):
    spheres = upload(gpu, mirt, N)
    gpu.history_reset()
    with history_motion(mirt, gpu):
        loop = Loop(gpu, mirt)
        loop.frame(None, "the first frame")
        # two installs between frames: the link starts at a scene no frame was rendered of
        s1, _, _ = gpu.update_scene(mc.diffused(spheres, mc.SIGMA, 60), 0, N, 0.0)
        s2, _, _ = gpu.update_scene(mc.diffused(s1, mc.SIGMA, 61), 0, N, 0.0)
        assert gpu.history_motion()["to_scene_id"] == gpu.scene_id()
        st = loop.frame(None, "after two installs")
        assert st["frames"] == 1 and gpu.history_motion()["carried"] == 0
        # an upload clears the link
        loop.frame("plain", "a second frame")
        held = upload(gpu, mirt, N)
        hm = gpu.history_motion()
        assert (hm["from_scene_id"], hm["to_scene_id"]) == (0, 0) and hm["bytes"] > 0, hm
        assert loop.frame(None, "after an upload")["frames"] == 1
        # and so does mirt_scene_build_device
        resident = gpu.build_scene(held)
        assert gpu.history_motion()["to_scene_id"] == 0
        assert loop.frame(None, "after a device build")["frames"] == 1
        # mirt_history_reset and another width empty it although the link fits
        before, sid = geo_now(gpu), gpu.scene_id()
        s3, _, _ = gpu.update_scene(mc.diffused(resident, mc.SIGMA, 62), 0, N, 0.0)
        assert gpu.history_motion()["from_scene_id"] == sid
        gpu.history_reset()
        assert loop.frame(None, "after mirt_history_reset")["frames"] == 1
        sid = gpu.scene_id()
        gpu.update_scene(mc.diffused(s3, mc.SIGMA, 63), 0, N, 0.0)
        assert gpu.history_motion()["from_scene_id"] == sid
        out = gpu.render_frame_reprojected(cam_of(0), W - 3, H, **frame_kw(0))
        st = gpu.history_stats()
        assert (st["frames"], st["reused"], st["width"]) == (1, 0, W - 3) and out.shape == (H, W - 3, 4), st
        assert gpu.history_motion()["carried"] == 0
    gpu.history_reset()


def test_a_failed_update_leaves_the_link(gpu, mirt):
    spheres = upload(gpu, mirt, N)
    gpu.history_reset()
    with history_motion(mirt, gpu):
        loop = Loop(gpu, mirt)
        loop.frame(None, "the first frame")
        before = geo_now(gpu)
        held, _, _ = gpu.update_scene(mc.diffused(spheres, mc.SIGMA, 70), 0, N, 0.0)
        hm, sid = gpu.history_motion(), gpu.scene_id()
        with pytest.raises(mirt.MirtError, match="999 spheres for a resident scene of 1000"):
            gpu.update_scene(held[:N - 1], 0, N - 1, 0.0)
        with pytest.raises(mirt.MirtError, match="invalid arguments"):
            gpu.update_scene(held, 0, N + 1, 1.1)
        with pytest.raises(mirt.MirtError):
            gpu.refit_scene(held[:N - 1])
        assert gpu.history_motion() == hm and gpu.scene_id() == sid
        st = loop.frame((geo_now(gpu), before, None), "after the refused calls")
        assert st["frames"] == 2 and gpu.history_motion()["carried"] == 1
    gpu.history_reset()


@pytest.mark.parametrize("call", ["update", "rebuild", "refit"])
def test_negative_zero_takes_the_host_path_and_is_carried(gpu, mirt, call):
    spheres = upload(gpu, mirt, N)
    gpu.history_reset()
    with history_motion(mirt, gpu):
        loop = Loop(gpu, mirt)
        loop.frame(None, "the first frame")
        before, sid = geo_now(gpu), gpu.scene_id()
        moved = mc.diffused(spheres, mc.SIGMA, 80)
        moved["center"][5] = [-0.0, 1.0, 2.0]
        moved["radius"][5] = 0.0
        perm = None
        if call == "refit":
            gpu.refit_scene(moved)
            assert gpu.last_refit_stats()["on_device"] == 0
            held = moved
        else:
            held, perm, res = gpu.update_scene(moved, 0, N, 1e-3 if call == "rebuild" else 0.0)
            assert res["on_device"] == 0 and res["rebuilt"] == int(call == "rebuild"), res
        hm = gpu.history_motion()
        assert (hm["from_scene_id"], hm["to_scene_id"], hm["rebuilt"]) == (sid, gpu.scene_id(), int(call == "rebuild"))
        after = geo_now(gpu)
        mc.same_bytes(after, mc.geo_of(held), "the resident geo array")
        st = loop.frame((after, before, perm if call == "rebuild" else None), f"-0.0, {call}")
        assert st["frames"] == 2 and gpu.history_motion()["carried"] == 1
    gpu.history_reset()


@pytest.mark.parametrize("installer_option", [1, 0])
def test_a_group_member_installs(gpu, mirt, installer_option):
    """Two ctxs share the scene. With the option on both, one installs and the
    other carries; an install by a member with the option at 0 empties it."""
    spheres = upload(gpu, mirt, N)
    gpu.history_reset()
    with mirt.Renderer(0) as other:
        other.share_scene(gpu)
        try:
            with history_motion(mirt, gpu), history_motion(mirt, other, value=installer_option):
                loop = Loop(gpu, mirt)
                loop.frame(None, "the first frame")
                before, sid = geo_now(gpu), gpu.scene_id()
                held, perm, res = other.update_scene(mc.diffused(spheres, mc.SIGMA, 90), 0, N, 1e-3)
                assert res["rebuilt"] == 1 and gpu.scene_id() == other.scene_id() != sid
                hm = gpu.history_motion()
                assert dict(hm, carried=0) == dict(other.history_motion(), carried=0)
                if installer_option:
                    assert (hm["from_scene_id"], hm["to_scene_id"], hm["rebuilt"]) == (sid, gpu.scene_id(), 1), hm
                    st = loop.frame((geo_now(gpu), before, perm), "the other member installed")
                    assert st["frames"] == 2 and gpu.history_motion()["carried"] == 1
                    assert other.history_motion()["carried"] == 0
                else:
                    assert (hm["from_scene_id"], hm["to_scene_id"]) == (0, 0), hm
                    st = loop.frame(None, "a member with the option at 0 installed")
                    assert st["frames"] == 1 and gpu.history_motion()["carried"] == 0
        finally:
            other.share_scene(None)
    gpu.history_reset()

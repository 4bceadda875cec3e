"""The moments reprojection and the variance-guided filter on the GPU:
mirt_reproject_moments_device / mirt_reproject_moments and
mirt_denoise_var_device / mirt_denoise_var equal their host forms byte for byte
on every case and parameter set of tests/vfilter_cases.py (which the host tests
hold against the numpy restatement), with canaries around every device output,
the outputs one at a time, a torch stream and back, d_out aliasing d_rgba, and
either pass kernel (MIRT_OPT_DENOISE_TILE); mirt_render_frame_reprojected_denoised
along a camera path equals mirt_render_frame_planes composed with the two host
forms frame by frame and leaves records, displays and accumulation buffer as
mirt_render_frame_reprojected does; its history empties when it must and
survives a refit or an update under MIRT_OPT_HISTORY_MOTION; a ctx that never
makes the call holds what it held."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_cases as dc
import reproject_cases as rc
import reproject_motion_cases as mc
import test_planes_cases as cases
import vfilter_cases as vc
from test_planes_gpu import options, upload

pytestmark = pytest.mark.gpu

W, H = rc.W, rc.H
CANARY, PAD = 0x5A, 256   # bytes around each device output
F32 = np.float32


def lib():
    return rc.mirt.load()


@functools.lru_cache(maxsize=None)
def host_moments(name, params):
    c, motion = vc.moment_case(name)
    got = vc.host_moments(lib(), c, params, vc.m2_prev_of(name), motion)
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def host_filter(name, params):
    got = vc.host(lib(), vc.case(name), params)
    for a in got:
        a.setflags(write=False)
    return got


def up(torch, a):
    return None if a is None else torch.from_numpy(np.array(a).view(np.uint8)).to(torch.device("cuda", 0))


def full(torch, nbytes):
    return torch.full((2 * PAD + nbytes,), CANARY, dtype=torch.uint8, device=torch.device("cuda", 0))


def canaries_hold(*bufs):
    for buf in bufs:
        edge = buf.cpu().numpy()
        assert (edge[:PAD] == CANARY).all() and (edge[-PAD:] == CANARY).all(), "a canary was overwritten"


def untouched(buf):
    return (buf.cpu().numpy() == CANARY).all()


dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None   # noqa: E731
ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731


class Moments:
    """A moments case in device memory, outputs between canaries."""

    def __init__(self, name):
        import torch
        self.torch = torch
        self.c, self.motion = vc.moment_case(name)
        c = self.c
        self.rgba, self.t, self.sphere = up(torch, c["rgba"]), up(torch, c["t"]), up(torch, c["sphere"])
        self.hist, self.t_prev, self.sphere_prev = up(torch, c["hist"]), up(torch, c["t_prev"]), up(torch, c["sphere_prev"])
        self.m2_prev = up(torch, vc.m2_prev_of(name))
        self.geo = self.geo_prev = self.idx = None
        if self.motion:
            self.geo, self.geo_prev, self.idx = up(torch, c["geo"]), up(torch, c["geo_prev"]), up(torch, c["prev_index"])
        n = c["width"] * c["height"]
        self.ho, self.out, self.rgb, self.m2 = full(torch, 16 * n), full(torch, 4 * n), full(torch, 12 * n), full(torch, 4 * n)
        torch.cuda.synchronize()

    def run(self, gpu, params, stream=None, alias=False, want_out=True, want_rgb=True):
        """mirt_reproject_moments_device: (hist_out, out, out_rgb, m2_out) from the device (None if not asked for)."""
        c, p = self.c, rc.params_struct(params)
        mo = None
        if self.motion:
            mo = rc.abi.SphereMotion(self.geo.data_ptr(), self.geo_prev.data_ptr(),
                                     self.idx.data_ptr() if self.idx is not None else None, len(c["geo"]),
                                     len(c["geo_prev"]))
        d_out = (dp(self.rgba) if alias else dp(self.out, PAD)) if want_out else None
        r = gpu.L.mirt_reproject_moments_device(gpu.h, c["width"], c["height"], ref(c["cam"]), ref(c["cam_prev"]),
                                                dp(self.rgba), dp(self.t), dp(self.sphere), dp(self.hist),
                                                dp(self.t_prev), dp(self.sphere_prev), C.byref(p), dp(self.ho, PAD),
                                                d_out, dp(self.rgb, PAD) if want_rgb else None,
                                                C.c_void_p(stream or 0), ref(mo), dp(self.m2_prev), dp(self.m2, PAD))
        assert r == 0, gpu.L.mirt_last_error().decode()
        self.torch.cuda.synchronize()
        h, w = c["height"], c["width"]
        hist = self.ho[PAD:-PAD].cpu().numpy().view(rc.abi.HISTORY).reshape(h, w)
        out_t = (self.rgba if alias else self.out[PAD:-PAD]) if want_out else None
        out = out_t.cpu().numpy().reshape(h, w, 4) if want_out else None
        rgb = self.rgb[PAD:-PAD].cpu().numpy().view(F32).reshape(h, w, 3) if want_rgb else None
        m2 = self.m2[PAD:-PAD].cpu().numpy().view(F32).reshape(h, w)
        canaries_hold(self.ho, self.out, self.rgb, self.m2)
        return hist, out, rgb, m2


NAMES4 = ("hist_out", "out", "out_rgb", "m2_out")


def prev_of(name):
    c, _ = vc.moment_case(name)
    if c["cam_prev"] is None:
        return None
    return (c["cam_prev"], c["hist"], c["t_prev"], c["sphere_prev"], vc.m2_prev_of(name))


def motion_of(name):
    c, motion = vc.moment_case(name)
    return (c["geo"], c["geo_prev"], c["prev_index"]) if motion else None


@pytest.mark.parametrize("name", vc.MOMENT_CASES)
def test_moments_both_forms_equal_the_host_form(gpu, name):
    c, _ = vc.moment_case(name)
    d = Moments(name)
    for params in c["params"]:
        want = host_moments(name, params)
        hist, out, rgb, m2 = gpu.reproject_moments(c["cam"], c["rgba"], c["t"], c["sphere"], prev=prev_of(name),
                                                   params=params, rgb=True, motion=motion_of(name))
        for g, w, what in zip((hist, out, rgb, m2), want, NAMES4):
            vc.same_bytes(g, w, f"mirt_reproject_moments {name} {params} {what}")
        for g, w, what in zip(d.run(gpu, params), want, NAMES4):
            vc.same_bytes(g, w, f"mirt_reproject_moments_device {name} {params} {what}")


def test_moments_outputs_one_at_a_time_aliasing_and_a_stream(gpu):
    import torch
    s = torch.cuda.Stream()
    for name in ("right", "first", "nonfinite_5_3", "syn_1_7", "motion:diffused_right", "motion:m_70_5",
                 "motion:range_9_3"):
        c, _ = vc.moment_case(name)
        for params in c["params"][:2]:
            want = host_moments(name, params)
            d = Moments(name)
            hist, out, rgb, m2 = d.run(gpu, params, want_rgb=False)
            for g, w, what in zip((hist, out, m2), (want[0], want[1], want[3]), ("hist_out", "out", "m2_out")):
                vc.same_bytes(g, w, f"{name} {params} {what}, out alone")
            assert untouched(d.rgb)
            d = Moments(name)
            hist, out, rgb, m2 = d.run(gpu, params, want_out=False)
            vc.same_bytes(rgb, want[2], f"{name} {params} out_rgb alone")
            vc.same_bytes(m2, want[3], f"{name} {params} m2_out, out_rgb alone")
            assert untouched(d.out)
            d = Moments(name)
            hist, out, rgb, m2 = d.run(gpu, params, want_out=False, want_rgb=False)
            vc.same_bytes(hist, want[0], f"{name} {params} hist_out alone")
            vc.same_bytes(m2, want[3], f"{name} {params} m2_out alone")
            assert untouched(d.out) and untouched(d.rgb)
            d = Moments(name)
            for g, w, what in zip(d.run(gpu, params, stream=s.cuda_stream), want, NAMES4):
                vc.same_bytes(g, w, f"{name} {params} on a torch stream, {what}")
            for g, w, what in zip(d.run(gpu, params), want, NAMES4):   # behind the other stream's launch
                vc.same_bytes(g, w, f"{name} {params} back on the default stream, {what}")
            d = Moments(name)
            for g, w, what in zip(d.run(gpu, params, alias=True), want, NAMES4):
                vc.same_bytes(g, w, f"{name} {params} d_out aliasing d_rgba, {what}")
            assert untouched(d.out)
    # the binding's device form: tensors in, tensors out
    name = "yaw"
    c, _ = vc.moment_case(name)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731
    records = np.array(c["hist"]).view(F32).reshape(H, W, 4)   # the same 16 bytes per pixel
    prev = (c["cam_prev"], to(records), to(c["t_prev"]), to(c["sphere_prev"]), to(vc.m2_prev_of(name)))
    want = host_moments(name, rc.DEFAULT)
    hist, out, rgb, m2 = gpu.reproject_moments(c["cam"], to(c["rgba"]), to(c["t"]), to(c["sphere"]), prev=prev, rgb=True)
    torch.cuda.synchronize()
    vc.same_bytes(hist.cpu().numpy().view(rc.abi.HISTORY).reshape(H, W), want[0], "Renderer.reproject_moments on tensors")
    vc.same_bytes(out.cpu().numpy(), want[1], "Renderer.reproject_moments on tensors, out")
    vc.same_bytes(rgb.cpu().numpy(), want[2], "Renderer.reproject_moments on tensors, rgb")
    vc.same_bytes(m2.cpu().numpy(), want[3], "Renderer.reproject_moments on tensors, m2")


class Filter:
    """A filter case in device memory, outputs between canaries."""

    def __init__(self, c):
        import torch
        self.torch, self.c = torch, c
        self.hist, self.m2, self.sphere = up(torch, c["hist"]), up(torch, c["m2"]), up(torch, c["sphere"])
        self.normal = up(torch, c["normal"])
        n = c["width"] * c["height"]
        self.out, self.rgb, self.var = full(torch, 4 * n), full(torch, 12 * n), full(torch, 4 * n)
        torch.cuda.synchronize()

    def run(self, gpu, params, stream=None, want_out=True, want_rgb=True, want_var=True):
        """mirt_denoise_var_device: (out, out_rgb, var_out) from the device (None if not asked for)."""
        c, p = self.c, vc.params_struct(params)
        r = gpu.L.mirt_denoise_var_device(gpu.h, c["width"], c["height"], dp(self.hist), dp(self.m2), dp(self.sphere),
                                          dp(self.normal) if params[4] else None, C.byref(p),
                                          dp(self.out, PAD) if want_out else None,
                                          dp(self.rgb, PAD) if want_rgb else None,
                                          dp(self.var, PAD) if want_var else None, C.c_void_p(stream or 0))
        assert r == 0, gpu.L.mirt_last_error().decode()
        self.torch.cuda.synchronize()
        h, w = c["height"], c["width"]
        out = self.out[PAD:-PAD].cpu().numpy().reshape(h, w, 4) if want_out else None
        rgb = self.rgb[PAD:-PAD].cpu().numpy().view(F32).reshape(h, w, 3) if want_rgb else None
        var = self.var[PAD:-PAD].cpu().numpy().view(F32).reshape(h, w) if want_var else None
        canaries_hold(self.out, self.rgb, self.var)
        return out, rgb, var


def blocking(gpu, c, params):
    return gpu.denoise_var(c["hist"], c["m2"], c["sphere"], c["normal"] if params[4] else None, params=params[:4],
                           rgb=True, var=True)


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("name", vc.FILTER_CASES)
def test_filter_both_forms_equal_the_host_form(gpu, mirt, name, tile):
    c = vc.case(name)
    d = Filter(c)
    hostile = name in vc.HOSTILE
    with options(gpu, {mirt.abi.OPT_DENOISE_TILE: tile}):
        for params in vc.PARAMS:
            want = host_filter(name, params)
            vc.check(blocking(gpu, c, params), want, f"mirt_denoise_var {name} {params} tile {tile}", hostile)
            vc.check(d.run(gpu, params), want, f"mirt_denoise_var_device {name} {params} tile {tile}", hostile)


@pytest.mark.parametrize("tile", [0, 1])
def test_filter_outputs_one_at_a_time_and_a_stream(gpu, mirt, tile):
    import torch
    s = torch.cuda.Stream()
    with options(gpu, {mirt.abi.OPT_DENOISE_TILE: tile}):
        for name in ("loop", "syn_129_70", "syn_1_37", "m2_33_65"):
            c = vc.case(name)
            hostile = name in vc.HOSTILE
            for params in (vc.DEFAULT, (5, 7, 0.5, 1, True), (2, 0, 4.0, 65536, False)):
                want = host_filter(name, params)
                d = Filter(c)
                got = d.run(gpu, params, want_rgb=False, want_var=False)
                assert got[1] is None and got[2] is None
                vc.check(got, want, f"{name} {params} out alone", hostile)
                assert untouched(d.rgb) and untouched(d.var)
                d = Filter(c)
                vc.check(d.run(gpu, params, want_out=False, want_var=False), want, f"{name} {params} out_rgb alone", hostile)
                assert untouched(d.out) and untouched(d.var)
                d = Filter(c)
                vc.check(d.run(gpu, params, stream=s.cuda_stream), want, f"{name} {params} on a torch stream", hostile)
                vc.check(d.run(gpu, params), want, f"{name} {params} back on the default stream", hostile)
    # the binding's device form: tensors in, tensors out
    c = vc.case("loop")
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731
    records = np.array(c["hist"]).view(F32).reshape(H, W, 4)
    out, rgb, var = gpu.denoise_var(to(records), to(c["m2"]), to(c["sphere"]), to(c["normal"]), params=vc.DEFAULT[:4],
                                    rgb=True, var=True)
    torch.cuda.synchronize()
    vc.check((out.cpu().numpy(), rgb.cpu().numpy(), var.cpu().numpy()), host_filter("loop", vc.DEFAULT),
             "Renderer.denoise_var on tensors", False)


def test_filter_scratch_grows_and_shrinks(mirt):
    """A ctx of its own: small, large, small again, with and without the second image."""
    with mirt.Renderer(0) as r:
        for name, params in [("syn_5_3", (1, 3, 4.0, 4, False)), ("syn_129_70", (5, 3, 0.5, 4, True)),
                             ("syn_2_2", (2, 3, 4.0, 4, True)), ("loop", vc.DEFAULT),
                             ("syn_129_70", (1, 0, 0.0, 1, False)), ("syn_1_1", (5, 7, 0.5, 65536, True))]:
            c = vc.case(name)
            vc.check(blocking(r, c, params), host_filter(name, params), f"{name} {params}", False)
            vc.check(Filter(c).run(r, params), host_filter(name, params), f"device {name} {params}", False)


# ---- the frame form

PATH = [f"path{k}" for k in range(5)]
N = rc.N


def frame_kw(k):
    return dict(depth=5, seed=1, sample=k)


class Loop:
    """mirt_render_frame_reprojected_denoised on a ctx beside mirt_render_frame_planes composed with the two host
    forms, frame by frame."""

    def __init__(self, gpu, mirt, params=rc.DEFAULT, var_params=None):
        self.gpu, self.L, self.params = gpu, mirt.load(), params
        p = mirt.Renderer._denoise_var_params(None)
        self.vp = var_params or (p.passes, p.normal_sharpness, p.sigma_lum, p.min_history)
        self.prev, self.k, self.frames = None, 0, 0

    def frame(self, cam, what, keep=True, motion=None, w=W):
        """One frame from `cam`. keep False: the host loop starts over. Returns (raw, reprojected, hist)."""
        gpu, k = self.gpu, self.k
        raw, pl = gpu.render_frame_planes(cam, w, H, planes=("t", "sphere", "normal"), **frame_kw(k))
        prev = self.prev if keep else None
        hist, want_rep, m2 = vc.host_moments_step(self.L, cam, raw, pl["t"], pl["sphere"], prev, self.params, motion)
        c = dict(width=w, height=H, hist=hist, m2=m2, sphere=pl["sphere"], normal=np.ascontiguousarray(pl["normal"]))
        want_out = vc.host(self.L, c, self.vp + (True,), want_rgb=False, want_var=False)[0]
        out, rep, raw2 = gpu.render_frame_reprojected_denoised(cam, w, H, params=self.params, var_params=self.vp,
                                                               reprojected=True, raw=True, **frame_kw(k))
        vc.same_bytes(raw2, raw, f"{what}: raw")
        vc.same_bytes(rep, want_rep, f"{what}: reprojected")
        vc.same_bytes(gpu.history_read(), hist, f"{what}: the records")
        vc.same_bytes(gpu.history_moments_read(), m2, f"{what}: m2")
        vc.same_bytes(out, want_out, f"{what}: out")
        self.prev, self.k = (cam, hist, pl["t"], pl["sphere"], m2), k + 1
        self.frames = 1 if prev is None else self.frames + 1
        st = gpu.history_stats()
        assert st["frames"] == self.frames and st["scene_id"] == gpu.scene_id(), (what, st)
        assert (st["reused"] > 0) == (prev is not None), (what, st)
        return raw, rep, hist


@pytest.mark.parametrize("params", [rc.DEFAULT, (3, 1, 0.015625)])
def test_the_frame_call_along_a_path(gpu, mirt, params):
    upload(gpu, mirt, N)
    gpu.history_reset()
    loop = Loop(gpu, mirt, params)
    with mirt.Renderer(0) as other:   # the plain reprojected loop, on a second ctx sharing the scene
        other.share_scene(gpu)
        try:
            for k, name in enumerate(PATH):
                cam = rc.camera(name)
                plain = gpu.render_frame(cam, W, H, **frame_kw(k))
                acc_plain = gpu.accum(3 * W * H)
                raw, rep, hist = loop.frame(cam, f"frame {k}")
                vc.same_bytes(raw, plain, f"raw of frame {k} against the plain frame")
                vc.same_bytes(gpu.accum(3 * W * H), acc_plain, f"the accumulation buffer after frame {k}")
                vc.same_bytes(other.render_frame_reprojected(cam, W, H, params=params, **frame_kw(k)), rep,
                              f"frame {k}: mirt_render_frame_reprojected's display")
                vc.same_bytes(other.history_read(), hist, f"frame {k}: mirt_render_frame_reprojected's records")
                with pytest.raises(mirt.MirtError):
                    other.history_moments_read()
            # without the optional outputs
            out = gpu.render_frame_reprojected_denoised(rc.camera("path4"), W, H, params=params, **frame_kw(5))
            assert out.shape == (H, W, 4) and gpu.history_stats()["frames"] == 6
        finally:
            other.share_scene(None)
    # a plain frame afterwards still matches its golden bytes
    vc.same_bytes(gpu.render_frame(cases.camera("A"), W, H, depth=5, seed=1, sample=1), dc.oracle_frame(1),
                  "a plain frame afterwards")


def test_the_frame_call_empties_its_history_when_it_must(gpu, mirt):
    upload(gpu, mirt, N)
    gpu.history_reset()
    loop = Loop(gpu, mirt)
    cams = [rc.camera(n) for n in PATH]
    loop.frame(cams[0], "first")
    loop.frame(cams[1], "second")
    assert gpu.history_stats()["frames"] == 2
    # a plain reprojected call in between keeps the history and drops the moments: the next denoised call starts over
    gpu.render_frame_reprojected(cams[2], W, H, **frame_kw(2))
    assert gpu.history_stats()["frames"] == 3
    with pytest.raises(mirt.MirtError):
        gpu.history_moments_read()
    loop.k = 3
    loop.frame(cams[3], "after a plain reprojected call", keep=False)
    assert gpu.history_stats()["frames"] == 1
    loop.frame(cams[4], "and on")
    gpu.history_reset()
    with pytest.raises(mirt.MirtError):
        gpu.history_moments_read()
    loop.frame(cams[0], "after mirt_history_reset", keep=False)
    loop.frame(cams[1], "and on")
    upload(gpu, mirt, N)   # the same scene again: a new scene id
    loop.frame(cams[2], "after an install", keep=False)
    loop.frame(cams[3], "and on")
    loop.frame(cams[4], "after a change of width", keep=False, w=W - 3)
    loop.frame(cams[0], "after a change of width back", keep=False)
    loop.frame(cams[1], "and on")


def test_the_frame_call_is_carried_over_a_refit_and_a_rebuild(gpu, mirt):
    from test_reproject_motion_gpu import geo_now, history_motion
    spheres = upload(gpu, mirt, N)
    gpu.history_reset()
    with history_motion(mirt, gpu):
        loop = Loop(gpu, mirt)
        loop.frame(rc.camera("path0"), "the first frame")
        held = spheres
        for step, max_decay in enumerate([0.0, 1e-3]):
            what = f"step {step}: update {max_decay}"
            before = geo_now(gpu)
            moved = mc.diffused(held, mc.SIGMA, 40 + step)
            held, perm, res = gpu.update_scene(moved, 0, N, max_decay)
            assert res["rebuilt"] == int(max_decay > 0), (what, res)
            frames = loop.frames
            loop.frame(rc.camera(f"path{step + 1}"), what, motion=(geo_now(gpu), before, perm if res["rebuilt"] else None))
            assert loop.frames == frames + 1 and gpu.history_motion()["carried"] == 1, what
    upload(gpu, mirt, N)
    gpu.history_reset()


def test_a_ctx_that_never_makes_the_call_holds_what_it_held(gpu, mirt):
    """the history is 256 + 2 * 16 n + 4 * 4 n + 4 n bytes; the first denoised call adds
    2 * 4 n + 12 n + 4 n."""
    upload(gpu, mirt, N)
    n = W * H
    with mirt.Renderer(0) as r:
        r.share_scene(gpu)
        try:
            assert r.history_stats()["bytes"] == 0
            r.render_frame_reprojected(rc.camera("path0"), W, H, **frame_kw(0))
            assert r.history_stats()["bytes"] == 256 + 2 * 16 * n + 4 * 4 * n + 4 * n
            r.render_frame_reprojected_denoised(rc.camera("path1"), W, H, **frame_kw(1))
            st = r.history_stats()
            assert st["bytes"] == 256 + 2 * 16 * n + 4 * 4 * n + 4 * n + 2 * 4 * n + 12 * n + 4 * n and st["frames"] == 1
        finally:
            r.share_scene(None)

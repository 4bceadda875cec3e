"""The reprojection on the GPU: mirt_reproject_device and mirt_reproject equal
mirt_reproject_host byte for byte on every case and parameter set of
tests/reproject_cases.py (which the host tests hold against the numpy
restatement) -- the non-finite t included, with canaries around every device
output -- with the outputs one at a time, d_out aliasing d_rgba and a torch
stream; mirt_render_frame_reprojected along a camera path equals
mirt_render_frame_planes composed with mirt_reproject_host frame by frame, its
history empties when it must, its counts add up, a plain frame afterwards is
unchanged, and the argument errors come back without a device call."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_cases as dc
import reproject_cases as rc
import test_planes_cases as cases
from test_planes_gpu import upload

pytestmark = pytest.mark.gpu

W, H = rc.W, rc.H
CANARY, PAD = 0x5A, 256   # bytes around each device output


@functools.lru_cache(maxsize=None)
def host(name, params):
    """mirt_reproject_host's (hist_out, out, out_rgb) of a case, computed once."""
    hist, out, rgb = rc.host(rc.mirt.load(), rc.case(name), params)
    for a in (hist, out, rgb):
        a.setflags(write=False)
    return hist, out, rgb


def prev_of(c):
    return None if c["cam_prev"] is None else (c["cam_prev"], c["hist"], c["t_prev"], c["sphere_prev"])


class Device:
    """A case in device memory, outputs between canaries."""

    def __init__(self, c):
        import torch
        self.torch, self.c = torch, c
        dev = torch.device("cuda", 0)
        up = lambda a: None if a is None else torch.from_numpy(np.array(a).view(np.uint8)).to(dev)   # noqa: E731
        self.rgba, self.t, self.sphere = up(c["rgba"]), up(c["t"]), up(c["sphere"])
        self.hist, self.t_prev, self.sphere_prev = up(c["hist"]), up(c["t_prev"]), up(c["sphere_prev"])
        n = c["width"] * c["height"]
        self.n = n
        full = lambda b: torch.full((2 * PAD + b,), CANARY, dtype=torch.uint8, device=dev)   # noqa: E731
        self.ho, self.out, self.rgb = full(16 * n), full(4 * n), full(12 * n)
        torch.cuda.synchronize()

    def run(self, gpu, params, stream=None, alias=False, want_out=True, want_rgb=True):
        """mirt_reproject_device; returns (hist_out, out, out_rgb) from the device (None if not asked for)."""
        c, p = self.c, rc.params_struct(params)
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None   # noqa: E731
        ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
        d_out = (dp(self.rgba) if alias else dp(self.out, PAD)) if want_out else None
        r = gpu.L.mirt_reproject_device(gpu.h, c["width"], c["height"], ref(c["cam"]), ref(c["cam_prev"]),
                                        dp(self.rgba), dp(self.t), dp(self.sphere), dp(self.hist), dp(self.t_prev),
                                        dp(self.sphere_prev), C.byref(p), dp(self.ho, PAD), d_out,
                                        dp(self.rgb, PAD) if want_rgb else None, C.c_void_p(stream or 0))
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


@pytest.mark.parametrize("name", rc.CASES)
def test_both_forms_equal_the_host_form(gpu, name):
    c = rc.case(name)
    d = Device(c)
    for params in c["params"]:
        want = host(name, params)
        got = gpu.reproject(c["cam"], c["rgba"], c["t"], c["sphere"], prev=prev_of(c), params=params, rgb=True)
        for g, w, what in zip(got, want, ("hist_out", "out", "out_rgb")):
            rc.same_bytes(g, w, f"mirt_reproject {name} {params} {what}")
        got = d.run(gpu, params)
        for g, w, what in zip(got, want, ("hist_out", "out", "out_rgb")):
            rc.same_bytes(g, w, f"mirt_reproject_device {name} {params} {what}")


def test_outputs_one_at_a_time_aliasing_and_a_stream(gpu):
    import torch
    s = torch.cuda.Stream()
    for name in ("right", "first", "nonfinite_5_3", "syn_1_7", "last_5_3"):
        c = rc.case(name)
        for params in c["params"][:2]:
            want_hist, want_out, want_rgb = host(name, params)
            d = Device(c)
            hist, out, rgb = d.run(gpu, params, want_rgb=False)
            rc.same_bytes(hist, want_hist, f"{name} {params} hist_out, out alone")
            rc.same_bytes(out, want_out, f"{name} {params} out alone")
            assert (d.rgb.cpu().numpy() == CANARY).all()
            d = Device(c)
            hist, out, rgb = d.run(gpu, params, want_out=False)
            rc.same_bytes(rgb, want_rgb, f"{name} {params} out_rgb alone")
            assert (d.out.cpu().numpy() == CANARY).all()
            d = Device(c)
            hist, out, rgb = d.run(gpu, params, want_out=False, want_rgb=False)
            rc.same_bytes(hist, want_hist, f"{name} {params} hist_out alone")
            assert (d.out.cpu().numpy() == CANARY).all() and (d.rgb.cpu().numpy() == CANARY).all()
            d = Device(c)
            hist, out, rgb = d.run(gpu, params, stream=s.cuda_stream)
            rc.same_bytes(hist, want_hist, f"{name} {params} on a torch stream, hist_out")
            rc.same_bytes(out, want_out, f"{name} {params} on a torch stream")
            rc.same_bytes(rgb, want_rgb, f"{name} {params} on a torch stream, out_rgb")
            hist, out, _ = d.run(gpu, params)   # back on the default stream: behind the other stream's launch
            rc.same_bytes(hist, want_hist, f"{name} {params} back on the default stream, hist_out")
            rc.same_bytes(out, want_out, f"{name} {params} back on the default stream")
            d = Device(c)
            hist, out, rgb = d.run(gpu, params, alias=True)
            rc.same_bytes(hist, want_hist, f"{name} {params} d_out aliasing d_rgba, hist_out")
            rc.same_bytes(out, want_out, f"{name} {params} d_out aliasing d_rgba")
            rc.same_bytes(rgb, want_rgb, f"{name} {params} aliasing, out_rgb")
            assert (d.out.cpu().numpy() == CANARY).all()
    # the binding's device form: tensors in, tensors out, `out` may be rgba itself
    c = rc.case("yaw")
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731
    rgba, t, sphere = up(c["rgba"]), up(c["t"]), up(c["sphere"])
    records = np.array(c["hist"]).view(np.float32).reshape(H, W, 4)   # the same 16 bytes per pixel
    prev = (c["cam_prev"], up(records), up(c["t_prev"]), up(c["sphere_prev"]))
    want_hist, want_out, want_rgb = host("yaw", rc.DEFAULT)
    hist, out, rgb = gpu.reproject(c["cam"], rgba, t, sphere, prev=prev, rgb=True)
    torch.cuda.synchronize()
    rc.same_bytes(hist.cpu().numpy().view(rc.abi.HISTORY).reshape(H, W), want_hist, "Renderer.reproject on tensors")
    rc.same_bytes(out.cpu().numpy(), want_out, "Renderer.reproject on tensors, out")
    rc.same_bytes(rgb.cpu().numpy(), want_rgb, "Renderer.reproject on tensors, rgb")
    assert gpu.reproject(c["cam"], rgba, t, sphere, prev=prev, out=rgba)[1] is rgba
    torch.cuda.synchronize()
    rc.same_bytes(rgba.cpu().numpy(), want_out, "Renderer.reproject in place")


PATH = [f"path{k}" for k in range(5)]


def frame_kw(k):
    return dict(depth=5, seed=1, sample=k)


def host_loop(gpu, L, names, params, prev=None, k0=0):
    """mirt_render_frame_planes composed with mirt_reproject_host along the
    cameras `names`: [(raw, out, hist, sphere)] and the last state."""
    steps = []
    for k, name in enumerate(names, k0):
        raw, pl = gpu.render_frame_planes(rc.camera(name), W, H, planes=("t", "sphere"), **frame_kw(k))
        hist, out = rc.host_step(L, rc.camera(name), raw, pl["t"], pl["sphere"], prev, params)
        prev = (rc.camera(name), hist, pl["t"], pl["sphere"])
        steps.append((raw, out, hist, pl["sphere"]))
    return steps, prev


@pytest.mark.parametrize("params", [rc.DEFAULT, (3, 1, 0.015625)])
def test_the_moving_camera_loop(gpu, mirt, params):
    upload(gpu, mirt, rc.N)
    L = mirt.load()
    gpu.history_reset()
    want, last = host_loop(gpu, L, PATH, params)
    acc_plain = None
    for k, name in enumerate(PATH):
        plain = gpu.render_frame(rc.camera(name), W, H, **frame_kw(k))
        acc_plain = gpu.accum(3 * W * H)
        out, raw = gpu.render_frame_reprojected(rc.camera(name), W, H, params=params, raw=True, **frame_kw(k))
        rc.same_bytes(raw, plain, f"raw of frame {k}")
        rc.same_bytes(raw, want[k][0], f"raw of frame {k} against the planes frame")
        rc.same_bytes(out, want[k][1], f"out of frame {k}")
        rc.same_bytes(gpu.history_read(), want[k][2], f"the records after frame {k}")
        rc.same_bytes(gpu.accum(3 * W * H), acc_plain, f"the accumulation buffer after frame {k}")
        st = gpu.history_stats()
        hist = want[k][2]
        sky = int((want[k][3] < 0).sum())
        assert st["reused"] + st["fresh"] + st["sky"] == W * H, st
        assert (st["frames"], st["width"], st["height"], st["scene_id"]) == (k + 1, W, H, gpu.scene_id()), st
        assert st["sky"] == sky and st["reused"] == int((hist["n"] > 1).sum()), (st, sky)
        assert st["bytes"] >= 2 * 24 * W * H + 4 * W * H
        if k == 0:
            assert st["reused"] == 0
        else:
            assert st["reused"] > 0.5 * (W * H - sky), st
    # without `raw`, from the history as it stands: frame 5 of the path
    more, _ = host_loop(gpu, L, ["path5"], params, prev=last, k0=5)
    rc.same_bytes(gpu.render_frame_reprojected(rc.camera("path5"), W, H, params=params, **frame_kw(5)), more[0][1],
                  "frame 5, without raw")
    # a plain frame afterwards still matches its golden bytes
    rc.same_bytes(gpu.render_frame(cases.camera("A"), W, H, depth=5, seed=1, sample=1), dc.oracle_frame(1),
                  "a plain frame afterwards")


def test_the_history_empties_when_it_must(gpu, mirt):
    upload(gpu, mirt, rc.N)
    L = mirt.load()
    gpu.history_reset()

    def two(k0, w=W):
        """Two frames along the path: the second one's reused count."""
        for k in (k0, k0 + 1):
            out = gpu.render_frame_reprojected(rc.camera(f"path{k % 5}"), w, H, **frame_kw(k))
        return out, gpu.history_stats()

    def first_again(k, what, w=W):
        """The next call starts from nothing: its display is its one-sample frame's."""
        cam = rc.camera(f"path{k % 5}")
        out, raw = gpu.render_frame_reprojected(cam, w, H, raw=True, **frame_kw(k))
        st = gpu.history_stats()
        assert (st["frames"], st["reused"], st["width"]) == (1, 0, w), (what, st)
        _, pl = gpu.render_frame_planes(cam, w, H, planes=("t", "sphere"), **frame_kw(k))
        hist, want = rc.host_step(L, cam, raw, pl["t"], pl["sphere"], None, rc.DEFAULT)
        rc.same_bytes(out, want, f"{what}: the display")
        rc.same_bytes(gpu.history_read(), hist, f"{what}: the records")
        assert (hist["n"] == 1).all()

    _, st = two(0)
    assert st["frames"] == 2 and st["reused"] > 0
    gpu.history_reset()
    assert gpu.history_stats()["frames"] == 0
    with pytest.raises(mirt.MirtError):
        gpu.history_read()
    first_again(2, "after mirt_history_reset")
    _, st = two(3)
    assert st["frames"] == 3 and st["reused"] > 0
    sid = gpu.scene_id()
    upload(gpu, mirt, rc.N)   # the same scene again: a new scene id
    assert gpu.scene_id() != sid
    first_again(5, "after an install of the same scene")
    _, st = two(6)
    assert st["frames"] == 3 and st["reused"] > 0
    first_again(8, "after a change of width", w=W - 3)
    first_again(9, "after a change of width back")
    # a ctx of its own starts empty, and grows and shrinks its buffers
    with mirt.Renderer(0) as r:
        r.share_scene(gpu)
        try:
            assert r.history_stats()["frames"] == 0 and r.history_stats()["bytes"] == 0
            for w in (5, W, 7):
                for k in (0, 1):
                    out, raw = r.render_frame_reprojected(rc.camera("path0"), w, H, raw=True, **frame_kw(k))
                    st = r.history_stats()
                    assert st["reused"] + st["fresh"] + st["sky"] == w * H and st["frames"] == k + 1, st
                    assert (st["reused"] > 0) == (k == 1) or st["sky"] == w * H
        finally:
            r.share_scene(None)


def test_argument_errors_without_a_device_call(gpu, mirt):
    """On the live ctx: each error leaves the history, its counts and the
    accumulation buffer as they were."""
    upload(gpu, mirt, rc.N)
    gpu.history_reset()
    gpu.render_frame_reprojected(rc.camera("path0"), W, H, **frame_kw(0))
    before, records, acc = gpu.history_stats(), gpu.history_read(), gpu.accum(3 * W * H)
    cam = rc.camera("path1")
    for kw in (dict(accumulate=True, frames=2), dict(samples=2), dict(num_shards=2), dict(jitter=True),
               dict(depth=0)):
        with pytest.raises(mirt.MirtError, match="invalid arguments"):
            gpu.render_frame_reprojected(cam, W, H, **dict(frame_kw(1), **kw))
    for params in ((0, 4, 0.0), (64, 2, 0.0), (64, 4, -1.0), (64, 4, float("nan")), (65537, 1, 0.0)):
        with pytest.raises(mirt.MirtError, match="invalid arguments"):
            gpu.render_frame_reprojected(cam, W, H, params=params, **frame_kw(1))
    c = rc.case("right")
    with pytest.raises(mirt.MirtError, match="invalid arguments"):
        gpu.reproject(c["cam"], c["rgba"], c["t"], c["sphere"], prev=(None,) + prev_of(c)[1:])
    with pytest.raises(mirt.MirtError, match="invalid arguments"):
        gpu.reproject(c["cam"], c["rgba"], c["t"], c["sphere"], prev=prev_of(c), params=(64, 3, 0.0))
    with mirt.Renderer(0) as other:
        other.share_scene(gpu)
        other.share_accum(gpu)
        try:
            for r in (gpu, other):
                with pytest.raises(mirt.MirtError, match="shares its accumulation buffer"):
                    r.render_frame_reprojected(cam, W, H, **frame_kw(1))
        finally:
            other.share_accum(None)
            other.share_scene(None)
    assert gpu.history_stats() == before
    rc.same_bytes(gpu.history_read(), records, "the records after the errors")
    rc.same_bytes(gpu.accum(3 * W * H), acc, "the accumulation buffer after the errors")
    out = gpu.render_frame_reprojected(cam, W, H, **frame_kw(1))
    assert gpu.history_stats()["frames"] == 2 and gpu.history_stats()["reused"] > 0 and out.shape == (H, W, 4)


def test_under_the_primary_cache(gpu, mirt):
    """The frame is the BYPASS (PLANES) any planes frame is, and leaves the cache valid."""
    from test_planes_gpu import options
    upload(gpu, mirt, rc.N)
    gpu.history_reset()
    with options(gpu, {mirt.abi.OPT_PRIMARY_CACHE: 1}):
        gpu.render_frame(cases.camera("A"), W, H, depth=5)
        assert gpu.primary_cache_stats()["last"] == "fill"
        out = gpu.render_frame_reprojected(cases.camera("A"), W, H, depth=5, seed=1, sample=1)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["valid"]) == ("bypass", "PLANES", 1), st
    pl = cases.expected("A")
    _, want = rc.host_step(mirt.load(), cases.camera("A"), dc.oracle_frame(1), pl["t"], pl["sphere"], None, rc.DEFAULT)
    rc.same_bytes(out, want, "against the host form of the oracle's frame and planes")

"""The denoiser on the GPU: mirt_denoise_device and mirt_denoise equal
mirt_denoise_host byte for byte on every case and parameter set of
tests/denoise_cases.py (which the host tests hold against the numpy
restatement), with either pass kernel (MIRT_OPT_DENOISE_TILE), both sources,
both outputs, d_out aliasing d_rgba, canaries around both outputs, a torch
stream, and scratch that grows and shrinks; mirt_render_frame_denoised returns
the plain frame and the host filter of it, leaves the accumulating loop's
buffer as the plain loop leaves it, also through a lens, and a plain frame
afterwards is unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_cases as dc
import lens_frame_cases as lc
import test_planes_cases as cases
from test_planes_gpu import options, upload

pytestmark = pytest.mark.gpu

W, H = dc.W, dc.H
CANARY, PAD = 0x5A, 256   # bytes around each device output
E_INVALID = -1


@functools.lru_cache(maxsize=None)
def host(name, params):
    """mirt_denoise_host's (out, out_rgb) of a case, computed once."""
    import importlib
    L = importlib.import_module("cs201_sah-bvh_ray_tracer_amd").load()
    out, rgb = dc.host(L, dc.case(name), params)
    out.setflags(write=False)
    rgb.setflags(write=False)
    return out, rgb


def blocking(gpu, c, params):
    return gpu.denoise(c["sphere"], c["normal"] if params[3] else None, rgba=c["rgba"], accum=c["accum"],
                       frames=c["frames"], params=params[:3], rgb=True)


class Device:
    """A case in device memory, outputs between canaries."""

    def __init__(self, c, with_normal=True):
        import torch
        self.torch, self.c = torch, c
        dev = torch.device("cuda", 0)
        up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)   # noqa: E731
        self.sphere, self.rgba, self.accum = up(c["sphere"]), up(c["rgba"]), up(c["accum"])
        self.normal = up(c["normal"]) if with_normal else None
        n = c["width"] * c["height"]
        self.out = torch.full((2 * PAD + 4 * n,), CANARY, dtype=torch.uint8, device=dev)
        self.rgb = torch.full((2 * PAD + 12 * n,), CANARY, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def run(self, gpu, params, stream=None, alias=False, want_out=True, want_rgb=True):
        """mirt_denoise_device; returns (out, out_rgb) from the device (None if not asked for)."""
        c, p = self.c, dc.params_struct(params)
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None   # noqa: E731
        d_out = (dp(self.rgba) if alias else dp(self.out, PAD)) if want_out else None
        rc = gpu.L.mirt_denoise_device(gpu.h, c["width"], c["height"], dp(self.rgba), dp(self.accum), c["frames"],
                                       dp(self.sphere), dp(self.normal) if params[3] else None, C.byref(p), d_out,
                                       dp(self.rgb, PAD) if want_rgb else None, C.c_void_p(stream or 0))
        assert rc == 0, gpu.L.mirt_last_error().decode()
        self.torch.cuda.synchronize()
        h, w = c["height"], c["width"]
        out_t = (self.rgba if alias else self.out[PAD:-PAD]) if want_out else None
        out = out_t.cpu().numpy().reshape(h, w, 4) if want_out else None
        rgb = self.rgb[PAD:-PAD].cpu().numpy().view(np.float32).reshape(h, w, 3) if want_rgb else None
        for buf in (self.out, self.rgb):
            edge = buf.cpu().numpy()
            assert (edge[:PAD] == CANARY).all() and (edge[-PAD:] == CANARY).all(), "a canary was overwritten"
        return out, rgb


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("name", dc.CASES)
def test_both_forms_equal_the_host_form(gpu, mirt, name, tile):
    c = dc.case(name)
    d = Device(c)
    with options(gpu, {mirt.abi.OPT_DENOISE_TILE: tile}):
        for params in dc.PARAMS:
            want_out, want_rgb = host(name, params)
            out, rgb = blocking(gpu, c, params)
            dc.same_bytes(rgb, want_rgb, f"mirt_denoise {name} {params} tile {tile} out_rgb")
            dc.same_bytes(out, want_out, f"mirt_denoise {name} {params} tile {tile} out")
            out, rgb = d.run(gpu, params)
            dc.same_bytes(rgb, want_rgb, f"mirt_denoise_device {name} {params} tile {tile} out_rgb")
            dc.same_bytes(out, want_out, f"mirt_denoise_device {name} {params} tile {tile} out")


@pytest.mark.parametrize("tile", [0, 1])
def test_outputs_one_at_a_time_aliasing_and_a_stream(gpu, mirt, tile):
    import torch
    s = torch.cuda.Stream()
    with options(gpu, {mirt.abi.OPT_DENOISE_TILE: tile}):
        for name in ("A1", "Asum", "syn_129_70", "acc_33_65", "syn_1_37"):
            c = dc.case(name)
            for params in (dc.DEFAULT, (5, 7, 0.5, True), (2, 0, 0.5, False)):
                want_out, want_rgb = host(name, params)
                d = Device(c)
                out, rgb = d.run(gpu, params, want_rgb=False)
                assert rgb is None
                dc.same_bytes(out, want_out, f"{name} {params} out alone")
                assert (d.rgb.cpu().numpy() == CANARY).all()
                d = Device(c)
                out, rgb = d.run(gpu, params, want_out=False)
                dc.same_bytes(rgb, want_rgb, f"{name} {params} out_rgb alone")
                assert (d.out.cpu().numpy() == CANARY).all()
                d = Device(c)
                out, rgb = d.run(gpu, params, stream=s.cuda_stream)
                dc.same_bytes(out, want_out, f"{name} {params} on a torch stream")
                dc.same_bytes(rgb, want_rgb, f"{name} {params} on a torch stream, out_rgb")
                out, _ = d.run(gpu, params)   # back on the default stream: behind the other stream's launch
                dc.same_bytes(out, want_out, f"{name} {params} back on the default stream")
                if c["rgba"] is not None:
                    d = Device(c)
                    out, rgb = d.run(gpu, params, alias=True)
                    dc.same_bytes(out, want_out, f"{name} {params} d_out aliasing d_rgba")
                    dc.same_bytes(rgb, want_rgb, f"{name} {params} aliasing, out_rgb")
                    assert (d.out.cpu().numpy() == CANARY).all()
    # the binding's device form: tensors in, tensors out, `out` may be rgba itself
    c = dc.case("A2")
    d = Device(c)
    got, rgb = gpu.denoise(d.sphere, d.normal, rgba=d.rgba, rgb=True)
    torch.cuda.synchronize()
    dc.same_bytes(got.cpu().numpy(), host("A2", dc.DEFAULT)[0], "Renderer.denoise on tensors")
    dc.same_bytes(rgb.cpu().numpy(), host("A2", dc.DEFAULT)[1], "Renderer.denoise on tensors, rgb")
    assert gpu.denoise(d.sphere, d.normal, rgba=d.rgba, out=d.rgba) is d.rgba
    torch.cuda.synchronize()
    dc.same_bytes(d.rgba.cpu().numpy(), host("A2", dc.DEFAULT)[0], "Renderer.denoise in place")


def test_scratch_grows_and_shrinks(mirt):
    """A ctx of its own: small, large, small again, with and without the
    normals and the second image."""
    with mirt.Renderer(0) as r:
        for name, params in [("syn_5_3", (1, 3, 0.0, False)), ("syn_129_70", (5, 3, 0.5, True)),
                             ("syn_2_2", (2, 3, 0.0, True)), ("A0", dc.DEFAULT), ("syn_129_70", (1, 0, 0.0, False)),
                             ("syn_1_1", (5, 7, 0.5, True))]:
            c = dc.case(name)
            out, rgb = blocking(r, c, params)
            dc.same_bytes(out, host(name, params)[0], f"{name} {params}")
            dc.same_bytes(rgb, host(name, params)[1], f"{name} {params} out_rgb")
            out, rgb = Device(c).run(r, params)
            dc.same_bytes(out, host(name, params)[0], f"device {name} {params}")
            dc.same_bytes(rgb, host(name, params)[1], f"device {name} {params} out_rgb")


def cam_a():
    return cases.camera("A")


def test_the_frame_form(gpu, mirt):
    upload(gpu, mirt, dc.N)
    L = mirt.load()
    for kw in (dict(depth=5), dict(depth=1, seed=3, sample=2), dict(depth=5, seed=3, sample=2, jitter=True),
               dict(depth=5, use_bvh=False)):
        want = gpu.render_frame(cam_a(), W, H, **kw)
        _, planes = gpu.render_frame_planes(cam_a(), W, H, planes=("sphere", "normal"), **kw)
        for params in (dc.DEFAULT, (5, 7, 0.5, True), (1, 0, 0.0, True)):
            out, raw = gpu.render_frame_denoised(cam_a(), W, H, params=params[:3], raw=True, **kw)
            dc.same_bytes(raw, want, f"raw {kw}")
            dc.same_bytes(out, dc.host_filter(L, W, H, planes["sphere"], planes["normal"], params, rgba=want),
                          f"out {kw} {params}")
            dc.same_bytes(gpu.render_frame_denoised(cam_a(), W, H, params=params[:3], **kw), out, "without raw")
        dc.same_bytes(gpu.render_frame(cam_a(), W, H, **kw), want, "a plain frame afterwards")
    # the oracle's frame and planes, for once: the case the host tests filter
    out, raw = gpu.render_frame_denoised(cam_a(), W, H, raw=True, depth=5, seed=1, sample=1)
    dc.same_bytes(raw, dc.oracle_frame(1), "raw against the oracle")
    dc.same_bytes(out, host("A1", dc.DEFAULT)[0], "out against the host filter of the oracle's frame and planes")


def loop(gpu, lens, denoised, frames=4, **base):
    """The accumulating loop of main.c:379-408: (displays, filtered or None, the buffer after each frame)."""
    shown, filtered, acc = [], [], []
    for k in range(frames):
        kw = dict(sample=k, accumulate=k > 0, frames=k + 1, **base)
        if denoised:
            out, raw = gpu.render_frame_denoised(cam_a(), W, H, lens=lens, raw=True, **kw)
            filtered.append(out)
        elif lens is not None:
            raw = gpu.render_lens_frame(cam_a(), lens, W, H, **kw)
        else:
            raw = gpu.render_frame(cam_a(), W, H, **kw)
        shown.append(raw)
        acc.append(gpu.accum(3 * W * H).reshape(H, W, 3))
    return shown, filtered, acc


@pytest.mark.parametrize("lens", [None, "lens"])
def test_the_accumulating_loop(gpu, mirt, lens):
    upload(gpu, mirt, dc.N)
    L = mirt.load()
    lens = None if lens is None else lc.LENSES[lens]
    base = dict(depth=5, seed=1)
    shown, _, acc = loop(gpu, lens, False, **base)
    got_shown, filtered, got_acc = loop(gpu, lens, True, **base)
    for k in range(4):
        dc.same_bytes(got_shown[k], shown[k], f"display of frame {k}")
        dc.same_bytes(got_acc[k], acc[k], f"accumulation buffer after frame {k}")
        if lens is None:
            _, planes = gpu.render_frame_planes(cam_a(), W, H, planes=("sphere", "normal"), sample=k, **base)
        else:
            _, planes = gpu.render_lens_frame(cam_a(), lens, W, H, planes=("sphere", "normal"), sample=k, **base)
        src = dict(rgba=shown[0]) if k == 0 else dict(accum=acc[k], frames=k + 1)
        dc.same_bytes(filtered[k], dc.host_filter(L, W, H, planes["sphere"], planes["normal"], dc.DEFAULT, **src),
                      f"filtered frame {k}")
    assert (filtered[3] != shown[3]).any()
    # four samples in one call: the source is the buffer after the last fold, divisor 4
    gpu.render_frame_denoised(cam_a(), W, H, lens=lens, sample=0, **base)
    out, raw = gpu.render_frame_denoised(cam_a(), W, H, lens=lens, raw=True, sample=1, samples=3, accumulate=True,
                                         frames=2, **base)
    dc.same_bytes(raw, shown[3], "three samples at once, display")
    dc.same_bytes(gpu.accum(3 * W * H).reshape(H, W, 3), acc[3], "three samples at once, buffer")
    dc.same_bytes(out, filtered[3], "three samples at once, filtered")
    # and the plain loop afterwards is the plain loop
    again, _, acc_again = loop(gpu, lens, False, **base)
    dc.same_bytes(again[3], shown[3], "a plain loop afterwards")
    dc.same_bytes(acc_again[3], acc[3], "a plain loop afterwards, buffer")


def test_a_shared_accumulation_buffer_is_refused(gpu, mirt):
    upload(gpu, mirt, dc.N)
    with mirt.Renderer(0) as other:
        other.share_scene(gpu)
        other.share_accum(gpu)
        try:
            for r in (gpu, other):
                with pytest.raises(mirt.MirtError, match="shares its accumulation buffer"):
                    r.render_frame_denoised(cam_a(), W, H, depth=5)
        finally:
            other.share_accum(None)
            other.share_scene(None)
    out = gpu.render_frame_denoised(cam_a(), W, H, depth=5, seed=1, sample=1)
    dc.same_bytes(out, host("A1", dc.DEFAULT)[0], "private again")


def test_the_still_camera_recipe(gpu, mirt):
    """with the primary cache on, a denoised frame is a BYPASS
    (PLANES) that leaves the cache valid; the loop keeps the first frame's
    planes and filters plain cached frames with mirt_denoise_device."""
    import torch
    upload(gpu, mirt, dc.N)
    L = mirt.load()
    with options(gpu, {mirt.abi.OPT_PRIMARY_CACHE: 1}):
        _, planes = gpu.render_frame_planes(cam_a(), W, H, planes=("sphere", "normal"), depth=5)
        gpu.render_frame(cam_a(), W, H, depth=5)
        assert gpu.primary_cache_stats()["last"] == "fill"
        gpu.render_frame_denoised(cam_a(), W, H, depth=5)
        st = gpu.primary_cache_stats()
        assert (st["last"], st["reason"], st["valid"]) == ("bypass", "PLANES", 1), st
        dev = torch.device("cuda", 0)
        d_sphere = torch.from_numpy(planes["sphere"]).to(dev)
        d_normal = torch.from_numpy(planes["normal"]).to(dev)
        d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        d_acc = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for k in range(3):
            fd = mirt.frame_desc(W, H, depth=5, sample=k, accumulate=k > 0, frames=k + 1)
            gpu.render_frame_device(cam_a(), fd, d_out.data_ptr(), d_acc.data_ptr())
            assert gpu.primary_cache_stats()["last"] == "hit"
            shown = gpu.denoise(d_sphere, d_normal, accum=d_acc, frames=k + 1)
            torch.cuda.synchronize()
            want = dc.host_filter(L, W, H, planes["sphere"], planes["normal"], dc.DEFAULT,
                                  accum=d_acc.cpu().numpy(), frames=k + 1)
            dc.same_bytes(shown.cpu().numpy(), want, f"cached frame {k}")

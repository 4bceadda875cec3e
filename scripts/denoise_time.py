"""What the denoiser costs (mirt_denoise_device, mirt_render_frame_denoised:
csrc/denoise.h) at 1080p, 10k spheres, depth 5. The arms run interleaved in one
process; each figure is the median over --rounds rounds of the median of
--calls calls, host clock from the call to the stream idle. Prints one JSON
line.

  denoise_p{1,3,5}[_nonormal]_{direct,tile}
             mirt_denoise_device of a one-sample frame resident in HBM, its
             planes resident too, 1 / 3 / 5 passes, with and without the normal
             plane, by either pass kernel (MIRT_OPT_DENOISE_TILE 0 / 1: the tile
             kernel serves the passes of spacing 1 and 2)
  copy       a device-to-device copy of the same records (16 bytes of colour
             and 16 of normal per pixel): the floor of one pass's traffic
  plain      mirt_render_frame_device, the frame left in HBM
  host_plain mirt_render_frame, blocking, into pageable host memory
  host_denoised[_raw]
             mirt_render_frame_denoised, blocking, the filtered display (and
             the raw display too) into pageable host memory

and checks that both pass kernels give the host form's bytes at this size.

  python scripts/denoise_time.py [--spheres 10000] [--rounds 5] [--calls 7]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, default=10000)
    a = ap.parse_args()
    import torch   # before libmirt.so: one HIP runtime in the process
    m = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")
    W, H, n = a.width, a.height, a.width * a.height
    s = m.create_random_spheres(a.spheres, 1)
    b = m.build_bvh(s)
    r = m.Renderer(0)
    r.upload(s, b)
    cam = m.default_camera()
    dev = torch.device("cuda", 0)
    stream = r.stream_handle
    rgba, planes = r.render_frame_planes(cam, W, H, planes=("sphere", "normal"), depth=5)
    d_rgba = torch.from_numpy(rgba).to(dev)
    d_sphere = torch.from_numpy(planes["sphere"]).to(dev)
    d_normal = torch.from_numpy(planes["normal"]).to(dev)
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    d_frame = torch.zeros(n, dtype=torch.int32, device=dev)
    rec_a = torch.zeros(n * 8, dtype=torch.float32, device=dev)   # 32 bytes per pixel
    rec_b = torch.zeros(n * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = {"workload": f"{W}x{H}, {a.spheres} spheres, depth 5", "rounds": a.rounds, "calls": a.calls}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def denoise(passes, normal, tile):
        def call():
            r.set_option(m.abi.OPT_DENOISE_TILE, tile)
            r.denoise(d_sphere, d_normal if normal else None, rgba=d_rgba, params=(passes, 3, 0.0), out=d_out,
                      stream=stream)
            r.wait()
        return lambda: timed(call)

    hip = C_hip()

    def copy():
        def call():
            hip.hipMemcpyAsync(rec_b.data_ptr(), rec_a.data_ptr(), n * 32, 3, stream)   # hipMemcpyDeviceToDevice
            r.wait()
        return lambda: timed(call)

    fd = m.frame_desc(W, H, depth=5)

    def plain():
        def call():
            r.render_frame_device(cam, fd, d_frame.data_ptr(), stream=stream)
            r.wait()
        return lambda: timed(call)

    arms = {}
    for passes in (1, 3, 5):
        for normal in (True, False):
            for tile in (0, 1):
                arms[f"denoise_p{passes}{'' if normal else '_nonormal'}_{'tile' if tile else 'direct'}"] = \
                    denoise(passes, normal, tile)
    arms["copy"] = copy()
    arms["plain"] = plain()
    arms["host_plain"] = lambda: timed(lambda: r.render_frame(cam, W, H, depth=5))
    arms["host_denoised"] = lambda: timed(lambda: r.render_frame_denoised(cam, W, H, depth=5))
    arms["host_denoised_raw"] = lambda: timed(lambda: r.render_frame_denoised(cam, W, H, raw=True, depth=5))
    default_tile = r.get_option(m.abi.OPT_DENOISE_TILE)
    for fn in arms.values():
        fn()
    per = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():   # interleaved: every arm once per round
            if k.startswith("host"):
                r.set_option(m.abi.OPT_DENOISE_TILE, default_tile)
            per[k].append(statistics.median(fn() for _ in range(a.calls)))
    for k, v in per.items():
        out[f"{k}_ms"] = round(statistics.median(v), 4)
        out[f"{k}_ms_spread"] = [round(min(v), 4), round(max(v), 4)]
    out["default_tile"] = default_tile
    for passes in (1, 3, 5):
        for suffix in ("", "_nonormal"):
            out[f"p{passes}{suffix}_tile_over_direct"] = round(out[f"denoise_p{passes}{suffix}_tile_ms"] /
                                                               out[f"denoise_p{passes}{suffix}_direct_ms"], 4)
    out["host_denoised_over_host_plain"] = round(out["host_denoised_ms"] / out["host_plain_ms"], 4)

    # both kernels give the host form's bytes
    want = np.zeros((H, W, 4), np.uint8)
    p = m.Renderer._denoise_params((3, 3, 0.0))
    import ctypes as C
    rc = r.L.mirt_denoise_host(W, H, m.abi.ptr(rgba), None, 1, m.abi.ptr(planes["sphere"]), m.abi.ptr(planes["normal"]),
                               C.byref(p), m.abi.ptr(want), None)
    assert rc == 0
    same = []
    for tile in (0, 1):
        r.set_option(m.abi.OPT_DENOISE_TILE, tile)
        r.denoise(d_sphere, d_normal, rgba=d_rgba, params=(3, 3, 0.0), out=d_out, stream=stream)
        r.wait()
        same.append(bool(d_out.cpu().numpy().tobytes() == want.tobytes()))
    out["direct_equals_host"], out["tile_equals_host"] = same
    r.set_option(m.abi.OPT_DENOISE_TILE, default_tile)
    filtered, raw = r.render_frame_denoised(cam, W, H, raw=True, depth=5)
    out["frame_form_equals_host"] = bool(filtered.tobytes() == want.tobytes() and raw.tobytes() == rgba.tobytes())
    r.close()
    print(json.dumps(out))


def C_hip():
    """The HIP runtime already in the process (torch's), for the copy arm."""
    import ctypes as C
    lib = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.hipMemcpyAsync.restype = C.c_int
    return lib


if __name__ == "__main__":
    main()

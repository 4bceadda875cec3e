"""What the reprojection costs (mirt_reproject_device,
mirt_render_frame_reprojected: csrc/reproject.h) at 1080p, 10k spheres, depth
5. The arms run interleaved in one process; each figure is the median over
--rounds rounds of the median of --calls calls, host clock from the call to the
stream idle. Prints one JSON line.

  reproject_t{1,4}   mirt_reproject_device of a one-sample frame resident in
                     HBM from the frame of a camera one MOVE_SPEED step to the
                     left, records and planes resident too, display and float
                     output both written, with one tap and with four
  reproject_first    the same without a previous frame
  denoise_p3         mirt_denoise_device, 3 passes with normals, of the same frame
  chain              reproject (four taps, float output) then mirt_denoise_device
                     on out_rgb with frames = 1, 3 passes with normals
  frame_hbm          mirt_render_frame_device, the frame left in HBM
  frame_planes_hbm   mirt_render_frame_planes_device storing t and sphere, likewise
  host_plain         mirt_render_frame, blocking, into pageable host memory
  host_planes        mirt_render_frame_planes (t, sphere), blocking, into
                     pageable host memory
  host_reprojected[_raw]
                     mirt_render_frame_reprojected, blocking, the camera
                     stepping right and left, into pageable host memory
  host_denoised      mirt_render_frame_denoised, blocking, likewise

and checks that both tap counts give the host form's bytes at this size.

  python scripts/reproject_time.py [--spheres 10000] [--rounds 5] [--calls 7]
"""
import argparse
import ctypes as C
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
    W, H = a.width, a.height
    s = m.create_random_spheres(a.spheres, 1)
    b = m.build_bvh(s)
    r = m.Renderer(0)
    r.upload(s, b)
    prev_cam, cam = m.default_camera(), m.default_camera()
    cam.position.x += 0.5 * cam.right.x   # one MOVE_SPEED step along `right`
    dev = torch.device("cuda", 0)
    stream = r.stream_handle
    prev_rgba, prev_pl = r.render_frame_planes(prev_cam, W, H, planes=("t", "sphere"), depth=5, sample=0)
    rgba, pl = r.render_frame_planes(cam, W, H, depth=5, sample=1)
    hist = np.zeros((H, W), m.abi.HISTORY)
    for ch, f in enumerate("rgb"):
        hist[f] = prev_rgba[..., ch].astype(np.float32) / np.float32(255.0)
    hist["n"] = 1
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_rgba, d_t, d_sphere, d_normal = up(rgba), up(pl["t"]), up(pl["sphere"]), up(pl["normal"])
    d_hist = up(hist.view(np.float32).reshape(H, W, 4))
    d_tp, d_sp = up(prev_pl["t"]), up(prev_pl["sphere"])
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    d_den = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    out = {"workload": f"{W}x{H}, {a.spheres} spheres, depth 5", "rounds": a.rounds, "calls": a.calls}
    prev = (prev_cam, d_hist, d_tp, d_sp)
    state = {}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def reproject(taps, with_prev=True):
        def call():
            state["rp"] = r.reproject(cam, d_rgba, d_t, d_sphere, prev=prev if with_prev else None,
                                      params=(64, taps, 0.015625), rgb=True, out=d_out, stream=stream)
            r.wait()
        return lambda: timed(call)

    def denoise():
        r.denoise(d_sphere, d_normal, rgba=d_rgba, params=(3, 3, 0.0), out=d_den, stream=stream)
        r.wait()

    def chain():
        _, _, rgb = r.reproject(cam, d_rgba, d_t, d_sphere, prev=prev, rgb=True, out=d_out, stream=stream)
        r.denoise(d_sphere, d_normal, accum=rgb, frames=1, params=(3, 3, 0.0), out=d_den, stream=stream)
        r.wait()

    d_frame = torch.zeros(W * H, dtype=torch.int32, device=dev)
    d_pt = torch.zeros(W * H, dtype=torch.float32, device=dev)
    d_ps = torch.zeros(W * H, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def frame_hbm(c, k):
        r.render_frame_device(c, m.frame_desc(W, H, depth=5, sample=k), d_frame.data_ptr(), stream=stream)
        r.wait()

    def frame_planes_hbm(c, k):
        r.render_frame_planes_device(c, m.frame_desc(W, H, depth=5, sample=k), d_frame.data_ptr(),
                                     {"t": d_pt.data_ptr(), "sphere": d_ps.data_ptr()}, stream=stream)
        r.wait()

    step = {"k": 0}

    def moving(fn):
        def call():
            step["k"] += 1
            fn(cam if step["k"] & 1 else prev_cam, step["k"])
        return lambda: timed(call)

    arms = {"reproject_t1": reproject(1), "reproject_t4": reproject(4), "reproject_first": reproject(4, False),
            "denoise_p3": lambda: timed(denoise), "chain": lambda: timed(chain),
            "frame_hbm": moving(frame_hbm), "frame_planes_hbm": moving(frame_planes_hbm),
            "host_plain": moving(lambda c, k: r.render_frame(c, W, H, depth=5, sample=k)),
            "host_planes": moving(lambda c, k: r.render_frame_planes(c, W, H, planes=("t", "sphere"), depth=5,
                                                                     sample=k)),
            "host_reprojected": moving(lambda c, k: r.render_frame_reprojected(c, W, H, depth=5, sample=k)),
            "host_reprojected_raw": moving(lambda c, k: r.render_frame_reprojected(c, W, H, raw=True, depth=5,
                                                                                   sample=k)),
            "host_denoised": moving(lambda c, k: r.render_frame_denoised(c, W, H, depth=5, sample=k))}
    for fn in arms.values():
        fn()
    per = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():   # interleaved: every arm once per round
            per[k].append(statistics.median(fn() for _ in range(a.calls)))
    for k, v in per.items():
        out[f"{k}_ms"] = round(statistics.median(v), 4)
        out[f"{k}_ms_spread"] = [round(min(v), 4), round(max(v), 4)]
    out["chain_over_denoise_p3"] = round(out["chain_ms"] / out["denoise_p3_ms"], 4)
    out["host_reprojected_over_host_planes"] = round(out["host_reprojected_ms"] / out["host_planes_ms"], 4)
    out["history"] = r.history_stats()

    # both tap counts give the host form's bytes
    ptr = m.abi.ptr
    for taps in (1, 4):
        p = m.Renderer._reproject_params((64, taps, 0.015625))
        want_h, want_o = np.zeros((H, W), m.abi.HISTORY), np.zeros((H, W, 4), np.uint8)
        want_rgb = np.zeros((H, W, 3), np.float32)
        rc = r.L.mirt_reproject_host(W, H, C.byref(cam), C.byref(prev_cam), ptr(rgba), ptr(pl["t"]), ptr(pl["sphere"]),
                                     ptr(hist), ptr(prev_pl["t"]), ptr(prev_pl["sphere"]), C.byref(p), ptr(want_h),
                                     ptr(want_o), ptr(want_rgb))
        assert rc == 0
        arms[f"reproject_t{taps}"]()
        got_h, got_o, got_rgb = (x.cpu().numpy() for x in state["rp"])
        out[f"t{taps}_equals_host"] = bool(got_h.tobytes() == want_h.tobytes() and got_o.tobytes() == want_o.tobytes()
                                           and got_rgb.tobytes() == want_rgb.tobytes())
        out[f"t{taps}_reused_share"] = round(float((want_h["n"] > 1).sum()) / max(1, int((pl["sphere"] >= 0).sum())), 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

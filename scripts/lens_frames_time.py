"""What a lens frame costs (mirt_render_lens_frame*: the thin lens computed in
the frame's own camera pass), against the ray frame of the same rays, the plain
pinhole frame, and the route a depth-of-field loop had before it. 1080p, 10k
spheres by default (--spheres 100000 for the larger scene), depth 5 and depth 1;
the arms run interleaved in one process, each figure is the median over
--rounds rounds of the median of --calls calls. Prints one JSON line.

  plain      mirt_render_frame_device, the frame left in HBM (call to stream idle)
  rays       mirt_render_rays_device of mirt_lens_rays' output, resident in HBM
  lens       mirt_render_lens_frame_device, the frame left in HBM
  host_rays  mirt_render_rays from host rays into pageable host memory: what a
             depth-of-field loop did per frame (the rays already made)
  host_lens  mirt_render_lens_frame into pageable host memory
  host_plain mirt_render_frame into pageable host memory

The device arms also give the camera pass and the bounce pass of depth 5
(mirt_last_phase_ms). Then the accumulating loop, every frame delivered to
page-locked host memory, milliseconds per frame over --loop frames:

  multi4_*   mirt_multi on one device, 4 lanes, one frame per launch
  async3_*   three rotated contexts on one accumulation buffer, _async

  python scripts/lens_frames_time.py [--spheres 10000] [--rounds 5] [--calls 7] [--loop 120] [--sample 0]

A single ray with a direction component of a few 1e-8 can double the per-lane
camera walk's time at 100k spheres: sample 0 at 1080p has one,
sample 1 none, which is what --sample is for.
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
LENS = (0.5, 50.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--loop", type=int, default=120)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, default=10000)
    ap.add_argument("--sample", type=int, default=0, help="RNG sample of the single-frame arms (the lens's re-sampling)")
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
    rays = r.lens_rays(cam, LENS, W, H, sample=a.sample)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = r.stream_handle
    out = {"workload": f"{W}x{H}, {a.spheres} spheres", "lens": LENS, "sample": a.sample, "rounds": a.rounds, "calls": a.calls,
           "loop_frames": a.loop}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def rounds(arms):
        """{arm: callable returning a tuple of ms} -> {arm: (medians over rounds of the per-round medians,
        the per-round medians of the first figure)}"""
        for fn in arms.values():
            fn()
        per = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():   # interleaved: every arm once per round
                vals = [fn() for _ in range(a.calls)]
                per[k].append(tuple(statistics.median(c) for c in zip(*vals)))
        return {k: (tuple(round(statistics.median(c), 4) for c in zip(*v)), [round(x[0], 4) for x in v])
                for k, v in per.items()}

    for depth in (5, 1):
        fd = m.frame_desc(W, H, depth=depth, sample=a.sample)

        def device(name):
            def call():
                if name == "plain":
                    r.render_frame_device(cam, fd, d_out.data_ptr(), stream=stream)
                elif name == "rays":
                    r.render_rays_device(d_rays.data_ptr(), fd, d_out.data_ptr(), stream=stream)
                else:
                    r.render_lens_frame_device(cam, LENS, fd, d_out.data_ptr(), stream=stream)
                r.wait()

            def run():
                ms = timed(call)
                return (ms,) + r.last_phase_ms() if depth >= 2 else (ms,)
            return run

        res = rounds({"plain": device("plain"), "rays": device("rays"), "lens": device("lens"),
                      "host_plain": lambda: (timed(lambda: r.render_frame(cam, W, H, depth=depth, sample=a.sample)),),
                      "host_rays": lambda: (timed(lambda: r.render_rays(rays, W, H, depth=depth, sample=a.sample)),),
                      "host_lens": lambda: (timed(lambda: r.render_lens_frame(cam, LENS, W, H, depth=depth, sample=a.sample)),)})
        for k, (v, per_round) in res.items():
            out[f"d{depth}_{k}_ms"] = v[0]
            if k in ("rays", "lens"):
                out[f"d{depth}_{k}_ms_rounds"] = per_round
            if len(v) == 3:
                out[f"d{depth}_{k}_camera_pass_ms"], out[f"d{depth}_{k}_bounce_pass_ms"] = v[1], v[2]
        out[f"d{depth}_lens_over_rays"] = round(res["lens"][0][0] / res["rays"][0][0], 4)
        out[f"d{depth}_host_rays_over_host_lens"] = round(res["host_rays"][0][0] / res["host_lens"][0][0], 3)
    # the lens frame is the ray frame of its rays
    fd = m.frame_desc(W, H, depth=5, sample=a.sample)
    r.render_rays_device(d_rays.data_ptr(), fd, d_out.data_ptr(), stream=stream)
    r.wait()
    want = d_out.cpu().numpy().copy()
    r.render_lens_frame_device(cam, LENS, fd, d_out.data_ptr(), stream=stream)
    r.wait()
    out["lens_equals_rays"] = bool(d_out.cpu().numpy().tobytes() == want.tobytes())

    # ---- the accumulating loop, every frame delivered
    F = a.loop

    def loop_fd(k):
        return m.frame_desc(W, H, depth=5, seed=1, sample=k, accumulate=k > 0, frames=k + 1)

    def multi_loop(lens):
        bufs = [m.HostBuffer((H, W, 4)) for _ in range(4)]
        try:
            with m.MultiRenderer([0], lanes=4) as mr:
                mr.upload(s, b)

                def run():
                    for k in range(F):
                        if lens:
                            mr.render_lens_frames_async(cam, LENS, loop_fd(k), [bufs[k % 4]])
                        else:
                            mr.render_frame_async(cam, loop_fd(k), bufs[k % 4])
                    mr.wait()
                run()
                return [timed(run) / F for _ in range(a.rounds)], bufs[(F - 1) % 4].array.copy()
        finally:
            for x in bufs:
                x.close()

    def async_loop(lens):
        rs = [m.Renderer(0) for _ in range(3)]
        bufs = [m.HostBuffer((H, W, 4)) for _ in rs]
        try:
            for x in rs:
                x.upload(s, b)
                x.share_accum(rs[0])

            def run():
                for k in range(F):
                    x = rs[k % 3]
                    x.wait()
                    if lens:
                        x.render_lens_frame_async(cam, LENS, loop_fd(k), bufs[k % 3])
                    else:
                        x.render_frame_async(cam, loop_fd(k), bufs[k % 3])
                for x in rs:
                    x.wait()
            run()
            return [timed(run) / F for _ in range(a.rounds)], bufs[(F - 1) % 3].array.copy()
        finally:
            for x in bufs:
                x.close()
            for x in rs:
                x.close()

    last = {}
    for name, fn in (("multi4", multi_loop), ("async3", async_loop)):
        per = {"plain": [], "lens": []}
        for lens in (False, True, False, True):   # interleaved: each arm twice
            ms, last[name, lens] = fn(lens)
            per["lens" if lens else "plain"] += ms
        for k, v in per.items():
            out[f"{name}_{k}_ms_per_frame"] = round(statistics.median(v), 4)
            out[f"{name}_{k}_ms_per_frame_spread"] = [round(min(v), 4), round(max(v), 4)]
    out["loops_agree"] = bool(last["multi4", True].tobytes() == last["async3", True].tobytes()
                              and last["multi4", False].tobytes() == last["async3", False].tobytes())
    out["host_rays_loop_over_multi4_lens"] = round(out["d5_host_rays_ms"] / out["multi4_lens_ms_per_frame"], 2)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

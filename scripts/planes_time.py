"""What the primary-hit planes of a frame cost (mirt_render_frame_planes*),
against the frame without them and against the route they replace. 1080p /
10k spheres (bench.py's workload), depth 5 and depth 1; the arms of a
comparison run interleaved, each figure is the median over --rounds rounds of
the median of --calls calls. Prints one JSON line.

  (a) device  the frame left in HBM (mirt_render_frame[_planes]_device on the
              ctx's stream, call to stream idle): plain, t | sphere, all three
              planes; and the camera pass alone (mirt_last_phase_ms, depth 5)
  (b) pinned  the blocking frame into page-locked memory: plain against
              t | sphere (the planes copied behind the frame)
  (c) route   what a caller did before: a plain frame, then mirt_camera_rays
              and mirt_intersect_rays host to host; and the intersect kernel
              alone (mirt_last_kernel_ms)

  python scripts/planes_time.py [--rounds 5] [--calls 11]
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
    ap.add_argument("--calls", type=int, default=11)
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
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d = {"t": torch.zeros(n, dtype=torch.float32, device=dev), "sphere": torch.zeros(n, dtype=torch.int32, device=dev),
         "normal": torch.zeros(3 * n, dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    stream = r.stream_handle
    out = {"workload": f"{W}x{H}, {a.spheres} spheres", "rounds": a.rounds, "calls": a.calls}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def rounds(arms):
        """{arm: callable returning ms or a tuple of ms} -> {arm: median over rounds of the per-round medians}"""
        for fn in arms.values():
            fn()
        per = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():   # interleaved: every arm once per round
                vals = [fn() for _ in range(a.calls)]
                cols = list(zip(*vals)) if isinstance(vals[0], tuple) else [vals]
                per[k].append(tuple(statistics.median(c) for c in cols))
        return {k: tuple(round(statistics.median(c), 4) for c in zip(*v)) for k, v in per.items()}

    hb = m.HostBuffer((H, W, 4))
    h_t, h_s = m.HostBuffer((H, W), np.float32), m.HostBuffer((H, W), np.int32)
    ts = m.abi.PrimaryPlanes(h_t.array.ctypes.data, h_s.array.ctypes.data, None)
    for depth in (5, 1):
        fd = m.frame_desc(W, H, depth=depth)

        def device(names):
            def run():
                def call():
                    if names:
                        r.render_frame_planes_device(cam, fd, d_out.data_ptr(), {k: d[k].data_ptr() for k in names},
                                                     stream=stream)
                    else:
                        r.render_frame_device(cam, fd, d_out.data_ptr(), stream=stream)
                    r.wait()
                ms = timed(call)
                return (ms, r.last_phase_ms()[0]) if depth >= 2 else (ms,)
            return run

        res = rounds({"plain": device(()), "t_sphere": device(("t", "sphere")), "all": device(("t", "sphere", "normal"))})
        for k, v in res.items():
            out[f"d{depth}_device_{k}_ms"] = v[0]
            if depth >= 2:
                out[f"d{depth}_device_{k}_camera_pass_ms"] = v[1]

        def pinned_planes():
            rc = r.L.mirt_render_frame_planes(r.h, C.byref(cam), C.byref(fd), m.abi.ptr(hb.array), C.byref(ts))
            assert rc == 0, r.L.mirt_last_error()

        res = rounds({"plain": lambda: (timed(lambda: r.render_frame_into(cam, W, H, hb.array, depth=depth)),),
                      "t_sphere": lambda: (timed(pinned_planes),)})
        for k, v in res.items():
            out[f"d{depth}_pinned_{k}_ms"] = v[0]

        kernel = []

        def route():
            r.render_frame_into(cam, W, H, hb.array, depth=depth)
            hits = r.closest_hit(r.get_camera_rays(cam, W, H).reshape(-1))
            kernel.append(r.last_kernel_ms)
            return hits

        res = rounds({"route": lambda: (timed(route),)})
        out[f"d{depth}_route_ms"] = res["route"][0]
        out[f"d{depth}_route_intersect_kernel_ms"] = round(statistics.median(kernel), 4)
        # the case for fusing: t | sphere left in HBM against the plain frame plus the intersect kernel alone
        fused, apart = out[f"d{depth}_device_t_sphere_ms"], out[f"d{depth}_device_plain_ms"] + out[
            f"d{depth}_route_intersect_kernel_ms"]
        out[f"d{depth}_fused_vs_frame_plus_intersect_kernel"] = [fused, round(apart, 4), bool(fused < apart)]
    # what came back is what the route gives
    hits = r.closest_hit(r.get_camera_rays(cam, W, H).reshape(-1))
    r.render_frame_planes_device(cam, m.frame_desc(W, H, depth=5), d_out.data_ptr(),
                                 {k: v.data_ptr() for k, v in d.items()}, stream=stream)
    r.wait()
    out["planes_equal_route"] = bool(
        d["t"].cpu().numpy().tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
        and d["sphere"].cpu().numpy().tobytes() == np.ascontiguousarray(hits["sphere"]).tobytes()
        and d["normal"].cpu().numpy().tobytes() == np.ascontiguousarray(hits["normal"]).tobytes())
    for x in (hb, h_t, h_s):
        x.close()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

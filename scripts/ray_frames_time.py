"""What a ray frame costs (mirt_render_rays*: a frame from caller-given camera
rays), against the plain frame of the same rays and against the route it
replaces. 1080p, 10k spheres by default (--spheres 100000 for the larger
scene), depth 5 and depth 1; the arms run interleaved, each figure is the
median over --rounds rounds of the median of --calls calls. Prints one JSON line.

  plain     mirt_render_frame_device, the frame left in HBM (call to stream idle)
  pinhole   mirt_render_rays_device of the same pinhole rays, resident in HBM
  lens      mirt_render_rays_device of a thin-lens ray set (disc of radius 0.5,
            focal plane through the scene's centre), resident in HBM
  ortho     mirt_render_rays_device of an orthographic camera's rays (direction
            exactly (0, 0, -1): every ray has zero components), resident in HBM
  route     what a caller did before: mirt_trace_rays host to host on
            width * height rays
  blocking  mirt_render_rays from host rays into pageable host memory

The device arms also give the camera pass and the bounce pass of depth 5
(mirt_last_phase_ms).

  python scripts/ray_frames_time.py [--spheres 10000] [--rounds 5] [--calls 7]
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


def thin_lens(m, cam, pin, radius=0.5, focal=50.0, seed=1):
    """Thin-lens rays over the pinhole rays `pin`: origins on a disc about the
    camera, normalised directions through the pinhole ray's focal point."""
    rng = np.random.default_rng(seed)
    shape = pin.shape + (1,)
    right = np.array([cam.right.x, cam.right.y, cam.right.z], np.float32)
    up = np.array([cam.up.x, cam.up.y, cam.up.z], np.float32)
    focus = pin["origin"] + pin["direction"] * np.float32(focal)
    rad = np.float32(radius) * np.sqrt(rng.random(shape, np.float32))
    phi = np.float32(2 * np.pi) * rng.random(shape, np.float32)
    out = np.zeros(pin.shape, m.abi.RAY)
    out["origin"] = pin["origin"] + rad * (np.cos(phi) * right + np.sin(phi) * up)
    d = focus - out["origin"]
    out["direction"] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return out


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
    pin = r.get_camera_rays(cam, W, H)
    lens = thin_lens(m, cam, pin)
    ortho = np.zeros((H, W), m.abi.RAY)
    ortho["origin"][..., 0] = np.linspace(-60.0, 60.0, W, dtype=np.float32)[None, :]
    ortho["origin"][..., 1] = np.linspace(34.0, -34.0, H, dtype=np.float32)[:, None]
    ortho["origin"][..., 2] = 50.0
    ortho["direction"][..., 2] = -1.0
    d_rays = {k: torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).to(dev)
              for k, v in (("pinhole", pin), ("lens", lens), ("ortho", ortho))}
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = r.stream_handle
    out = {"workload": f"{W}x{H}, {a.spheres} spheres", "rounds": a.rounds, "calls": a.calls}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def rounds(arms):
        """{arm: callable returning a tuple of ms} -> {arm: median over rounds of the per-round medians}"""
        for fn in arms.values():
            fn()
        per = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():   # interleaved: every arm once per round
                vals = [fn() for _ in range(a.calls)]
                per[k].append(tuple(statistics.median(c) for c in zip(*vals)))
        return {k: tuple(round(statistics.median(c), 4) for c in zip(*v)) for k, v in per.items()}

    for depth in (5, 1):
        fd = m.frame_desc(W, H, depth=depth)

        def device(name):
            def call():
                if name == "plain":
                    r.render_frame_device(cam, fd, d_out.data_ptr(), stream=stream)
                else:
                    r.render_rays_device(d_rays[name].data_ptr(), fd, d_out.data_ptr(), stream=stream)
                r.wait()

            def run():
                ms = timed(call)
                return (ms,) + r.last_phase_ms() if depth >= 2 else (ms,)
            return run

        flat = {"pinhole": pin.reshape(-1), "lens": lens.reshape(-1)}
        res = rounds({"plain": device("plain"), "pinhole": device("pinhole"), "lens": device("lens"),
                      "ortho": device("ortho"),
                      "route_pinhole": lambda: (timed(lambda: r.trace_ray(flat["pinhole"], depth=depth)),),
                      "route_lens": lambda: (timed(lambda: r.trace_ray(flat["lens"], depth=depth)),),
                      "blocking_pinhole": lambda: (timed(lambda: r.render_rays(pin, W, H, depth=depth)),),
                      "blocking_lens": lambda: (timed(lambda: r.render_rays(lens, W, H, depth=depth)),)})
        for k, v in res.items():
            out[f"d{depth}_{k}_ms"] = v[0]
            if len(v) == 3:
                out[f"d{depth}_{k}_camera_pass_ms"], out[f"d{depth}_{k}_bounce_pass_ms"] = v[1], v[2]
        out[f"d{depth}_pinhole_over_plain"] = round(res["pinhole"][0] / res["plain"][0], 3)
        out[f"d{depth}_route_over_ray_frame_lens"] = round(res["route_lens"][0] / res["lens"][0], 2)
    # the pinhole ray frame is the plain frame, and the lens frame what the route gives
    fd = m.frame_desc(W, H, depth=5)
    r.render_frame_device(cam, fd, d_out.data_ptr(), stream=stream)
    r.wait()
    plain = d_out.cpu().numpy().copy()
    r.render_rays_device(d_rays["pinhole"].data_ptr(), fd, d_out.data_ptr(), stream=stream)
    r.wait()
    out["pinhole_equals_plain"] = bool(d_out.cpu().numpy().tobytes() == plain.tobytes())
    out["lens_equals_route"] = bool(r.render_rays(lens, W, H, depth=5).tobytes()
                                    == r.trace_ray(lens.reshape(-1), depth=5).tobytes())
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

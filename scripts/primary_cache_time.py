"""What the primary cache (MIRT_OPT_PRIMARY_CACHE) saves a still camera: frames
that are steady hits (option 1) against the same frames with the option at 0,
on the same ctx. 1080p, 10k and 100k spheres, depth 5 and depth 1; the arms of
a comparison run interleaved, each figure is the median over --rounds rounds of
the median of --calls calls; every timed shape is also compared byte for byte
once. Prints one JSON line.

  (a) device  the frame left in HBM (mirt_render_frame_device on the ctx's
              stream, call to stream idle): the whole frame and, at depth 5,
              the camera pass and the bounce pass apart (mirt_last_phase_ms).
              Arms: plain, hit; and fill against plain with the camera
              alternating between two positions in both (every frame of the
              fill arm misses: what a fill costs on top of the walk)
  (b) pinned  the blocking frame into page-locked memory: plain against hit
  (c) loop    the accumulating loop through mirt_multi, 4 lanes, every frame
              delivered into page-locked memory: ms per frame, plain against
              the option on (each lane fills once, then hits)

  python scripts/primary_cache_time.py [--rounds 5] [--calls 11] [--spheres 10000 100000]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--loop-frames", type=int, default=64)
    a = ap.parse_args()
    import torch   # before libmirt.so: one HIP runtime in the process
    m = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")
    OPT = m.abi.OPT_PRIMARY_CACHE
    W, H, n = a.width, a.height, a.width * a.height
    cam = m.default_camera()
    cam2 = m.default_camera()
    cam2.position.x += 0.01
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out = {"workload": f"{W}x{H}", "rounds": a.rounds, "calls": a.calls, "equal": True}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def rounds(arms):
        """{arm: (enter, call, leave)}: call returns a tuple of ms -> {arm: medians over rounds of per-round medians}"""
        per = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, (enter, call, leave) in arms.items():   # interleaved: every arm once per round
                enter()
                vals = [call() for _ in range(a.calls)]
                leave()
                per[k].append(tuple(statistics.median(c) for c in zip(*vals)))
        return {k: tuple(round(statistics.median(c), 4) for c in zip(*v)) for k, v in per.items()}

    for ns in a.spheres:
        r = m.Renderer(0)
        spheres = m.create_random_spheres(ns, 1)
        r.build_scene(spheres)
        stream = r.stream_handle
        hb = m.HostBuffer((H, W, 4))
        for depth in (5, 1):
            tag = f"{ns // 1000}k_d{depth}"
            fd = m.frame_desc(W, H, depth=depth)
            flip = [0]

            def device(cams):
                def call():
                    flip[0] += 1
                    c = cams[flip[0] % len(cams)]

                    def go():
                        r.render_frame_device(c, fd, d_out.data_ptr(), stream=stream)
                        r.wait()
                    ms = timed(go)
                    return (ms, *r.last_phase_ms()) if depth >= 2 else (ms,)
                return call

            def on(warm):
                def enter():
                    r.set_option(OPT, 1)
                    for c in warm:   # the fill, untimed
                        r.render_frame_device(c, fd, d_out.data_ptr(), stream=stream)
                    r.wait()
                return enter

            def off():
                r.set_option(OPT, 0)

            def expect(kind):
                def leave():
                    st = r.primary_cache_stats()
                    assert st["last"] == kind and st[kind + "s" if kind != "bypass" else "bypassed"] >= a.calls, st
                    r.set_option(OPT, 0)
                return leave

            res = rounds({"plain": (off, device([cam]), off), "hit": (on([cam]), device([cam]), expect("hit")),
                          "plain_alt": (off, device([cam, cam2]), off),
                          "fill_alt": (on([]), device([cam, cam2]), expect("fill"))})
            for k, v in res.items():
                out[f"{tag}_device_{k}_ms"] = v[0]
                if depth >= 2:
                    out[f"{tag}_device_{k}_camera_pass_ms"], out[f"{tag}_device_{k}_bounce_pass_ms"] = v[1], v[2]

            def pinned():
                return (timed(lambda: r.render_frame_into(cam, W, H, hb.array, depth=depth)),)

            res = rounds({"plain": (off, pinned, off), "hit": (on([cam]), pinned, expect("hit"))})
            for k, v in res.items():
                out[f"{tag}_pinned_{k}_ms"] = v[0]
            # the timed frames, once, byte for byte
            off()
            want = r.render_frame_into(cam, W, H, hb.array, depth=depth).copy()
            on([cam])()
            got = r.render_frame_into(cam, W, H, hb.array, depth=depth).copy()
            assert r.primary_cache_stats()["last"] == "hit"
            r.render_frame_device(cam, fd, d_out.data_ptr(), stream=stream)
            r.wait()
            off()
            out["equal"] = bool(out["equal"] and got.tobytes() == want.tobytes()
                                and d_out.cpu().numpy().tobytes() == want.tobytes())
        hb.close()
        r.close()

        # (c) the accumulating loop, frames in flight on four lanes
        with m.MultiRenderer([0], lanes=4) as mr:
            mr.build_scene(spheres)
            bufs = [m.HostBuffer((H, W, 4)) for _ in range(4)]
            K = a.loop_frames

            def loop():
                def go():
                    for k in range(K):
                        fdk = m.frame_desc(W, H, depth=5, sample=k, accumulate=k > 0, frames=k + 1)
                        mr.render_frame_async(cam, fdk, bufs[k % 4])
                    mr.wait()
                return (timed(go) / K,)

            frames = {}

            def keep(k):
                def leave():
                    frames[k] = bufs[(K - 1) % 4].array.tobytes()
                    mr.set_option(OPT, 0)
                return leave

            a_calls, a.calls = a.calls, 3
            res = rounds({"plain": (lambda: mr.set_option(OPT, 0), loop, keep("plain")),
                          "cache": (lambda: mr.set_option(OPT, 1), loop, keep("cache"))})
            a.calls = a_calls
            for k, v in res.items():
                out[f"{ns // 1000}k_loop4_{k}_ms_per_frame"] = v[0]
            out["equal"] = bool(out["equal"] and frames["plain"] == frames["cache"])
            for b in bufs:
                b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

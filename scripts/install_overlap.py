"""Does a scene install wait for a frame in flight on another member of its
group? Context B (sharing A's scene) gets a frame behind a bounded `--stall`
ms wait (MIRT_OPT_DEBUG_STALL_MS); the host then times the install through A.
An install that returns in its usual 1-2 ms overlaps; one that takes about the
stall waits for the device. One JSON line per call.

    python scripts/install_overlap.py [--stall 100] [--spheres 10000]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime in the process: torch's, as in bench.py)

mirt = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stall", type=int, default=100)
    ap.add_argument("--spheres", type=int, default=10000)
    a = ap.parse_args()
    n = a.spheres
    s = mirt.create_random_spheres(n, 1)
    tree = mirt.build_bvh(s)
    r = np.random.default_rng(1)
    s2 = s.copy()
    s2["center"] += r.normal(0.0, 0.5, (n, 3)).astype(np.float32)
    cam, fd = mirt.default_camera(), mirt.frame_desc(1920, 1080, depth=5, seed=1)
    hb = mirt.HostBuffer((1080, 1920, 4))
    calls = {
        "refit_scene": lambda A: A.refit_scene(s2),
        "update_scene max_decay 0": lambda A: A.update_scene(s2, 0, n, 0.0),
        "update_scene max_decay 1e-9": lambda A: A.update_scene(s2, 0, n, 1e-9),
        "build_scene": lambda A: A.build_scene(s2),
        "upload (host)": lambda A: A.upload(s, tree),
    }
    try:
        with mirt.Renderer(0) as A, mirt.Renderer(0) as B:
            B.share_scene(A)
            for name, call in calls.items():
                for stall in (0, a.stall):
                    A.upload(s, tree)
                    call(A)                                   # warm: scratch allocated
                    A.upload(s, tree)
                    B.set_option(mirt.abi.OPT_DEBUG_STALL_MS, stall)
                    B.render_frame_async(cam, fd, hb)
                    t0 = time.perf_counter()
                    call(A)
                    ms = (time.perf_counter() - t0) * 1e3
                    B.wait()
                    print(json.dumps({"call": name, "spheres": n, "frame_in_flight_stall_ms": stall,
                                      "call_ms": round(ms, 3)}), flush=True)
    finally:
        hb.close()


if __name__ == "__main__":
    main()

"""Host and device SAH build side by side on one machine, in one run.

    python scripts/build_time.py [--reps 5] [--shapes render:10000,render:100000,render:1000000,bench:1000000]

For every shape: one warm-up, then the median of `reps` runs of
mirt_bvh_build_flat (default threads; host wall clock around the call) and of
mirt_bvh_build_flat_device (total_ms: call to return, sphere H2D and node D2H
included; device_ms: HIP-event time of its kernels). Each run starts from a
fresh copy of the scene; the two builders' nodes and reordered spheres are
checked byte-equal. Render scenes are built as (0, n, 0), the benchmark scene
as benchmark.c:317 builds it, (0, n - 1, 20). One JSON line per shape.
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
import torch  # noqa: E402,F401  (one HIP runtime in the process: torch's, as in bench.py)

mirt = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="render:10000,render:100000,render:1000000,bench:1000000")
    a = ap.parse_args()
    L = mirt.load()
    with mirt.Renderer(0) as r:
        for shape in a.shapes.split(","):
            kind, n = shape.split(":")
            n = int(n)
            if kind == "render":
                scene, rng = mirt.create_random_spheres(n, 1), (0, n, 0)
            else:
                scene, rng = mirt.create_benchmark_spheres(n, 1), (0, n - 1, 20)
            host_ms, total_ms, device_ms = [], [], []
            stats = None
            for rep in range(a.reps + 1):          # rep 0: warm-up
                hs, ds = scene.copy(), scene.copy()
                out, cnt = C.c_void_p(), C.c_int()
                t0 = time.perf_counter()          # the C call alone, as total_ms is taken inside the C call
                rc = L.mirt_bvh_build_flat(mirt.abi.ptr(hs), *rng, C.byref(out), C.byref(cnt))
                t1 = time.perf_counter()
                if rc:
                    raise SystemExit(f"{shape}: mirt_bvh_build_flat failed ({rc}): {L.mirt_last_error().decode()}")
                buf = (C.c_char * (cnt.value * mirt.abi.NODE.itemsize)).from_address(out.value)
                hb = np.frombuffer(bytes(buf), dtype=mirt.abi.NODE)
                L.mirt_bvh_free_flat(out)
                db = r.build_bvh(ds, *rng).nodes
                stats = r.last_build_stats()
                if stats["on_device"] != 1:
                    raise SystemExit(f"{shape}: the device builder declined the scene")
                if hs.tobytes() != ds.tobytes() or hb.tobytes() != db.tobytes():
                    raise SystemExit(f"{shape}: host and device builds differ")
                if rep:
                    host_ms.append((t1 - t0) * 1e3)
                    total_ms.append(stats["total_ms"])
                    device_ms.append(stats["device_ms"])
            med = statistics.median
            print(json.dumps({
                "shape": shape, "range": list(rng), "nodes": stats["nodes"], "levels": stats["levels"],
                "reps": a.reps,
                "host_ms": round(med(host_ms), 3), "host_ms_min_max": [round(min(host_ms), 3), round(max(host_ms), 3)],
                "device_total_ms": round(med(total_ms), 3),
                "device_total_ms_min_max": [round(min(total_ms), 3), round(max(total_ms), 3)],
                "device_kernels_ms": round(med(device_ms), 3),
                "host_over_device_total": round(med(host_ms) / med(total_ms), 2),
                "byte_equal": True}), flush=True)


if __name__ == "__main__":
    main()

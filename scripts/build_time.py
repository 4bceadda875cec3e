"""Host and device SAH build side by side on one machine, in one run.

    python scripts/build_time.py [--reps 5] [--shapes render:10000,render:100000,render:1000000,bench:1000000]

For every shape: one warm-up, then the median of `reps` runs of
mirt_bvh_build_flat (default threads; host wall clock around the call) and of
mirt_bvh_build_flat_device (total_ms: call to return, sphere H2D and node D2H
included; device_ms: HIP-event time of its kernels). Each run starts from a
fresh copy of the scene; the two builders' nodes and reordered spheres are
checked byte-equal. Render scenes are built as (0, n, 0), the benchmark scene
as benchmark.c:317 builds it, (0, n - 1, 20). One JSON line per shape.

--finish 0,16,32,64 (the default) times the device build once per value of
MIRT_OPT_BUILD_FINISH, the arms interleaved within every rep; each arm reports
its totals, its kernels and the finish's own two passes (finish_ms, round,
subtrees). A library without the option (MIRT_LIB: an older build under A/B)
runs one arm, "none".
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
    ap.add_argument("--finish", default="0,16,32,64", help="MIRT_OPT_BUILD_FINISH values, one arm each")
    a = ap.parse_args()
    L = mirt.load()
    arms = [int(f) for f in a.finish.split(",")] if hasattr(L, "mirt_last_build_finish") else [None]
    with mirt.Renderer(0) as r:
        for shape in a.shapes.split(","):
            kind, n = shape.split(":")
            n = int(n)
            if kind == "render":
                scene, rng = mirt.create_random_spheres(n, 1), (0, n, 0)
            else:
                scene, rng = mirt.create_benchmark_spheres(n, 1), (0, n - 1, 20)
            host_ms = []
            total_ms, device_ms, finish_ms = ({f: [] for f in arms} for _ in range(3))
            stats, fin = {}, {}
            for rep in range(a.reps + 1):          # rep 0: warm-up
                hs = scene.copy()
                out, cnt = C.c_void_p(), C.c_int()
                t0 = time.perf_counter()          # the C call alone, as total_ms is taken inside the C call
                rc = L.mirt_bvh_build_flat(mirt.abi.ptr(hs), *rng, C.byref(out), C.byref(cnt))
                t1 = time.perf_counter()
                if rc:
                    raise SystemExit(f"{shape}: mirt_bvh_build_flat failed ({rc}): {L.mirt_last_error().decode()}")
                buf = (C.c_char * (cnt.value * mirt.abi.NODE.itemsize)).from_address(out.value)
                hb = np.frombuffer(bytes(buf), dtype=mirt.abi.NODE)
                L.mirt_bvh_free_flat(out)
                if rep:
                    host_ms.append((t1 - t0) * 1e3)
                for f in arms:
                    ds = scene.copy()
                    if f is not None:
                        r.set_option(mirt.abi.OPT_BUILD_FINISH, f)
                    db = r.build_bvh(ds, *rng).nodes
                    stats[f] = r.last_build_stats()
                    fin[f] = r.last_build_finish() if f is not None else {"finish_ms": 0.0, "round": -1, "subtrees": 0}
                    if stats[f]["on_device"] != 1:
                        raise SystemExit(f"{shape}: the device builder declined the scene")
                    if hs.tobytes() != ds.tobytes() or hb.tobytes() != db.tobytes():
                        raise SystemExit(f"{shape}: host and device builds differ (finish {f})")
                    if rep:
                        total_ms[f].append(stats[f]["total_ms"])
                        device_ms[f].append(stats[f]["device_ms"])
                        finish_ms[f].append(fin[f]["finish_ms"])
            med = statistics.median
            row = {"shape": shape, "range": list(rng), "nodes": stats[arms[0]]["nodes"], "reps": a.reps,
                   "host_ms": round(med(host_ms), 3), "host_ms_min_max": [round(min(host_ms), 3), round(max(host_ms), 3)],
                   "byte_equal": True, "arms": {}}
            for f in arms:
                row["arms"]["none" if f is None else str(f)] = {
                    "levels": stats[f]["levels"], "round": fin[f]["round"], "subtrees": fin[f]["subtrees"],
                    "device_total_ms": round(med(total_ms[f]), 3),
                    "device_total_ms_min_max": [round(min(total_ms[f]), 3), round(max(total_ms[f]), 3)],
                    "device_kernels_ms": round(med(device_ms[f]), 3),
                    "finish_ms": round(med(finish_ms[f]), 3),
                    "host_over_device_total": round(med(host_ms) / med(total_ms[f]), 2)}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

"""Spheres in, scene resident: the three ways to get there, side by side on one
machine, in one run.

    python scripts/scene_time.py [--reps 5] [--shapes render:10000,render:100000,render:1000000,bench:1000000]

For every shape: one warm-up, then the median of `reps` rounds. A round times,
interleaved, each on a fresh copy of the scene, host wall clock around the C
calls alone:
  A  mirt_bvh_build_flat        + mirt_scene_upload_flat
  B  mirt_bvh_build_flat_device + mirt_scene_upload_flat
  C  mirt_scene_build_device    (with the reordered spheres returned)
and, on A's tree, mirt_scene_upload_flat against mirt_scene_upload_flat_device.
After every path the context's resident layout is read back and compared,
byte for byte and scalar for scalar, with path A's of the same round (not
timed). C's build_ms / layout_ms split comes from mirt_scene_build_stats.
Render scenes are built as (0, n, 0), the benchmark scene as benchmark.c:317
builds it, (0, n - 1, 20). One JSON line per shape.

--finish 0,16,32,64 (the default) runs path C once per value of
MIRT_OPT_BUILD_FINISH in every round (C_f0_ms, C_f16_ms, ...: the call, its
build_ms and the finish's finish_ms); C itself and path B run under the
library's default. A library without the option (MIRT_LIB) runs no such arms.
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
abi = mirt.abi


def same_layout(a, b):
    (ia, pa), (ib, pb) = a, b
    for k in ia:
        x, y = ia[k], ib[k]
        if (np.float32(x).tobytes() != np.float32(y).tobytes()) if isinstance(x, float) else x != y:
            return f"info.{k}: {x!r} != {y!r}"
    for name in pa:
        if pa[name].shape != pb[name].shape or not np.array_equal(pa[name].view(np.uint8), pb[name].view(np.uint8)):
            return f"part {name}"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="render:10000,render:100000,render:1000000,bench:1000000")
    ap.add_argument("--finish", default="0,16,32,64", help="MIRT_OPT_BUILD_FINISH values, one arm of path C each")
    a = ap.parse_args()
    L = mirt.load()
    arms = [int(f) for f in a.finish.split(",")] if hasattr(L, "mirt_last_build_finish") else []
    p = abi.ptr
    clock = time.perf_counter

    def fail(shape, what, rc):
        raise SystemExit(f"{shape}: {what} failed ({rc}): {L.mirt_last_error().decode()}")

    with mirt.Renderer(0) as r:
        for shape in a.shapes.split(","):
            kind, n = shape.split(":")
            n = int(n)
            if kind == "render":
                scene, rng = mirt.create_random_spheres(n, 1), (0, n, 0)
            else:
                scene, rng = mirt.create_benchmark_spheres(n, 1), (0, n - 1, 20)
            t = {k: [] for k in ("A", "A_build", "A_upload", "B", "B_build", "B_upload", "C", "C_build", "C_layout",
                                 "upload_host", "upload_device")}
            for f in arms:
                t.update({f"C_f{f}": [], f"C_f{f}_build": [], f"C_f{f}_finish": []})
            stats = None
            for rep in range(a.reps + 1):          # rep 0: warm-up
                ms = {}
                # A: host build + host upload
                sa = scene.copy()
                out, cnt = C.c_void_p(), C.c_int()
                t0 = clock()
                rc = L.mirt_bvh_build_flat(p(sa), *rng, C.byref(out), C.byref(cnt))
                t1 = clock()
                if rc:
                    fail(shape, "mirt_bvh_build_flat", rc)
                rc = L.mirt_scene_upload_flat(r.h, p(sa), n, out, cnt.value)
                t2 = clock()
                if rc:
                    fail(shape, "mirt_scene_upload_flat", rc)
                ms["A"], ms["A_build"], ms["A_upload"] = t2 - t0, t1 - t0, t2 - t1
                ref = r.resident_layout()
                # the two uploads of A's tree
                t0 = clock()
                rc = L.mirt_scene_upload_flat_device(r.h, p(sa), n, out, cnt.value)
                t1 = clock()
                if rc:
                    fail(shape, "mirt_scene_upload_flat_device", rc)
                ms["upload_device"] = t1 - t0
                bad = same_layout(r.resident_layout(), ref)
                if bad:
                    raise SystemExit(f"{shape}: mirt_scene_upload_flat_device's layout differs from A's: {bad}")
                t0 = clock()
                rc = L.mirt_scene_upload_flat(r.h, p(sa), n, out, cnt.value)
                t1 = clock()
                if rc:
                    fail(shape, "mirt_scene_upload_flat", rc)
                ms["upload_host"] = t1 - t0
                L.mirt_bvh_free_flat(out)
                # B: device build + host upload
                sb = scene.copy()
                out, cnt = C.c_void_p(), C.c_int()
                t0 = clock()
                rc = L.mirt_bvh_build_flat_device(r.h, p(sb), *rng, C.byref(out), C.byref(cnt))
                t1 = clock()
                if rc:
                    fail(shape, "mirt_bvh_build_flat_device", rc)
                rc = L.mirt_scene_upload_flat(r.h, p(sb), n, out, cnt.value)
                t2 = clock()
                if rc:
                    fail(shape, "mirt_scene_upload_flat", rc)
                L.mirt_bvh_free_flat(out)
                ms["B"], ms["B_build"], ms["B_upload"] = t2 - t0, t1 - t0, t2 - t1
                if r.last_build_stats()["on_device"] != 1:
                    raise SystemExit(f"{shape}: the device builder declined the scene")
                bad = same_layout(r.resident_layout(), ref)
                if bad or sb.tobytes() != sa.tobytes():
                    raise SystemExit(f"{shape}: path B's scene differs from A's: {bad or 'spheres'}")
                # C: one call
                sc = scene.copy()
                reordered = np.zeros(n, abi.SPHERE)
                t0 = clock()
                rc = L.mirt_scene_build_device(r.h, p(sc), n, *rng, p(reordered))
                t1 = clock()
                if rc:
                    fail(shape, "mirt_scene_build_device", rc)
                ms["C"] = t1 - t0
                stats = r.last_scene_build_stats()
                if stats["on_device"] != 1:
                    raise SystemExit(f"{shape}: mirt_scene_build_device declined the scene")
                bad = same_layout(r.resident_layout(), ref)
                if bad or reordered.tobytes() != sa.tobytes() or sc.tobytes() != scene.tobytes():
                    raise SystemExit(f"{shape}: path C's scene differs from A's: {bad or 'spheres'}")
                # C again, once per finish setting
                for f in arms:
                    r.set_option(abi.OPT_BUILD_FINISH, f)
                    t0 = clock()
                    rc = L.mirt_scene_build_device(r.h, p(sc), n, *rng, p(reordered))
                    t1 = clock()
                    r.set_option(abi.OPT_BUILD_FINISH, 1)
                    if rc:
                        fail(shape, "mirt_scene_build_device", rc)
                    bad = same_layout(r.resident_layout(), ref)
                    if bad or reordered.tobytes() != sa.tobytes():
                        raise SystemExit(f"{shape}: path C's scene with finish {f} differs from A's: {bad or 'spheres'}")
                    ms[f"C_f{f}"] = t1 - t0
                    if rep:
                        t[f"C_f{f}_build"].append(r.last_scene_build_stats()["build_ms"])
                        t[f"C_f{f}_finish"].append(r.last_build_finish()["finish_ms"])
                if rep:
                    for k, v in ms.items():
                        t[k].append(v * 1e3)
                    t["C_build"].append(stats["build_ms"])
                    t["C_layout"].append(stats["layout_ms"])
                del ref
                print(f"{shape} round {rep}: A {ms['A'] * 1e3:.1f} B {ms['B'] * 1e3:.1f} C {ms['C'] * 1e3:.1f} ms",
                      file=sys.stderr, flush=True)
            med = statistics.median
            row = {"shape": shape, "range": list(rng), "nodes": stats["nodes"], "levels": stats["levels"],
                   "reps": a.reps, "layouts_byte_equal": True}
            for k, v in t.items():
                row[k + "_ms"] = round(med(v), 3)
                row[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            row["A_over_C"] = round(med(t["A"]) / med(t["C"]), 2)
            row["B_over_C"] = round(med(t["B"]) / med(t["C"]), 2)
            row["upload_host_over_device"] = round(med(t["upload_host"]) / med(t["upload_device"]), 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

"""The spheres of a resident scene have moved: refit against rebuild, side by
side on one machine, in one run.

    python scripts/refit_time.py [--reps 5] [--sigma 0.5] [--shapes render:10000,render:100000,render:1000000,bench:1000000]

For every shape the tree is built once (mirt_bvh_build_flat); then one
warm-up and the median of `reps` rounds. A round moves the spheres (centres +
N(0, sigma), radii x U(0.5, 1.5), another seed every round) and times,
interleaved, host wall clock around the C call alone, each call straight after
the original scene has been put back (mirt_scene_upload_flat_device, not
timed: the same resident scene and a device that is not idle in front of
every timed call -- the host-side checks between them take up to seconds):
  R  mirt_scene_refit_device      the moved spheres in host memory
  P  mirt_scene_refit_device_ptr  the moved spheres in a torch tensor on the device
  C  mirt_scene_build_device      on the moved spheres: the rebuild a refit replaces
After every call the context's resident layout is read back and compared, byte
for byte and scalar for scalar, with the host's (not timed): for R and P
mirt_scene_layout of mirt_bvh_refit_flat's tree, for C of mirt_bvh_build_flat's.
refit_ms / layout_ms and build_ms / layout_ms come from mirt_refit_stats and
mirt_scene_build_stats. Render scenes are built as (0, n, 0), the benchmark
scene as benchmark.c:317 builds it, (0, n - 1, 20). One JSON line per shape.
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
import torch  # noqa: E402  (one HIP runtime in the process: torch's, as in bench.py)

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


def moved(s, sigma, seed):
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(np.float32)
    out["radius"] *= r.uniform(0.5, 1.5, len(s)).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--shapes", default="render:10000,render:100000,render:1000000,bench:1000000")
    a = ap.parse_args()
    L = mirt.load()
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
            end = rng[1]
            s = scene.copy()
            nodes = mirt.build_bvh(s, *rng).nodes          # s: the scene's order from here on
            t = {k: [] for k in ("R", "R_refit", "R_layout", "P", "P_refit", "P_layout", "C", "C_build", "C_layout")}
            for rep in range(a.reps + 1):          # rep 0: warm-up
                s2 = moved(s, a.sigma, rep)
                want = mirt.scene_layout(s2, mirt.refit_bvh(nodes, s2, end))
                d2 = torch.from_numpy(s2.view(np.uint8).reshape(n, 20).copy()).to("cuda:0")
                torch.cuda.synchronize()
                ms = {}

                def original():
                    rc = L.mirt_scene_upload_flat_device(r.h, p(s), n, p(nodes), len(nodes))
                    if rc:
                        fail(shape, "mirt_scene_upload_flat_device", rc)

                original()
                # R: the moved spheres from host memory
                t0 = clock()
                rc = L.mirt_scene_refit_device(r.h, p(s2), n, end, None)
                t1 = clock()
                if rc:
                    fail(shape, "mirt_scene_refit_device", rc)
                st = r.last_refit_stats()
                ms["R"], ms["R_refit"], ms["R_layout"] = (t1 - t0) * 1e3, st["refit_ms"], st["layout_ms"]
                bad = same_layout(r.resident_layout(), want)
                if bad or st["on_device"] != 1:
                    raise SystemExit(f"{shape}: mirt_scene_refit_device's scene differs from the host's: "
                                     f"{bad or 'declined'}")
                # P: the moved spheres already on the device
                original()
                t0 = clock()
                rc = L.mirt_scene_refit_device_ptr(r.h, C.c_void_p(d2.data_ptr()), n, end, None)
                t1 = clock()
                if rc:
                    fail(shape, "mirt_scene_refit_device_ptr", rc)
                st = r.last_refit_stats()
                ms["P"], ms["P_refit"], ms["P_layout"] = (t1 - t0) * 1e3, st["refit_ms"], st["layout_ms"]
                bad = same_layout(r.resident_layout(), want)
                if bad or st["on_device"] != 1:
                    raise SystemExit(f"{shape}: mirt_scene_refit_device_ptr's scene differs from the host's: "
                                     f"{bad or 'declined'}")
                del want
                # C: the rebuild on the moved spheres
                reordered = np.zeros(n, abi.SPHERE)
                original()
                t0 = clock()
                rc = L.mirt_scene_build_device(r.h, p(s2), n, *rng, p(reordered))
                t1 = clock()
                if rc:
                    fail(shape, "mirt_scene_build_device", rc)
                sb = r.last_scene_build_stats()
                ms["C"], ms["C_build"], ms["C_layout"] = (t1 - t0) * 1e3, sb["build_ms"], sb["layout_ms"]
                host = s2.copy()
                rebuilt = mirt.build_bvh(host, *rng).nodes
                bad = same_layout(r.resident_layout(), mirt.scene_layout(host, rebuilt))
                if bad or sb["on_device"] != 1 or host.tobytes() != reordered.tobytes():
                    raise SystemExit(f"{shape}: mirt_scene_build_device's scene differs from the host's: "
                                     f"{bad or 'declined / spheres'}")
                if rep:
                    for k, v in ms.items():
                        t[k].append(v)
                print(f"{shape} round {rep}: R {ms['R']:.2f} (refit {ms['R_refit']:.2f} layout {ms['R_layout']:.2f}) "
                      f"P {ms['P']:.2f} C {ms['C']:.2f} (build {ms['C_build']:.2f} layout {ms['C_layout']:.2f}) ms",
                      file=sys.stderr, flush=True)
            med = statistics.median
            row = {"shape": shape, "range": list(rng), "nodes": len(nodes), "sigma": a.sigma, "reps": a.reps,
                   "layouts_byte_equal": True}
            for k, v in t.items():
                row[k + "_ms"] = round(med(v), 3)
                row[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            row["C_over_R"] = round(med(t["C"]) / med(t["R"]), 2)
            row["C_over_P"] = round(med(t["C"]) / med(t["P"]), 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

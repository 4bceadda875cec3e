"""What following the spheres' motion costs (mirt_reproject_motion_device,
MIRT_OPT_HISTORY_MOTION: csrc/reproject.h) at 1080p, depth 5.
The arms run interleaved in one process; each figure is the median over
--rounds rounds of the median of --calls calls, host clock from the call to the
stream idle. Prints one JSON line.

  plain_t{1,4}       mirt_reproject_device of a one-sample frame resident in
                     HBM, records and planes resident too, display and float
                     output both written
  motion_t{1,4}      mirt_reproject_motion_device of the same frame with the
                     motion of an update that rebuilt (every sphere moved, a
                     permutation), all of it resident
  refit_opt{0,1}     mirt_scene_update_device, max_decay 0 (the refit branch),
                     of diffusing spheres, the option off and on
  rebuild_opt{0,1}   the same with a max_decay every tree exceeds (the rebuild
                     branch)
  frame_history      mirt_render_frame_reprojected, blocking, of a scene that
                     stays: the history kept without a motion
  frame_first        the same with the history emptied before every call
  loop_opt{0,1}      update (refit branch) then mirt_render_frame_reprojected,
                     both blocking, in frames per second, and the two calls
                     apart

and checks that the motion form gives the host form's bytes at this size, and
how much of the frame reuses history with and without the link.

  python scripts/reproject_motion_time.py [--spheres 10000] [--rounds 5] [--calls 7]
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
    ap.add_argument("--sigma", type=float, default=0.1)
    a = ap.parse_args()
    import torch   # before libmirt.so: one HIP runtime in the process
    m = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")
    W, H, N = a.width, a.height, a.spheres
    OPT = m.abi.OPT_HISTORY_MOTION
    rng = np.random.default_rng(1)

    def diffused(s):
        out = s.copy()
        out["center"] += rng.normal(0.0, a.sigma, (len(s), 3)).astype(np.float32)
        return out

    def geo_now(r):
        return np.ascontiguousarray(r.resident_layout()[1]["geo"][:N])

    s = m.create_random_spheres(N, 1)
    b = m.build_bvh(s)
    r = m.Renderer(0)
    r.upload(s, b)
    cam = m.default_camera()
    dev = torch.device("cuda", 0)
    stream = r.stream_handle
    out = {"workload": f"{W}x{H}, {N} spheres, depth 5, sigma {a.sigma}", "rounds": a.rounds, "calls": a.calls}

    # ---- the kernels: a frame of the scene, an update that rebuilds, a frame of the new scene
    prev_rgba, prev_pl = r.render_frame_planes(cam, W, H, planes=("t", "sphere"), depth=5, sample=0)
    geo_prev = geo_now(r)
    held, perm, res = r.update_scene(diffused(s), 0, N, 1e-3)
    assert res["rebuilt"] == 1
    geo = geo_now(r)
    rgba, pl = r.render_frame_planes(cam, W, H, planes=("t", "sphere"), depth=5, sample=1)
    hist = np.zeros((H, W), m.abi.HISTORY)
    for ch, f in enumerate("rgb"):
        hist[f] = prev_rgba[..., ch].astype(np.float32) / np.float32(255.0)
    hist["n"] = 1
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_rgba, d_t, d_sphere = up(rgba), up(pl["t"]), up(pl["sphere"])
    d_hist = up(hist.view(np.float32).reshape(H, W, 4))
    d_tp, d_sp = up(prev_pl["t"]), up(prev_pl["sphere"])
    d_motion = (up(geo), up(geo_prev), up(perm))
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    prev = (cam, d_hist, d_tp, d_sp)
    state = {}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def reproject(taps, motion):
        def call():
            state["rp"] = r.reproject(cam, d_rgba, d_t, d_sphere, prev=prev, params=(64, taps, 0.015625), rgb=True,
                                      out=d_out, stream=stream, motion=d_motion if motion else None)
            r.wait()
        return lambda: timed(call)

    # ---- the installs and the loop: ctxs of their own, the option off and on
    ctx = {}
    for opt in (0, 1):
        c = m.Renderer(0)
        c.upload(s, b)
        c.set_option(OPT, opt)
        c.update_scene(s, 0, N, 0.0)   # (the base cost is this call's from here on)
        ctx[opt] = {"r": c, "held": s, "k": 0}

    def update(opt, max_decay):
        def call():
            st = ctx[opt]
            moved = diffused(st["held"])
            t0 = time.perf_counter()
            st["held"], _, res = st["r"].update_scene(moved, 0, N, max_decay)
            ms = (time.perf_counter() - t0) * 1e3
            assert res["on_device"] == 1 and res["rebuilt"] == int(max_decay > 0), res
            return ms
        return call

    def loop(opt):
        def call():
            st = ctx[opt]
            moved = diffused(st["held"])
            st["k"] += 1
            t0 = time.perf_counter()
            st["held"], _, _ = st["r"].update_scene(moved, 0, N, 0.0)
            t1 = time.perf_counter()
            st["r"].render_frame_reprojected(cam, W, H, depth=5, sample=st["k"])
            t2 = time.perf_counter()
            parts[opt].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            return (t2 - t0) * 1e3
        return call

    parts = {0: [], 1: []}
    tick = {"k": 0}

    def frame(first):
        """mirt_render_frame_reprojected of a scene that stays, with the history kept (plain) or emptied first."""
        def call():
            tick["k"] += 1
            if first:
                r.history_reset()
            r.render_frame_reprojected(cam, W, H, depth=5, sample=tick["k"])
        return lambda: timed(call)

    arms = {"plain_t1": reproject(1, False), "motion_t1": reproject(1, True), "plain_t4": reproject(4, False),
            "motion_t4": reproject(4, True), "refit_opt0": update(0, 0.0), "refit_opt1": update(1, 0.0),
            "rebuild_opt0": update(0, 1e-3), "rebuild_opt1": update(1, 1e-3), "loop_opt0": loop(0),
            "loop_opt1": loop(1), "frame_history": frame(False), "frame_first": frame(True)}
    for fn in arms.values():
        fn()
    per = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():   # interleaved: every arm once per round
            per[k].append(statistics.median(fn() for _ in range(a.calls)))
    for k, v in per.items():
        out[f"{k}_ms"] = round(statistics.median(v), 4)
        out[f"{k}_ms_spread"] = [round(min(v), 4), round(max(v), 4)]
    for taps in (1, 4):
        out[f"motion_over_plain_t{taps}"] = round(out[f"motion_t{taps}_ms"] / out[f"plain_t{taps}_ms"], 4)
    for k in ("refit", "rebuild"):
        out[f"{k}_link_ms"] = round(out[f"{k}_opt1_ms"] - out[f"{k}_opt0_ms"], 4)
        out[f"{k}_opt1_over_opt0"] = round(out[f"{k}_opt1_ms"] / out[f"{k}_opt0_ms"], 4)
    for opt in (0, 1):
        out[f"loop_opt{opt}_fps"] = round(1e3 / out[f"loop_opt{opt}_ms"], 2)
        # the loop's two calls apart: medians over every iteration
        out[f"loop_opt{opt}_update_ms"] = round(statistics.median(u for u, _ in parts[opt]), 4)
        out[f"loop_opt{opt}_frame_ms"] = round(statistics.median(f for _, f in parts[opt]), 4)
        st = ctx[opt]["r"].history_stats()
        hit = st["reused"] + st["fresh"]
        out[f"loop_opt{opt}_reused_share"] = round(st["reused"] / max(1, hit), 4)
        out[f"loop_opt{opt}_frames"] = st["frames"]
    out["link"] = ctx[1]["r"].history_motion()

    # the motion form gives the host form's bytes
    ptr = m.abi.ptr
    for taps in (1, 4):
        p = m.Renderer._reproject_params((64, taps, 0.015625))
        want_h, want_o = np.zeros((H, W), m.abi.HISTORY), np.zeros((H, W, 4), np.uint8)
        want_rgb = np.zeros((H, W, 3), np.float32)
        perm = np.ascontiguousarray(perm, np.int32)
        mo = m.abi.SphereMotion(geo.ctypes.data, geo_prev.ctypes.data, perm.ctypes.data, N, N)
        rc = r.L.mirt_reproject_motion_host(W, H, C.byref(cam), C.byref(cam), ptr(rgba), ptr(pl["t"]),
                                            ptr(pl["sphere"]), ptr(hist), ptr(prev_pl["t"]), ptr(prev_pl["sphere"]),
                                            C.byref(p), ptr(want_h), ptr(want_o), ptr(want_rgb), C.byref(mo))
        assert rc == 0
        arms[f"motion_t{taps}"]()
        got_h, got_o, got_rgb = (x.cpu().numpy() for x in state["rp"])
        out[f"t{taps}_equals_host"] = bool(got_h.tobytes() == want_h.tobytes() and got_o.tobytes() == want_o.tobytes()
                                           and got_rgb.tobytes() == want_rgb.tobytes())
        hits = max(1, int((pl["sphere"] >= 0).sum()))
        out[f"t{taps}_reused_share"] = round(float((want_h["n"] > 1).sum()) / hits, 4)
        arms[f"plain_t{taps}"]()
        plain_h = state["rp"][0].cpu().numpy().view(m.abi.HISTORY).reshape(H, W)
        out[f"t{taps}_reused_share_plain"] = round(float((plain_h["n"] > 1).sum()) / hits, 4)
    for c in ctx.values():
        c["r"].close()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

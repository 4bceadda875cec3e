"""mirt_reproject_motion_host (csrc/reproject_host.cpp) against the numpy
restatement of the definition with a motion (tests/reproject_motion_cases.py),
byte for byte, on every case x reproject_cases.PARAMS and all three outputs;
the identity motion against mirt_reproject_host; that the cases reach step 2a
and 2b's branches; the geometry of a rigid shift against a float64 projection;
that following a shifted sphere reuses more history than the plain
reprojection; that a diffusing scene's carried display is nearer the converged
frame than its one-sample frame; the argument table; and the host form under
the sanitizers (a program of its own: nothing is loaded into Python). No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reproject_cases as rc
import reproject_motion_cases as mc
import test_planes_cases as cases
from conftest import ROOT

E_INVALID = -1
F32 = np.float32


@pytest.mark.parametrize("name", mc.CASES)
def test_host_equals_the_restatement(mirt, name):
    L = mirt.load()
    c = mc.case(name)
    assert {p[1] for p in mc.PARAMS} == {1, 4}
    for params in mc.PARAMS:
        want_hist, want_out, want_rgb, _ = mc.expected(name, params)
        hist, out, rgb = mc.host(L, c, params)
        mc.same_bytes(hist, want_hist, f"{name} {params} hist_out")
        mc.same_bytes(rgb, want_rgb, f"{name} {params} out_rgb")
        mc.same_bytes(out, want_out, f"{name} {params} out")
    p0 = mc.PARAMS[0]
    want_hist, want_out, want_rgb, _ = mc.expected(name, p0)
    hist, out, rgb = mc.host(L, c, p0, want_rgb=False)
    assert rgb is None
    mc.same_bytes(hist, want_hist, f"{name} hist_out, out alone")
    mc.same_bytes(out, want_out, f"{name} out alone")
    hist, out, rgb = mc.host(L, c, p0, want_out=False)
    mc.same_bytes(rgb, want_rgb, f"{name} out_rgb alone")
    hist, _, _ = mc.host(L, c, p0, want_out=False, want_rgb=False)
    mc.same_bytes(hist, want_hist, f"{name} hist_out alone")


@pytest.mark.parametrize("name", [n for n in rc.CASES if n != "first"])   # (a motion needs a previous frame)
def test_the_identity_motion_is_the_plain_reprojection(mirt, name):
    """geo_prev equal to geo and no map (and the identity map written out):
    mirt_reproject_host's bytes, on every case of the plain form that has a
    previous frame -- its non-finite t and exact pixel centres included."""
    L = mirt.load()
    base = rc.case(name)
    assert base["cam_prev"] is not None
    n = int(max(base["sphere"].max(), base["sphere_prev"].max())) + 1
    geo = np.random.default_rng(5).uniform(-9.0, 9.0, (n, 4)).astype(F32)
    for idx in (None, np.arange(n, dtype=np.int32)):
        c = dict(base, geo=geo, geo_prev=geo.copy(), prev_index=idx)
        for params in base["params"]:
            want = rc.host(L, base, params)
            got = mc.host(L, c, params)
            for g, w, what in zip(got, want, ("hist_out", "out", "out_rgb")):
                mc.same_bytes(g, w, f"{name} {params} {what}, identity motion (map {idx is not None})")
            want = rc.expected(name, params)
            got = mc.restate(c, params)
            for g, w, what in zip(got[:3], want[:3], ("hist_out", "out", "out_rgb")):
                mc.same_bytes(g, w, f"{name} {params} {what}, the restatements")


def test_the_cases_cover_every_branch():
    why = {name: mc.expected(name, rc.DEFAULT)[3]["why"] for name in mc.CASES}
    for name in mc.REAL:
        hits = int((mc.case(name)["sphere"] >= 0).sum())
        reused = int((why[name] == mc.REUSED).sum())
        print(name, "reused", reused, "of", hits, "hit pixels")
        assert hits >= 200 and reused >= 100, (name, hits, reused)
        assert not (why[name] == mc.NO_SPHERE).any()
    # nothing moved: the plain cases' bytes
    for cam, plain in (("A", "still"), ("right", "right")):
        c = mc.case(f"still_{cam}")
        assert (c["geo"] == c["geo_prev"]).all() and c["prev_index"] is None
        p = rc.case(plain)
        rc.same_bytes(c["sphere"], p["sphere"], "the frame's sphere plane")
        for params in mc.PARAMS:
            for g, w in zip(mc.expected(f"still_{cam}", params)[:3], rc.expected(plain, params)[:3]):
                mc.same_bytes(g, w, f"still_{cam} {params} against {plain}")
    # every sphere moved / a tenth / only radii / a real permutation
    c = mc.case("diffused_A")
    assert ((c["geo"] != c["geo_prev"]).any(axis=1)).all()
    c = mc.case("shifted_A")
    moved = (c["geo"] != c["geo_prev"]).any(axis=1)
    assert moved.sum() == mc.N // mc.SHIFT_EVERY and (c["geo"][moved, 3] == c["geo_prev"][moved, 3]).all()
    c = mc.case("radii_A")
    assert (c["geo"][:, :3] == c["geo_prev"][:, :3]).all() and (c["geo"][:, 3] != c["geo_prev"][:, 3]).mean() > 0.99
    c, d = mc.case("permuted_A"), mc.case("diffused_A")
    idx = c["prev_index"]
    assert (np.sort(idx) == np.arange(mc.N)).all() and (idx != np.arange(mc.N)).mean() > 0.9
    assert (c["geo_prev"][idx] == d["geo_prev"]).all()
    for params in mc.PARAMS:   # the same pixels, whatever the previous order was
        for g, w in zip(mc.expected("permuted_A", params)[:3], mc.expected("diffused_A", params)[:3]):
            mc.same_bytes(g, w, f"permuted_A {params} against diffused_A")
    # 2a: each way out of range occurs on a pixel, takes no history, and leaves its neighbours theirs
    c = mc.case("range_9_3")
    s, n = c["sphere"].reshape(-1), len(c["geo"])
    assert s[0] == n and s[1] == 2 ** 31 - 1 and s[2] == -5 and s[3] == -(2 ** 31)
    assert list(c["prev_index"]) == [0, -1, len(c["geo_prev"]), 1] and (s == 1).any() and (s == 2).any()
    w_ = why["range_9_3"].reshape(-1)
    assert (w_[(s >= n) | (s == 1) | (s == 2)] == mc.NO_SPHERE).all() and (w_[s < 0] == mc.SKY).all()
    for taps in (1, 4):
        h_ = mc.expected("range_9_3", (64, taps, 0.015625))[0].reshape(-1)
        assert (h_["n"][(s >= n) | (s == 1) | (s == 2) | (s < 0)] == 1).all()
    assert (why["range_9_3"] == mc.REUSED).any()
    # 2b: zero and NaN radii give non-finite points and no history; a previous radius of 0 gives the centre
    c = mc.case("radius_9_3")
    assert c["geo"][1, 3] == 0 and np.isnan(c["geo"][2, 3]) and c["geo_prev"][3, 3] == 0 and np.isnan(c["geo_prev"][4, 3])
    Xp, ok, sp = mc.moved_point(c)
    s = c["sphere"]
    assert ok[s >= 0].all()
    for bad in (0, 1, 2):
        assert (s == bad).any() and not np.isfinite(Xp[s == bad]).all(axis=-1).any(), bad
        assert not (why["radius_9_3"][s == bad] == mc.REUSED).any()
    assert (s == 3).any() and (Xp[s == 3] == c["geo_prev"][3, :3]).all()
    # num_prev != num_spheres, and a map onto the extra entries
    c = mc.case("counts_5_3")
    assert len(c["geo"]) == 3 and len(c["geo_prev"]) == 5 and c["prev_index"].max() == 4
    assert (why["counts_5_3"] == mc.REUSED).any()
    # more than one tile of the kernel in both directions
    c = mc.case("m_70_5")
    assert c["width"] > 64 and c["height"] > 4 and (why["m_70_5"] == mc.REUSED).sum() > 64
    for name in ("m_5_3", "m_7_1", "m_1_7", "index_5_3"):
        assert (why[name] == mc.REUSED).any(), name


# the largest difference measured below, in pixels, and the bound asserted: 16 times it, rounded up to a power of two
GEOMETRY_MEASURED = 2.836e-6
GEOMETRY_BOUND = 2.0 ** -14


def test_the_geometry_of_a_rigid_shift():
    """shifted_A and shifted_right: on the pixels of the shifted spheres, the
    restated (xf, yf) against the float64 projection of X - SHIFT into the
    previous camera, X the float64 point of the frame's own d and t (measured:
    2.84e-6 and 2.33e-6 px)."""
    worst = 0.0
    for name in ("shifted_A", "shifted_right"):
        c = mc.case(name)
        w, h = c["width"], c["height"]
        xf, yf, zf, _, ok, _ = mc.project(c)
        on = np.isin(c["sphere"], mc.shifted_ids()) & ok & (zf > 0)
        assert on.sum() >= 50, (name, int(on.sum()))
        _, d = mc.lc.pinhole(c["cam"], None, w, h)
        cur, prv = rc.cam_consts(c["cam"], w, h), rc.cam_consts(c["cam_prev"], w, h)
        f64 = lambda v: np.asarray(v, np.float64)   # noqa: E731
        X = f64(cur["p"]) + f64(d) * f64(c["t"])[..., None] - f64(mc.SHIFT)
        e = X - f64(prv["p"])
        with np.errstate(all="ignore"):   # (sky pixels: t is 0)
            z = e @ f64(prv["fwd"])
            u = (e @ f64(prv["right"])) / z / f64(prv["sw"])
            v = (e @ f64(prv["up"])) / z / f64(prv["sh"])
        x64 = (u / f64(prv["aspect"]) + 0.5) * w
        y64 = (0.5 - v) * h
        off = float(np.maximum(np.abs(f64(xf) - x64), np.abs(f64(yf) - y64))[on].max())
        print(f"{name}: {int(on.sum())} pixels on shifted spheres, (xf, yf) off the float64 projection by at most "
              f"{off:.3e} px")
        worst = max(worst, off)
    print(f"largest difference {worst:.3e} px (recorded: {GEOMETRY_MEASURED:.3e}); bound {GEOMETRY_BOUND:.3e}")
    assert GEOMETRY_BOUND == 2.0 ** np.ceil(np.log2(16 * GEOMETRY_MEASURED))
    assert worst <= GEOMETRY_BOUND, (worst, GEOMETRY_BOUND)


def test_following_a_shifted_sphere_reuses_more():
    """One tap, shifted_A: of the pixels on the shifted spheres, the share that
    reuses a record with the motion and with the plain reprojection of the same
    frame (measured: 33 of 61, 0.541, with the motion; 3, 0.049, without)."""
    c = mc.case("shifted_A")
    params = (64, 1, 0.015625)
    on = np.isin(c["sphere"], mc.shifted_ids())
    with_motion = mc.expected("shifted_A", params)[0]["n"] > 1
    plain = rc.restate(c, params)[0]["n"] > 1
    a, b, n = int(with_motion[on].sum()), int(plain[on].sum()), int(on.sum())
    print(f"{n} pixels on shifted spheres: {a} ({a / n:.3f}) reuse history with the motion, {b} ({b / n:.3f}) without")
    assert n >= 50 and b < 0.5 * n, (b, n)
    assert a > b, (a, b)
    # the pixels of the spheres that did not move are the plain form's
    assert (with_motion[~on & (c["sphere"] >= 0)] == plain[~on & (c["sphere"] >= 0)]).all()


def test_a_diffusing_scene_converges(mirt):
    """Eight oracle frames of spheres diffusing by SIGMA per frame under camera
    A, the default parameters, each frame reprojected with the motion from the
    one before: the last display's mean squared error against the float64 mean
    of samples 8 .. 71 of the last scene is below that of its one-sample
    frame -- what an emptied history shows. The figures are printed (measured:
    627.6 against 1,783.9, a ratio of 0.352, with 83-86% of the hit pixels
    reusing a record in each frame after the first)."""
    L = mirt.load()
    cam = rc.camera("A")
    prev, shares = None, []
    for k in range(8):
        kind = f"walk{k}"
        pl = mc.oracle_planes(kind, "A")
        raw = mc.oracle_frame(kind, "A", k)
        motion = None if k == 0 else (mc.geo_of(mc.spheres_of(kind)), mc.geo_of(mc.spheres_of(f"walk{k - 1}")), None)
        hist, out = mc.host_step(L, cam, raw, pl["t"], pl["sphere"], prev, rc.DEFAULT, motion)
        prev = (cam, hist, pl["t"], pl["sphere"])
        hit = pl["sphere"] >= 0
        shares.append(float((hist["n"][hit] > 1).mean()))
    ref = np.mean([mc.oracle_frame("walk7", "A", s)[..., :3].astype(np.float64) for s in range(8, 72)], axis=0)
    mse_raw = np.mean((raw[..., :3].astype(np.float64) - ref) ** 2)
    mse_out = np.mean((out[..., :3].astype(np.float64) - ref) ** 2)
    print(f"mse {mse_raw:.2f} one sample, {mse_out:.2f} carried: ratio {mse_out / mse_raw:.4f}; reused share of the "
          f"hit pixels per frame {[round(s, 3) for s in shares]}; mean n on the last frame's hits "
          f"{hist['n'][hit].mean():.2f}")
    assert mse_out < mse_raw, (mse_out, mse_raw)


def test_argument_table(mirt):
    """The plain forms' MIRT_E_INVALID cases and the motion's own, for all three
    forms, before any HIP call and before the context is looked at."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    R, M = mirt.abi.ReprojectParams, mirt.abi.SphereMotion
    good = R(64, 4, 0.015625)
    cam, cam_prev = mirt.default_camera(), mirt.default_camera()
    n = 16
    rgba, t, sph = np.zeros((4, 4, 4), np.uint8), np.ones((4, 4), F32), np.zeros((4, 4), np.int32)
    hist, tp, sp = np.zeros(n, mirt.abi.HISTORY), np.ones((4, 4), F32), np.zeros((4, 4), np.int32)
    ho, out, rgb = np.zeros(n, mirt.abi.HISTORY), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), F32)
    geo, geo_prev, idx = np.ones((2, 4), F32), np.ones((3, 4), F32), np.zeros(2, np.int32)
    a_ = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    fine_m = M(a_(geo), a_(geo_prev), a_(idx), 2, 3)
    same_m = M(a_(geo), a_(geo), None, 2, 2)
    names = ("width", "height", "cam", "cam_prev", "rgba", "t", "sphere", "hist", "t_prev", "sphere_prev", "params",
             "hist_out", "motion")
    fine = (4, 4, cam, cam_prev, rgba, t, sph, hist, tp, sp, good, ho, fine_m)

    def but(**kw):
        a = dict(zip(names, fine))
        a.update(kw)
        return tuple(a[k] for k in names)

    nan = float("nan")
    bad = [("NULL motion", but(motion=None)), ("NULL geo", but(motion=M(None, a_(geo_prev), a_(idx), 2, 3))),
           ("NULL geo_prev", but(motion=M(a_(geo), None, a_(idx), 2, 3))),
           ("num_spheres 0", but(motion=M(a_(geo), a_(geo_prev), a_(idx), 0, 3))),
           ("num_prev 0", but(motion=M(a_(geo), a_(geo_prev), a_(idx), 2, 0))),
           ("num_spheres -1", but(motion=M(a_(geo), a_(geo_prev), a_(idx), -1, 3))),
           ("num_prev -1", but(motion=M(a_(geo), a_(geo_prev), None, 2, -1))),
           ("no map, other counts", but(motion=M(a_(geo), a_(geo_prev), None, 2, 3))),
           ("no previous frame", but(cam_prev=None, hist=None, t_prev=None, sphere_prev=None)),
           # and the plain forms' own
           ("NULL params", but(params=None)), ("NULL cam", but(cam=None)), ("NULL rgba", but(rgba=None)),
           ("NULL t", but(t=None)), ("NULL sphere", but(sphere=None)), ("NULL hist_out", but(hist_out=None)),
           ("no cam_prev", but(cam_prev=None)), ("no hist", but(hist=None)), ("hist_out is hist", but(hist_out=hist)),
           ("width 0", but(width=0)), ("height -4", but(height=-4)), ("beyond 2^31 pixels", but(width=65536, height=32769)),
           ("max_history 0", but(params=R(0, 4, 0.0))), ("taps 2", but(params=R(64, 2, 0.0))),
           ("tolerance nan", but(params=R(64, 4, nan)))]

    def call(name, c, a):
        w, h, cm, cp, r, t_, s, hi, tp_, sp_, prm, o, mo = a
        args = (w, h, ref(cm), ref(cp), p(r), p(t_), p(s), p(hi), p(tp_), p(sp_), ref(prm), p(o), p(out), p(rgb))
        if name == "mirt_reproject_motion_host":
            return L.mirt_reproject_motion_host(*args, ref(mo))
        if name == "mirt_reproject_motion":
            return L.mirt_reproject_motion(c, *args, ref(mo))
        return L.mirt_reproject_motion_device(c, *args, None, ref(mo))

    for name in ("mirt_reproject_motion_host", "mirt_reproject_motion", "mirt_reproject_motion_device"):
        if name != "mirt_reproject_motion_host":
            assert call(name, None, fine) == E_INVALID
            assert L.mirt_last_error().decode() == name + ": null context", name
        for what, a in bad:
            r = call(name, ctx, a)
            assert r == E_INVALID, (name, what, r)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, what)
            assert not ho.view(np.uint8).any() and not out.any() and not rgb.any()
    assert bytes(fake) == bytes(16384)
    assert call("mirt_reproject_motion_host", None, fine) == 0
    assert call("mirt_reproject_motion_host", None, but(motion=same_m)) == 0


def test_host_form_under_the_sanitizers(mirt):
    """tests/c/san_reproject_motion.cpp via `make -C csrc san_reproject_motion`:
    mirt_reproject_motion_host on 1 x 1, 1 x N and N x 1 images with sphere
    and prev_index entries out of range, zero and NaN radii and every invalid
    motion under ASan + UBSan, a program of its own: every check holds, no
    sanitizer reports, and the structs' sizes are abi.py's."""
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "san_reproject_motion"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(csrc, "build", "san_reproject_motion")], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0 and "san_reproject_motion: ok" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])
    sizes = dict(re.findall(r"sizeof\((\w+)\) = (\d+)", p.stdout))
    assert int(sizes["mirt_sphere_motion"]) == C.sizeof(mirt.abi.SphereMotion) == 32
    assert int(sizes["mirt_history_motion"]) == C.sizeof(mirt.abi.HistoryMotion) == 32

"""mirt_reproject_host (csrc/reproject_host.cpp) against the numpy restatement
of the definition (tests/reproject_cases.py), byte for byte, on every case,
both tap counts and all three outputs; that the cases cover every branch; that
a still camera accumulates like the accumulating loop; that a moving camera's
display is nearer the converged frame than its one-sample frame; the argument
table; and the host form under the sanitizers (a program of its own: nothing is
loaded into Python). No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_cases as dc
import reproject_cases as rc
import test_planes_cases as cases
from conftest import ROOT

E_INVALID = -1
F32 = np.float32


@pytest.mark.parametrize("name", rc.CASES)
def test_host_equals_the_restatement(mirt, name):
    L = mirt.load()
    c = rc.case(name)
    assert {p[1] for p in c["params"]} == {1, 4}
    for params in c["params"]:
        want_hist, want_out, want_rgb, _ = rc.expected(name, params)
        hist, out, rgb = rc.host(L, c, params)
        rc.same_bytes(hist, want_hist, f"{name} {params} hist_out")
        rc.same_bytes(rgb, want_rgb, f"{name} {params} out_rgb")
        rc.same_bytes(out, want_out, f"{name} {params} out")
    # the optional outputs one at a time, and neither
    p0 = c["params"][0]
    want_hist, want_out, want_rgb, _ = rc.expected(name, p0)
    hist, out, rgb = rc.host(L, c, p0, want_rgb=False)
    assert rgb is None
    rc.same_bytes(hist, want_hist, f"{name} hist_out, out alone")
    rc.same_bytes(out, want_out, f"{name} out alone")
    hist, out, rgb = rc.host(L, c, p0, want_out=False)
    rc.same_bytes(rgb, want_rgb, f"{name} out_rgb alone")
    hist, _, _ = rc.host(L, c, p0, want_out=False, want_rgb=False)
    rc.same_bytes(hist, want_hist, f"{name} hist_out alone")


def test_the_cases_cover_every_branch():
    why = {name: rc.expected(name, rc.DEFAULT)[3]["why"] for name in rc.REAL}
    hits = int((cases.expected("A")["sphere"] >= 0).sum())
    assert hits >= 200
    # every "no history" reason occurs, each where it is meant to
    assert (why["first"] != rc.REUSED).all() and (why["first"] == rc.FIRST).sum() == hits
    for name in rc.REAL:
        assert (why[name] == rc.SKY).sum() >= 200, name
    assert (why["behind"] == rc.BEHIND).sum() == hits and not (why["behind"] == rc.REUSED).any()
    for name in ("still", "right", "forward", "yaw"):
        reused = int((why[name] == rc.REUSED).sum())
        print(name, "reused", reused, "of", int((rc.case(name)["sphere"] >= 0).sum()), "hit pixels")
        assert reused >= 100, (name, reused)
    assert (why["right"] == rc.NO_TAP).sum() > 0   # disocclusions and the image's edge
    # the turn: most hit pixels' points leave the previous image
    c = rc.case("turn")
    xf, yf, zf, _ = rc.project(c)
    hit = c["sphere"] >= 0
    outside = ~((xf >= -1) & (xf < rc.W) & (yf >= -1) & (yf < rc.H)) | ~(zf > 0)
    assert hit.sum() > 0 and outside[hit].sum() > 0.5 * hit.sum(), (int(outside[hit].sum()), int(hit.sum()))
    # every count of valid taps from 1 to 4, with four taps; exactly one where three of four mismatch
    counts = set()
    for name, params in rc.runs():
        if params[1] == 4:
            counts |= set(np.unique(rc.expected(name, params)[3]["valid"]).tolist())
    assert counts >= {0, 1, 2, 3, 4}, counts
    mm = rc.expected("mismatch_6_4", (64, 4, 0.015625))[3]["valid"]
    assert (mm <= 1).all() and (mm == 1).sum() >= 6, mm
    # points exactly on a pixel centre, and on the last column and row
    for name, (px, py, gx, gy) in rc.AIMED.items():
        c = rc.case(name)
        xf, yf, zf, _ = rc.project(c)
        assert xf[py, px] == gx and yf[py, px] == gy and zf[py, px] > 0, (name, xf[py, px], yf[py, px])
        assert gx < c["width"] and gy < c["height"]
        for taps in (1, 4):
            h_ = rc.expected(name, (64, taps, 1.0))[0]
            want = c["hist"][gy, gx]
            col = c["rgba"][py, px, :3].astype(F32) / F32(255.0)
            n_new = min(int(want["n"]) + 1, 64)
            # an exact position: the one tap, or the first of four with weight exactly 1
            for ch, f in enumerate("rgb"):
                m = (F32(0.0) + want[f] * F32(1.0)) / (F32(0.0) + F32(1.0))
                assert h_[py, px][f] == m + (col[ch] - m) / F32(n_new), (name, taps, f)
            assert h_[py, px]["n"] == n_new
    assert rc.AIMED["last_5_3"][2:] == (4, 2) and rc.AIMED["last_7_1"][2] == 6 and rc.AIMED["last_1_7"][3] == 6
    # non-finite and huge t: nothing reused from NaN, and the case holds each kind on a hit pixel
    c = rc.case("nonfinite_5_3")
    t = c["t"].reshape(-1)
    assert np.isnan(t).any() and np.isposinf(t).any() and np.isneginf(t).any() and (t == F32(1e38)).any()
    assert (c["sphere"] >= 0).all()
    for taps in (1, 4):
        valid = rc.expected("nonfinite_5_3", (64, taps, 0.015625))[3]["valid"].reshape(-1)
        assert not valid[np.isnan(t)].any() and valid[np.isfinite(t) & (t == 16)].any()
    # n = 0 and n < 0 are no history; n at max_history stays there
    c = rc.case("n0_5_3")
    assert (c["hist"]["n"] == 0).any() and (c["hist"]["n"] < 0).any() and (c["hist"]["n"] == 1).any()
    h_ = rc.expected("n0_5_3", (64, 1, 0.015625))[0]
    assert set(np.unique(h_["n"])) <= {1, 2}
    h_ = rc.expected("nmax_5_3", (64, 1, 0.015625))
    assert (h_[0]["n"][h_[3]["why"] == rc.REUSED] == 64).all() and (h_[3]["why"] == rc.REUSED).any()
    h_ = rc.expected("nmax_5_3", (65536, 1, 1.0))
    assert (h_[0]["n"] == 65536).any() and (h_[0]["n"] == 65).any()
    # t_tolerance = 0: taps whose stored distance is l itself are valid, the others are not
    for params in rc.TOL0:
        v0 = rc.expected("tol0_5_3", params)[3]["valid"]
        v1 = rc.expected("tol0_5_3", (64, params[1], 0.015625))[3]["valid"]
        assert v0.sum() > 0 and (v0 <= v1).all() and v0.sum() < v1.sum(), (params, v0, v1)


def test_a_still_camera_accumulates(mirt):
    """Bitwise the same camera twice, one tap: every hit pixel of case A takes
    its own previous pixel, and after frames of samples 0 .. 3 its mean is
    step 10's recursion on the oracle's four colours."""
    L = mirt.load()
    cam = cases.camera("A")
    pl = cases.expected("A")
    hit = pl["sphere"] >= 0
    c = dict(width=rc.W, height=rc.H, cam=cam, cam_prev=cam, t=pl["t"])
    xf, yf, _, _ = rc.project(c)
    ys, xs = np.mgrid[0:rc.H, 0:rc.W]
    off = np.maximum(np.abs(xf - xs), np.abs(yf - ys))[hit].max()
    print("the round trip is off by at most", off, "pixels")
    assert off < 0.01
    assert ((np.floor(xf + F32(0.5)) == xs) & (np.floor(yf + F32(0.5)) == ys))[hit].all()
    prev, want = None, None
    for k in range(4):
        col = dc.oracle_frame(k)[..., :3].astype(F32) / F32(255.0)
        want = col if k == 0 else want + (col - want) / F32(k + 1)
        hist, out = rc.host_step(L, cam, dc.oracle_frame(k), pl["t"], pl["sphere"], prev, (64, 1, 0.015625))
        prev = (cam, hist, pl["t"], pl["sphere"])
        assert (hist["n"][hit] == k + 1).all(), k
        assert (hist["n"][~hit] == 1).all()
        got = np.stack([hist["r"], hist["g"], hist["b"]], axis=-1)
        rc.same_bytes(got[hit], want[hit], f"the mean after frame {k}")
        rc.same_bytes(out, rc.display(got), f"the display of frame {k}")


def test_a_moving_camera_converges(mirt):
    """Eight cameras, one MOVE_SPEED step along `right` each, the default
    parameters: the last display's mean squared error against the float64 mean
    of the oracle's samples 8 .. 71 from the last camera is below that
    camera's one-sample frame's. The figures are printed (MEASUREMENTS.md E
    records them: 647.6 against 1,978.3, a ratio of 0.327, with 85-88% of the
    hit pixels reusing a record in each frame after the first)."""
    L = mirt.load()
    prev, shares = None, []
    for k in range(8):
        name = f"path{k}"
        pl = rc.oracle_planes(name)
        raw = rc.oracle_frame(name, k)
        hist, out = rc.host_step(L, rc.camera(name), raw, pl["t"], pl["sphere"], prev, rc.DEFAULT)
        prev = (rc.camera(name), hist, pl["t"], pl["sphere"])
        hit = pl["sphere"] >= 0
        shares.append(float((hist["n"][hit] > 1).mean()))
    ref = np.mean([rc.oracle_frame("path7", s)[..., :3].astype(np.float64) for s in range(8, 72)], axis=0)
    mse_raw = np.mean((raw[..., :3].astype(np.float64) - ref) ** 2)
    mse_out = np.mean((out[..., :3].astype(np.float64) - ref) ** 2)
    print(f"mse {mse_raw:.2f} one sample, {mse_out:.2f} reprojected: ratio {mse_out / mse_raw:.4f}; "
          f"reused share of the hit pixels along the path {[round(s, 3) for s in shares]}; "
          f"mean n on the last frame's hits {hist['n'][hit].mean():.2f}")
    assert mse_out < mse_raw, (mse_out, mse_raw)
    assert shares[0] == 0.0 and min(shares[1:]) > 0.5


def test_argument_table(mirt):
    """Every MIRT_E_INVALID of the three forms, before any HIP call (on a
    machine without a GPU a HIP call would be MIRT_E_DEVICE) and before the
    context is looked at: a block of zero bytes stands in for it."""
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    R = mirt.abi.ReprojectParams
    good = R(64, 4, 0.015625)
    cam, cam_prev = mirt.default_camera(), mirt.default_camera()
    n = 16
    rgba, t, sph = np.zeros((4, 4, 4), np.uint8), np.ones((4, 4), F32), np.zeros((4, 4), np.int32)
    hist, tp, sp = np.zeros(n, mirt.abi.HISTORY), np.ones((4, 4), F32), np.zeros((4, 4), np.int32)
    ho, out, rgb = np.zeros(n, mirt.abi.HISTORY), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), F32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    nan, inf = float("nan"), float("inf")
    # (width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params, hist_out)
    fine = (4, 4, cam, cam_prev, rgba, t, sph, hist, tp, sp, good, ho)
    first = (4, 4, cam, None, rgba, t, sph, None, None, None, good, ho)

    def but(**kw):
        names = ("width", "height", "cam", "cam_prev", "rgba", "t", "sphere", "hist", "t_prev", "sphere_prev",
                 "params", "hist_out")
        a = dict(zip(names, fine))
        a.update(kw)
        return tuple(a[k] for k in names)

    bad = [("NULL params", but(params=None)), ("NULL cam", but(cam=None)), ("NULL rgba", but(rgba=None)),
           ("NULL t", but(t=None)), ("NULL sphere", but(sphere=None)), ("NULL hist_out", but(hist_out=None)),
           ("no cam_prev", but(cam_prev=None)), ("no hist", but(hist=None)), ("no t_prev", but(t_prev=None)),
           ("no sphere_prev", but(sphere_prev=None)),
           ("only cam_prev", but(hist=None, t_prev=None, sphere_prev=None)),
           ("only hist", but(cam_prev=None, t_prev=None, sphere_prev=None)),
           ("hist_out is hist", but(hist_out=hist)),
           ("width 0", but(width=0)), ("height 0", but(height=0)), ("width -4", but(width=-4)),
           ("height -4", but(height=-4)), ("beyond 2^31 pixels", but(width=65536, height=32769)),
           ("max_history 0", but(params=R(0, 4, 0.0))), ("max_history 65537", but(params=R(65537, 4, 0.0))),
           ("max_history -1", but(params=R(-1, 1, 0.0))), ("taps 0", but(params=R(64, 0, 0.0))),
           ("taps 2", but(params=R(64, 2, 0.0))), ("taps 3", but(params=R(64, 3, 0.0))),
           ("taps 5", but(params=R(64, 5, 0.0))), ("tolerance -1", but(params=R(64, 4, -1.0))),
           ("tolerance nan", but(params=R(64, 4, nan))), ("tolerance inf", but(params=R(64, 4, inf))),
           ("tolerance -inf", but(params=R(64, 4, -inf)))]

    def call(name, c, a):
        w, h, cm, cp, r, t_, s, hi, tp_, sp_, prm, o = a
        args = (w, h, ref(cm), ref(cp), p(r), p(t_), p(s), p(hi), p(tp_), p(sp_), ref(prm), p(o), p(out), p(rgb))
        if name == "mirt_reproject_host":
            return L.mirt_reproject_host(*args)
        if name == "mirt_reproject":
            return L.mirt_reproject(c, *args)
        return L.mirt_reproject_device(c, *args, None)

    for name in ("mirt_reproject_host", "mirt_reproject", "mirt_reproject_device"):
        if name != "mirt_reproject_host":
            for a in (fine, first):
                assert call(name, None, a) == E_INVALID
                assert L.mirt_last_error().decode() == name + ": null context", name
        for what, a in bad:
            rc_ = call(name, ctx, a)
            assert rc_ == E_INVALID, (name, what, rc_)
            assert L.mirt_last_error().decode() == name + ": invalid arguments", (name, what)
            assert not ho.view(np.uint8).any() and not out.any() and not rgb.any()
    assert bytes(fake) == bytes(16384)
    # and the valid ones are valid: all of the previous frame, or none of it; the outputs optional; the limits
    assert call("mirt_reproject_host", None, fine) == 0 and call("mirt_reproject_host", None, first) == 0
    for prm in (R(1, 1, 0.0), R(65536, 4, 3.0e38)):
        assert call("mirt_reproject_host", None, but(params=prm)) == 0
    assert L.mirt_reproject_host(4, 4, ref(cam), None, p(rgba), p(t), p(sph), None, None, None, ref(good), p(ho), None,
                                 None) == 0


def test_frame_form_invalid_before_any_hip_call(mirt):
    L = mirt.load()
    fake = C.create_string_buffer(16384)
    ctx = C.cast(fake, C.c_void_p)
    R = mirt.abi.ReprojectParams
    cam, good = mirt.default_camera(), R(64, 4, 0.015625)
    fd = mirt.frame_desc(8, 8, depth=5)
    out, raw = np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 4), np.uint8)
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
    name = "mirt_render_frame_reprojected"

    def call(c, cam_, fd_, prm, o, r):
        return L.mirt_render_frame_reprojected(c, ref(cam_), ref(fd_), ref(prm), p(o), p(r))

    assert call(None, cam, fd, good, out, raw) == E_INVALID
    assert L.mirt_last_error().decode() == name + ": null context"
    fdk = lambda **kw: mirt.frame_desc(8, 8, **dict(dict(depth=5), **kw))   # noqa: E731
    bad = [("NULL camera", (None, fd, good, out, raw)), ("NULL descriptor", (cam, None, good, out, raw)),
           ("NULL params", (cam, fd, None, out, raw)), ("NULL out", (cam, fd, good, None, raw)),
           ("accumulate", (cam, fdk(accumulate=True, frames=2), good, out, raw)),
           ("samples 2", (cam, fdk(samples=2), good, out, raw)),
           ("two shards", (cam, fdk(shard=0, num_shards=2), good, out, raw)),
           ("second of two shards", (cam, fdk(shard=1, num_shards=2), good, out, None)),
           ("jitter", (cam, fdk(jitter=True), good, out, raw)),
           ("max_depth 0", (cam, fdk(depth=0), good, out, raw)),
           ("zero width", (cam, mirt.frame_desc(0, 8, depth=5), good, out, raw)),
           ("taps 2", (cam, fd, R(64, 2, 0.0), out, raw)), ("max_history 0", (cam, fd, R(0, 4, 0.0), out, raw)),
           ("tolerance nan", (cam, fd, R(64, 4, float("nan")), out, raw))]
    for what, a in bad:
        rc_ = call(ctx, *a)
        assert rc_ == E_INVALID, (what, rc_)
        assert L.mirt_last_error().decode() == name + ": invalid arguments", what
        assert not out.any() and not raw.any()
    assert bytes(fake) == bytes(16384)
    for fn in (L.mirt_history_reset, lambda c: L.mirt_history_stats_get(c, C.byref(mirt.abi.HistoryStats())),
               lambda c: L.mirt_history_read(c, p(np.zeros(4, mirt.abi.HISTORY)), 4)):
        assert fn(None) == E_INVALID


def test_host_reprojection_under_the_sanitizers():
    """tests/c/san_reproject.cpp via `make -C csrc san_reproject`:
    mirt_reproject_host on 1 x 1, 1 x N and N x 1 images, previous cameras
    behind and beside the point, NaN, infinite and huge t and every invalid
    argument under ASan + UBSan, a program of its own: every check holds and no
    sanitizer reports."""
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "san_reproject"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(csrc, "build", "san_reproject")], capture_output=True, text=True, timeout=600,
                       env=env)
    assert p.returncode == 0 and "san_reproject: ok" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])

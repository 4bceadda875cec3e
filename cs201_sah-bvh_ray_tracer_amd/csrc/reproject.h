// The reprojection of a frame's history of mirt_reproject* (include/mirt.h
// mirt_reproject_params), stated once for the host form (reproject_host.cpp)
// and the kernels (reproject.hip). Under -ffp-contract=off every operation
// below is one correctly rounded binary32 operation, in the order written
// (tests/reproject_cases.py restates it in numpy, bit for bit); sqrtf is the
// correctly rounded root (trace.h sqrt_rn32 has why that spelling serves).
//
// An image of width x height pixels, row-major, pixel i = y * width + x,
// unsharded. Two cameras, the current one and the previous one, each as the
// constants make_frame_const computes (render.hip; ReprojectCam below): position
// p, forward, right, up, sw = 2 half_w, sh = 2 half_h, hor = right * sw,
// ver = up * sh, aspect, wf, hf. Per pixel of the current frame: rgba (the
// display of a one-sample frame), t and sphere (mirt_primary_planes). Per
// pixel of the previous frame: hist = {r, g, b, n}, the mean of n samples
// (n == 0: no history), t_prev and sphere_prev. Without a previous frame every
// pixel takes "no history". For pixel (x, y):
//
//  1 c[ch] = (float)u8 / 255.0f (main.c:368-370); s = sphere[i]. s < 0: no
//    history (the sky carries no noise).
//  2 d = the unjittered pinhole direction of (x, y) under the current camera
//    (render.hip camera_ray's arithmetic, normalize3 included: zero for a zero
//    length); X[k] = p[k] + d[k] * t[i].
//  3 e[k] = X[k] - p_prev[k]; zf = dot3(e, forward_prev), left to right.
//    !(zf > 0.0f): no history.
//  4 a = dot3(e, right_prev) / zf; b = dot3(e, up_prev) / zf; u = a / sw_prev;
//    v = b / sh_prev; xf = (u / aspect + 0.5f) * wf; yf = (0.5f - v) * hf
//    (the inverse of main.c:362-365).
//  5 l = sqrtf(dot3(e, e)).
//  6 taps == 1: gx = floorf(xf + 0.5f), gy likewise; one tap (gx, gy), w = 1.0f.
//    taps == 4: gx = floorf(xf), gy = floorf(yf), ax = xf - gx, ay = yf - gy;
//    the taps in this order: (gx, gy) with (1 - ax) * (1 - ay), (gx + 1, gy)
//    with ax * (1 - ay), (gx, gy + 1) with (1 - ax) * ay, (gx + 1, gy + 1)
//    with ax * ay.
//  7 A tap (tx, ty) is kept as floats and is inside iff tx >= 0.0f && tx < wf
//    && ty >= 0.0f && ty < hf; only then is it cast to int. NaN or infinite
//    coordinates fail every comparison: no position computed from the data
//    ever indexes outside the image.
//  8 An inside tap q is valid iff w > 0.0f, sphere_prev[q] == s,
//    hist[q].n >= 1 and fabsf(l - t_prev[q]) <= t_tolerance * l (which rejects
//    the far side, or another part, of the same sphere).
//  9 Over the valid taps, in visiting order, from +0.0f: sw_ = sw_ + w,
//    sc[ch] = sc[ch] + hist[q].c[ch] * w, nmin = min n. No valid tap: no
//    history. Else m[ch] = sc[ch] / sw_.
// 10 n_new = min(nmin + 1, max_history); mean[ch] = m[ch] + (c[ch] - m[ch]) /
//    (float)n_new. No history: n_new = 1, mean = c.
// 11 hist_out[i] = {mean, n_new}; out: RGBA8 by denoise_display's cast of
//    mean; out_rgb: the three floats of mean.
//
// Unlike the denoiser's, the tap positions depend on the data; step 7 is what
// keeps every access inside the image whatever t holds.
//
// With a MOTION (mirt_reproject_motion*, mirt_sphere_motion: the spheres moved
// between the two frames) the hit point is first carried back to where its
// sphere was. geo[num_spheres] is the scene `sphere` indexes, geo_prev[num_prev]
// the previous frame's, each {centre.xyz, radius}; prev_index[s] is the index in
// geo_prev of the sphere that is now s (none: the identity). Steps 2, 3 and 8
// become:
//
//  2  as above, X[j] = p[j] + d[j] * t[i].
//  2a s is data: !(0 <= s < num_spheres): no history. sp = prev_index ?
//     prev_index[s] : s; !(0 <= sp < num_prev): no history. Both comparisons
//     are made before either value indexes anything (ReprojectMoved below: a
//     value out of range reads index 0 and is dropped).
//  2b g = geo[s], gp = geo_prev[sp]. All four floats of gp == g's (float ==: a
//     NaN is unequal): Xp = X. Otherwise k = gp.r / g.r; o = X[j] - g.c[j];
//     o = o * k; Xp[j] = gp.c[j] + o: the same surface point where the sphere
//     was, rescaled if its radius changed. A zero or non-finite radius gives a
//     non-finite Xp, and step 7 keeps every access inside the image.
//  3  e[j] = Xp[j] - p_prev[j]; the rest of 3 and 4 - 7 unchanged.
//  8  ... sphere_prev[q] == sp (not s) ...
//
// A motion with geo_prev equal to geo and the identity map is the plain
// reprojection byte for byte; without a motion nothing above changes.
//
// With MOMENTS (mirt_reproject_moments*) a float plane m2 travels with the
// records: the running mean of lum(sample)^2, lum(c) being L = 0.2126f * c[0];
// L = L + 0.7152f * c[1]; L = L + 0.0722f * c[2] (reproject_lum). It is carried
// exactly as the record's colour is; steps 1 - 11 are unchanged and these join:
//
//  1' Lc = lum(c); q2 = Lc * Lc.
//  9' over the same valid taps, in the same order, from +0.0f:
//     s2 = s2 + m2_prev[q] * w; then M2 = s2 / sw_. (m2_prev[q] is loaded with
//     the tap's other loads, before any is used.)
// 10' m2_out[i] = M2 + (q2 - M2) / (float)n_new. No history (sky, first frame,
//     behind the camera, no valid tap): m2_out[i] = q2.
//
// The records, out and out_rgb are byte for byte those without the moments.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "../../include/mirt.h"
#include "denoise.h"   // denoise_size_valid, denoise_display
#include "rng.h"       // MIRT_HD

namespace mirt {

constexpr int kReprojectMaxHistory = 65536;

// A camera as the frames see it (make_frame_const's expressions, computed on
// the host: libm tan stays there).
struct ReprojectCam {
    float p[3], fwd[3], right[3], up[3];
    float hor[3], ver[3];   // right * sw, up * sh
    float sw, sh;
    float aspect, wf, hf;
};

inline ReprojectCam reproject_cam(const mirt_camera* cam, int width, int height)
{
    ReprojectCam r{};
    const float aspect = (float)width / (float)height;
    const float fov_rad = (float)((double)cam->fov * (M_PI / 180.0));
    const float half_h = (float)std::tan((double)(fov_rad / 2.0f));
    const float half_w = aspect * half_h;
    r.sw = 2.0f * half_w;
    r.sh = 2.0f * half_h;
    r.p[0] = cam->position.x; r.p[1] = cam->position.y; r.p[2] = cam->position.z;
    r.fwd[0] = cam->forward.x; r.fwd[1] = cam->forward.y; r.fwd[2] = cam->forward.z;
    r.right[0] = cam->right.x; r.right[1] = cam->right.y; r.right[2] = cam->right.z;
    r.up[0] = cam->up.x; r.up[1] = cam->up.y; r.up[2] = cam->up.z;
    for (int k = 0; k < 3; k++) {
        r.hor[k] = r.right[k] * r.sw;
        r.ver[k] = r.up[k] * r.sh;
    }
    r.aspect = aspect;
    r.wf = (float)width;
    r.hf = (float)height;
    return r;
}

inline bool reproject_params_valid(const mirt_reproject_params* p)
{
    return p && p->max_history >= 1 && p->max_history <= kReprojectMaxHistory && (p->taps == 1 || p->taps == 4) &&
           std::isfinite(p->t_tolerance) && p->t_tolerance >= 0.0f;
}

MIRT_HD float reproject_dot3(const float a[3], const float b[3])   // trace.h dot3: left to right
{
    float s = a[0] * b[0];
    s = s + a[1] * b[1];
    return s + a[2] * b[2];
}

// lum(c) of 1' (and of csrc/vfilter.h)
MIRT_HD float reproject_lum(float r, float g, float b)
{
    float L = 0.2126f * r;
    L = L + 0.7152f * g;
    return L + 0.0722f * b;
}

// What became of a pixel (mirt_history_stats counts them).
enum { kReprojectSky = 0, kReprojectFresh = 1, kReprojectReused = 2 };

// Steps 2a and 2b's loads for a pixel whose sphere is s: g, gp, sp, and ok =
// both range tests passed. `mo` gives the motion: mo.num_spheres, mo.num_prev
// (each >= 1), mo.has_index(), mo.index(i), mo.geo(i, out), mo.geo_prev(i, out)
// at indices INSIDE the arrays. Every load is unconditional -- an index out of
// range reads element 0 and ok is false -- so that the kernels issue geo[s]
// and prev_index[s] together, then geo_prev[sp], ahead of the taps.
struct ReprojectMoved {
    float g[4], gp[4];
    int32_t sp;
    bool ok;
};
template <class Mo>
MIRT_HD ReprojectMoved reproject_moved(const Mo& mo, int32_t s)
{
    ReprojectMoved m;
    const bool in = s >= 0 && s < mo.num_spheres;
    const int32_t si = in ? s : 0;
    mo.geo(si, m.g);
    m.sp = mo.has_index() ? mo.index(si) : si;
    m.ok = in && m.sp >= 0 && m.sp < mo.num_prev;
    mo.geo_prev(m.ok ? m.sp : 0, m.gp);
    return m;
}

inline bool reproject_motion_valid(const mirt_sphere_motion* m, bool has_prev)
{
    return m && has_prev && m->geo && m->geo_prev && m->num_spheres >= 1 && m->num_prev >= 1 &&
           (m->prev_index || m->num_prev == m->num_spheres);
}

// Pixel (x, y)'s new record, from its own rgba, t and s = sphere. has_prev
// false: no previous frame (prev is not looked at). `at` gives the previous frame at an index INSIDE the
// image: at.hist(q), at.t(q), at.sphere(q). TAPS: 1 or 4. *kind: one of the
// three above. moved: none (the plain reprojection), or the pixel's one
// ReprojectMoved (the reprojection with a motion). MOMENTS: an `at` that also
// has at.m2(q), the previous frame's m2, and a float* at.m2_new, which
// receives the value of step 10'.
template <class At, class = void>
struct reproject_at_moments : std::false_type {};
template <class At>
struct reproject_at_moments<At, std::void_t<decltype(std::declval<const At&>().m2(size_t{}))>> : std::true_type {};

template <int TAPS, class At, class... Moved>
MIRT_HD mirt_history_px reproject_pixel(const ReprojectCam& cur, const ReprojectCam& prev, bool has_prev, const At& at,
                                        int width, int x, int y, uint32_t rgba, float t, int32_t s, int max_history,
                                        float t_tolerance, int* kind, const Moved&... moved)
{
    static_assert(sizeof...(Moved) <= 1, "at most one ReprojectMoved");
    constexpr bool MOMENTS = reproject_at_moments<At>::value;
    const float c[3] = {(float)(rgba & 0xffu) / 255.0f, (float)((rgba >> 8) & 0xffu) / 255.0f,
                        (float)((rgba >> 16) & 0xffu) / 255.0f};
    mirt_history_px fresh{c[0], c[1], c[2], 1};
    float q2 = 0.0f;
    if constexpr (MOMENTS) {
        // 1'
        const float Lc = reproject_lum(c[0], c[1], c[2]);
        q2 = Lc * Lc;
        *at.m2_new = q2;
    }
    *kind = s < 0 ? kReprojectSky : kReprojectFresh;
    if (s < 0 || !has_prev) return fresh;
    int32_t sp = s;   // 8 compares the previous frame's sphere with it
    if constexpr (sizeof...(Moved) == 1) {
        // 2a
        if (!(moved.ok && ...)) return fresh;
        sp = (moved.sp + ...);
    }
    // 2: the hit point
    const float u0 = ((float)x / cur.wf - 0.5f) * cur.aspect;
    const float v0 = -((float)y / cur.hf - 0.5f);
    float d[3];
    for (int k = 0; k < 3; k++) {
        d[k] = cur.fwd[k] + cur.hor[k] * u0;
        d[k] = d[k] + cur.ver[k] * v0;
    }
    float sq = d[0] * d[0];
    sq = sq + d[1] * d[1];
    sq = sq + d[2] * d[2];
    const float len = __builtin_sqrtf(sq);
    for (int k = 0; k < 3; k++) d[k] = len != 0.0f ? d[k] / len : 0.0f;
    // 3 .. 5: where the previous camera saw it, and how far away
    float e[3];
    for (int k = 0; k < 3; k++) {
        float X = cur.p[k] + d[k] * t;
        if constexpr (sizeof...(Moved) == 1) {
            // 2b
            const ReprojectMoved& m = (moved, ...);
            if (!(m.gp[0] == m.g[0] && m.gp[1] == m.g[1] && m.gp[2] == m.g[2] && m.gp[3] == m.g[3])) {
                const float kr = m.gp[3] / m.g[3];
                float o = X - m.g[k];
                o = o * kr;
                X = m.gp[k] + o;
            }
        }
        e[k] = X - prev.p[k];
    }
    const float zf = reproject_dot3(e, prev.fwd);
    if (!(zf > 0.0f)) return fresh;
    const float a = reproject_dot3(e, prev.right) / zf;
    const float b = reproject_dot3(e, prev.up) / zf;
    const float u = a / prev.sw;
    const float v = b / prev.sh;
    const float xf = (u / prev.aspect + 0.5f) * prev.wf;
    const float yf = (0.5f - v) * prev.hf;
    const float l = __builtin_sqrtf(reproject_dot3(e, e));
    // 6: the taps
    float tx[TAPS], ty[TAPS], w[TAPS];
    if (TAPS == 1) {
        tx[0] = floorf(xf + 0.5f);
        ty[0] = floorf(yf + 0.5f);
        w[0] = 1.0f;
    } else {
        const float gx = floorf(xf), gy = floorf(yf);
        const float ax = xf - gx, ay = yf - gy;
        const float bx = 1.0f - ax, by = 1.0f - ay;
        tx[0] = gx;             ty[0] = gy;             w[0] = bx * by;
        tx[1 % TAPS] = gx + 1.0f; ty[1 % TAPS] = gy;        w[1 % TAPS] = ax * by;
        tx[2 % TAPS] = gx;        ty[2 % TAPS] = gy + 1.0f; w[2 % TAPS] = bx * ay;
        tx[3 % TAPS] = gx + 1.0f; ty[3 % TAPS] = gy + 1.0f; w[3 % TAPS] = ax * ay;
    }
    // 7: every tap's loads before any is used, unconditionally (a tap that is
    // not inside reads the pixel's own index and is dropped), so that the
    // kernels issue them together
    const size_t self = (size_t)y * width + x;
    bool inside[TAPS];
    mirt_history_px hq[TAPS];
    float tq[TAPS];
    int32_t sq_[TAPS];
    float m2q[TAPS];
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < TAPS; j++) {
        inside[j] = tx[j] >= 0.0f && tx[j] < prev.wf && ty[j] >= 0.0f && ty[j] < prev.hf;
        const size_t q = inside[j] ? (size_t)(int)ty[j] * width + (int)tx[j] : self;
        hq[j] = at.hist(q);
        tq[j] = at.t(q);
        sq_[j] = at.sphere(q);
        if constexpr (MOMENTS) m2q[j] = at.m2(q);
    }
    // 8, 9
    float sw_ = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f};
    float s2 = 0.0f;   // (MOMENTS)
    int32_t nmin = 0;
    bool any = false;
    const float bound = t_tolerance * l;
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < TAPS; j++) {
        if (!inside[j] || !(w[j] > 0.0f) || sq_[j] != sp || hq[j].n < 1 || !(fabsf(l - tq[j]) <= bound)) continue;
        sw_ = sw_ + w[j];
        sc[0] = sc[0] + hq[j].r * w[j];
        sc[1] = sc[1] + hq[j].g * w[j];
        sc[2] = sc[2] + hq[j].b * w[j];
        if constexpr (MOMENTS) s2 = s2 + m2q[j] * w[j];
        nmin = any && nmin < hq[j].n ? nmin : hq[j].n;
        any = true;
    }
    if (!any) return fresh;
    // 10 (nmin + 1 without the overflow an unchecked record could provoke)
    const int32_t n_new = nmin >= max_history ? max_history : nmin + 1;
    const float nf = (float)n_new;
    mirt_history_px out;
    const float m0 = sc[0] / sw_, m1 = sc[1] / sw_, m2 = sc[2] / sw_;
    out.r = m0 + (c[0] - m0) / nf;
    out.g = m1 + (c[1] - m1) / nf;
    out.b = m2 + (c[2] - m2) / nf;
    out.n = n_new;
    if constexpr (MOMENTS) {
        // 9', 10'
        const float M2 = s2 / sw_;
        *at.m2_new = M2 + (q2 - M2) / nf;
    }
    if (n_new > 1) *kind = kReprojectReused;
    return out;
}

// 11: the display of a record
MIRT_HD uint32_t reproject_display(const mirt_history_px& h)
{
    return denoise_display(DenoiseColour{h.r, h.g, h.b, 0});
}

}  // namespace mirt

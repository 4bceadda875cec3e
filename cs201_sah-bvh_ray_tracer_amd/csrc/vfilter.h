// The variance-guided a-trous filter of mirt_denoise_var* (include/mirt.h
// mirt_denoise_var_params), stated once for the host form (vfilter_host.cpp)
// and the kernels (vfilter.hip). Under -ffp-contract=off every operation below
// is one correctly rounded binary32 operation, in the order written
// (tests/vfilter_cases.py restates it in numpy, bit for bit). No square root.
//
// An image of width x height pixels, row-major, pixel i = y * width + x, with
//   hist     mirt_history_px: the colour c = {r, g, b} and n, the samples in it;
//   m2       the running mean of lum(sample)^2 (csrc/reproject.h, MOMENTS);
//   sphere   the pixel's primary-hit sphere index, < 0 on a miss;
//   normal   three floats per pixel, or none.
// lum(c) is reproject_lum: L = 0.2126f * c[0]; L = L + 0.7152f * c[1];
// L = L + 0.0722f * c[2].
//
// V1 Lp = lum(c_p). n_p >= min_history: vt = fmaxf(m2_p - Lp * Lp, 0.0f);
//    var_p = vt / (float)n_p -- the variance of the mean of n_p samples.
// V2 Otherwise (every n_p <= 0 included) the estimate is spatial, over the
//    7 x 7 window at spacing 1, dy = -3 .. 3 outermost and dx = -3 .. 3
//    innermost, centre included: a tap q inside the image with
//    sphere[q] == sphere[p] contributes k = k + 1.0f, S1 = S1 + Lq,
//    S2 = S2 + Lq * Lq, Lq = lum(c_q), all three from +0.0f. Then mu = S1 / k
//    and var_p = fmaxf(S2 / k - mu * mu, 0.0f). (The centre always
//    contributes: k >= 1.)
// V3 Pass i = 0 .. passes - 1 has spacing s = 2^i, reads the colours and
//    variances the pass before wrote (pass 0: c and var of V1 - V2) and writes
//    new ones. Taps, visiting order, B, the same-sphere rule, the normal
//    weight and the centre's 9/64 are denoise.h's. With sigma_lum > 0 every
//    other tap is also weighted by luminance, Lp and Lq of this pass's input:
//      dl = Lp - Lq;  g = dl * dl
//      den = sl2 * var_p;  den = den + 1e-6f
//      w = w * (1.0f / (1.0f + g / den))
//    sl2 = sigma_lum * sigma_lum, computed on the host, the same in every pass
//    (the shrinking variance does the rescaling). The accumulations are
//    sw = sw + w, sc[ch] = sc[ch] + c_q[ch] * w and sv = sv + var_q * (w * w),
//    from +0.0f in visiting order; the pass writes the colour sc[ch] / sw and
//    the variance sv / (sw * sw).
// V4 The outputs are the denoiser's: out_rgb the three floats, out the RGBA8
//    of denoise_display.
//
// With sigma_lum == 0 the colours' operations are denoise_pixel's with
// inv == 0, one for one. Tap positions come from the pixel's coordinates
// alone: non-finite data gives unspecified values and no access outside the
// image.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mirt.h"
#include "denoise.h"     // denoise_b, denoise_display, denoise_size_valid
#include "reproject.h"   // reproject_lum, kReprojectMaxHistory
#include "rng.h"         // MIRT_HD

namespace mirt {

// What a pass reads per tap, 16 bytes each: the colour with its variance,
// which ping-pong, and the normal with the sphere index, constant across the
// passes.
struct alignas(16) VfColour {
    float r, g, b, var;
};
struct alignas(16) VfGuide {
    float nx, ny, nz;
    int32_t sphere;
};

inline bool vfilter_params_valid(const mirt_denoise_var_params* p)
{
    return p && p->passes >= 1 && p->passes <= kDenoiseMaxPasses && p->normal_sharpness >= 0 &&
           p->normal_sharpness <= kDenoiseMaxSharpness && std::isfinite(p->sigma_lum) && p->sigma_lum >= 0.0f &&
           p->min_history >= 1 && p->min_history <= kReprojectMaxHistory;
}

// sl2 (0 when there is no luminance weight)
inline float vfilter_sl2(float sigma_lum) { return sigma_lum > 0.0f ? sigma_lum * sigma_lum : 0.0f; }

// V1, V2: var_p of pixel (x, y). `at` gives the inputs at a pixel INSIDE the
// image: at.hist(qx, qy) and at.sphere(qx, qy); hp, m2p, sp: the pixel's own.
template <class At>
MIRT_HD float vfilter_variance(const At& at, int width, int height, int x, int y, const mirt_history_px& hp, float m2p,
                               int32_t sp, int min_history)
{
    if (hp.n >= min_history) {
        const float Lp = reproject_lum(hp.r, hp.g, hp.b);
        const float vt = fmaxf(m2p - Lp * Lp, 0.0f);
        return vt / (float)hp.n;
    }
    float k = 0.0f, S1 = 0.0f, S2 = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
        // (unsigned: a position below 0 is outside too)
        const uint32_t qy = (uint32_t)y + (uint32_t)dy;
        // the row's seven taps are loaded before any is used (a tap outside reads the pixel itself and is dropped)
        mirt_history_px hq[7];
        int32_t sq[7];
        bool inside[7];
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 7; j++) {
            const uint32_t qx = (uint32_t)x + (uint32_t)(j - 3);
            inside[j] = qy < (uint32_t)height && qx < (uint32_t)width;
            const int tx = inside[j] ? (int)qx : x, ty = inside[j] ? (int)qy : y;
            hq[j] = at.hist(tx, ty);
            sq[j] = at.sphere(tx, ty);
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 7; j++) {
            if (!inside[j] || sq[j] != sp) continue;
            const float Lq = reproject_lum(hq[j].r, hq[j].g, hq[j].b);
            k = k + 1.0f;
            S1 = S1 + Lq;
            S2 = S2 + Lq * Lq;
        }
    }
    const float mu = S1 / k;
    return fmaxf(S2 / k - mu * mu, 0.0f);
}

// V3: one pass's colour and variance of pixel (x, y). `at` gives the pass's
// input at a pixel INSIDE the image: at.colour(qx, qy) and at.guide(qx, qy)
// (the guide's normal is not used with has_normal false).
template <class At>
MIRT_HD VfColour vfilter_pixel(const At& at, int width, int height, int x, int y, int s, bool has_normal, int sharpness,
                               float sl2)
{
    const VfColour cp = at.colour(x, y);
    const VfGuide gp = at.guide(x, y);
    const bool use_n = has_normal && gp.sphere >= 0;
    const bool use_l = sl2 > 0.0f;
    const float Lp = reproject_lum(cp.r, cp.g, cp.b);
    float den = sl2 * cp.var;
    den = den + 1e-6f;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        // (unsigned: a position below 0 or past INT_MAX is outside too)
        const uint32_t qy = (uint32_t)y + (uint32_t)(dy * s);
        // the row's five taps are loaded before any is used, unconditionally
        // (a tap outside the image reads the pixel itself and is dropped)
        VfColour cq[5];
        VfGuide gq[5];
        bool inside[5];
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 5; j++) {
            const uint32_t qx = (uint32_t)x + (uint32_t)((j - 2) * s);
            inside[j] = qy < (uint32_t)height && qx < (uint32_t)width;
            const int tx = inside[j] ? (int)qx : x, ty = inside[j] ? (int)qy : y;
            cq[j] = at.colour(tx, ty);
            gq[j] = at.guide(tx, ty);
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 5; j++) {
            if (!inside[j] || gq[j].sphere != gp.sphere) continue;
            float w = denoise_b(dy + 2) * denoise_b(j);
            if (j != 2 || dy != 0) {
                if (use_n) {
                    float d = gp.nx * gq[j].nx;
                    d = d + gp.ny * gq[j].ny;
                    d = d + gp.nz * gq[j].nz;
                    float m = fmaxf(d, 0.0f);
                    for (int k = 0; k < sharpness; k++) m = m * m;
                    w = w * m;
                }
                if (use_l) {
                    const float Lq = reproject_lum(cq[j].r, cq[j].g, cq[j].b);
                    const float dl = Lp - Lq;
                    const float g = dl * dl;
                    w = w * (1.0f / (1.0f + g / den));
                }
            }
            sw = sw + w;
            sr = sr + cq[j].r * w;
            sg = sg + cq[j].g * w;
            sb = sb + cq[j].b * w;
            sv = sv + cq[j].var * (w * w);
        }
    }
    return VfColour{sr / sw, sg / sw, sb / sw, sv / (sw * sw)};
}

// V4: the display of a filtered colour
MIRT_HD uint32_t vfilter_display(const VfColour& c) { return denoise_display(DenoiseColour{c.r, c.g, c.b, 0}); }

}  // namespace mirt

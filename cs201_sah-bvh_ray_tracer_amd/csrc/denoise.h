// The edge-avoiding a-trous filter of mirt_denoise* (include/mirt.h
// mirt_denoise_params), stated once for the host form (denoise_host.cpp) and
// the kernels (denoise.hip). Under -ffp-contract=off every operation below is
// one correctly rounded binary32 operation, in the order written
// (tests/denoise_cases.py restates it in numpy, bit for bit).
//
// An image of width x height pixels, row-major, pixel i = y * width + x, with
//   colour   c[ch] = (float)u8 / 255.0f of a packed RGBA8 display
//            (main.c:368-370), or a[ch] / (float)frames of float3 sums;
//   sphere   the pixel's primary-hit sphere index, < 0 on a miss;
//   normal   three floats per pixel, or none.
// Pass i = 0 .. passes - 1 has tap spacing s = 2^i, reads the colours the pass
// before it wrote (pass 0: the source colours) and writes a new image. For
// pixel p = (x, y) the taps q = (x + dx * s, y + dy * s) are visited with
// dy = -2 .. 2 outermost and dx = -2 .. 2 innermost. A tap outside the image
// or with sphere[q] != sphere[p] contributes nothing (two misses are equal:
// sky filters with sky). Otherwise
//   w = B[dy + 2] * B[dx + 2], B = {1/16, 1/4, 3/8, 1/4, 1/16} (exact products)
// and the centre tap keeps exactly that, 9/64, so the weight sum is never zero.
// Every other tap:
//   with normals and sphere[p] >= 0:
//     d = nx_p * nx_q;  d = d + ny_p * ny_q;  d = d + nz_p * nz_q
//     m = fmaxf(d, 0);  m = m * m, normal_sharpness times;  w = w * m
//   with sigma_colour > 0:
//     e = c_p - c_q per channel, of this pass's input
//     g = er * er;  g = g + eg * eg;  g = g + eb * eb
//     w = w * (1.0f / (1.0f + g * inv_i))
//     inv_0 = 1.0f / (sigma_colour * sigma_colour), inv_{i+1} = inv_i * 4.0f
//     (both computed on the host: denoise_inv)
// sw = sw + w and sc[ch] = sc[ch] + c_q[ch] * w in visiting order, both from
// +0.0f; the pass's colour is sc[ch] / sw. After the last pass the float
// output takes the three floats and the RGBA8 output
// (uint32_t)(int)fminf(c * 255.0f, 255.0f) per channel (the cast of
// main.c:398-400) with alpha 255.
//
// Tap positions come from the pixel's coordinates alone, never from the data:
// non-finite colours or normals give unspecified values and no access outside
// the image.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mirt.h"
#include "rng.h"   // MIRT_HD

namespace mirt {

constexpr int kDenoiseMaxPasses = 5, kDenoiseMaxSharpness = 7;

// What a pass reads and writes per pixel, 16 bytes each, so that a tap is two
// 16-byte loads: the colour with the sphere index in the fourth word, and the
// normal.
struct alignas(16) DenoiseColour {
    float r, g, b;
    int32_t sphere;
};
struct alignas(16) DenoiseNormal {
    float x, y, z, pad;
};

inline bool denoise_params_valid(const mirt_denoise_params* p)
{
    return p && p->passes >= 1 && p->passes <= kDenoiseMaxPasses && p->normal_sharpness >= 0 &&
           p->normal_sharpness <= kDenoiseMaxSharpness && std::isfinite(p->sigma_colour) && p->sigma_colour >= 0.0f;
}

// width x height within the frame descriptor's pixel limit (frame_desc_valid)
inline bool denoise_size_valid(int width, int height)
{
    return width >= 1 && height >= 1 && (int64_t)width * height <= (int64_t)1 << 31;
}

// inv_i of pass i (0 when there is no colour weight)
inline float denoise_inv(float sigma_colour, int pass)
{
    if (!(sigma_colour > 0.0f)) return 0.0f;
    float inv = 1.0f / (sigma_colour * sigma_colour);
    for (int i = 0; i < pass; i++) inv = inv * 4.0f;
    return inv;
}

// The source colour of a pixel, with its sphere index: of the packed RGBA8
// px (r in the low byte), or of the pixel's three sums a.
MIRT_HD DenoiseColour denoise_source_rgba(uint32_t px, int32_t sphere)
{
    return DenoiseColour{(float)(px & 0xffu) / 255.0f, (float)((px >> 8) & 0xffu) / 255.0f,
                         (float)((px >> 16) & 0xffu) / 255.0f, sphere};
}
MIRT_HD DenoiseColour denoise_source_accum(const float* a, int frames, int32_t sphere)
{
    const float f = (float)frames;
    return DenoiseColour{a[0] / f, a[1] / f, a[2] / f, sphere};
}

MIRT_HD float denoise_b(int i)   // B[i], i = 0 .. 4
{
    return i == 2 ? 0.375f : (i == 1 || i == 3) ? 0.25f : 0.0625f;
}

// One pass's colour of pixel (x, y). `at` gives the pass's input at a pixel
// INSIDE the image: at.colour(qx, qy) and at.normal(qx, qy) (anything without
// a normal plane, has_normal false: it is not used).
template <class At>
MIRT_HD DenoiseColour denoise_pixel(const At& at, int width, int height, int x, int y, int s, bool has_normal,
                                    int sharpness, float inv)
{
    const DenoiseColour cp = at.colour(x, y);
    const bool use_n = has_normal && cp.sphere >= 0;
    const DenoiseNormal np = at.normal(x, y);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        // (unsigned: a position below 0 or past INT_MAX is outside too)
        const uint32_t qy = (uint32_t)y + (uint32_t)(dy * s);
        // The row's five taps are loaded before any is used, unconditionally
        // (a tap outside the image reads the pixel itself and is dropped), so
        // that the kernels issue a row's loads together.
        DenoiseColour cq[5];
        DenoiseNormal nq[5];
        bool inside[5];
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 5; j++) {
            const uint32_t qx = (uint32_t)x + (uint32_t)((j - 2) * s);
            inside[j] = qy < (uint32_t)height && qx < (uint32_t)width;
            const int tx = inside[j] ? (int)qx : x, ty = inside[j] ? (int)qy : y;
            cq[j] = at.colour(tx, ty);
            nq[j] = at.normal(tx, ty);
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 5; j++) {
            if (!inside[j] || cq[j].sphere != cp.sphere) continue;
            float w = denoise_b(dy + 2) * denoise_b(j);
            if (j != 2 || dy != 0) {
                if (use_n) {
                    float d = np.x * nq[j].x;
                    d = d + np.y * nq[j].y;
                    d = d + np.z * nq[j].z;
                    float m = fmaxf(d, 0.0f);
                    for (int k = 0; k < sharpness; k++) m = m * m;
                    w = w * m;
                }
                if (inv > 0.0f) {
                    const float er = cp.r - cq[j].r, eg = cp.g - cq[j].g, eb = cp.b - cq[j].b;
                    float g = er * er;
                    g = g + eg * eg;
                    g = g + eb * eb;
                    w = w * (1.0f / (1.0f + g * inv));
                }
            }
            sw = sw + w;
            sr = sr + cq[j].r * w;
            sg = sg + cq[j].g * w;
            sb = sb + cq[j].b * w;
        }
    }
    return DenoiseColour{sr / sw, sg / sw, sb / sw, cp.sphere};
}

// The display of a filtered colour (main.c:398-400's cast, alpha 255).
MIRT_HD uint32_t denoise_channel(float c)
{
    const float v = fminf(c * 255.0f, 255.0f);   // (255 for a NaN)
    // below int's range the cast is undefined: an unspecified value, 0, instead
    return v >= -2147483648.0f ? (uint32_t)(int)v & 0xffu : 0u;
}
MIRT_HD uint32_t denoise_display(const DenoiseColour& c)
{
    return denoise_channel(c.r) | (denoise_channel(c.g) << 8) | (denoise_channel(c.b) << 16) | 0xff000000u;
}

}  // namespace mirt

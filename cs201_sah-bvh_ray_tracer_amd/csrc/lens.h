// The thin lens of a lens frame (mirt_render_lens_frame*, mirt_lens_rays;
// include/mirt.h mirt_lens), stated once for the host and the kernels. Under
// -ffp-contract=off every operation below is one correctly rounded binary32
// operation, in the order written (tests/lens_frame_cases.py restates it in
// numpy, bit for bit). For pixel (x, y) of RNG sample s:
//
//   key       = pixel_key(seed, y * width + x, s), the frame's own
//   (p, d)    = the pinhole's ray of that pixel and sample (camera_ray, with
//               the frame's jitter if set)
//   (a, b)    = a point of the unit disc by rejection: try i = 0 .. 15 draws
//               a from draw(key, kLensDraw0 + 2i), b from kLensDraw0 + 2i + 1,
//               each (float)draw / 2^31 * 2 - 1; the first try with
//               a * a + b * b < 1 is taken, and (0, 0) if none is
//   origin    = (p + L * a) + U * b, L = right * aperture, U = up * aperture
//   direction = normalised ((p + d * focus) - origin)
//
// The draws lie where neither the bounce sampling (k = 0, 1, ...) nor the
// jitter reaches (rng.h), so the bounce pass of a lens frame is a plain
// frame's. aperture == 0 never gets here: those frames are plain frames.
#pragma once
#include <cmath>

#include "../../include/mirt.h"
#include "rng.h"

namespace mirt {

constexpr int kLensTries = 16;

// What the lens kernels take beside FrameConst: L, U (computed on the host,
// per component, once per frame) and the focus distance.
struct LensConst {
    float lx, ly, lz;
    float ux, uy, uz;
    float focus;
};

inline bool lens_valid(const mirt_lens* l)
{
    return l && std::isfinite(l->aperture) && l->aperture >= 0.0f && std::isfinite(l->focus) && l->focus > 0.0f;
}

inline LensConst lens_const(const mirt_camera* cam, const mirt_lens* l)
{
    const float ap = l->aperture;
    return LensConst{cam->right.x * ap, cam->right.y * ap, cam->right.z * ap,
                     cam->up.x * ap,    cam->up.y * ap,    cam->up.z * ap,    l->focus};
}

// The pixel's point of the unit disc. Returns the number of tries made (1 ..
// kLensTries; kLensTries + 1: none was accepted, the point is the centre).
MIRT_HD int lens_point(uint64_t key, float& a, float& b)
{
#if defined(__clang__)
#pragma unroll 1
#endif
    for (int i = 0; i < kLensTries; i++) {
        const float qa = (float)draw(key, kLensDraw0 + 2u * (uint32_t)i) / 2147483648.0f;
        const float qb = (float)draw(key, kLensDraw0 + 2u * (uint32_t)i + 1u) / 2147483648.0f;
        a = qa * 2.0f - 1.0f;
        b = qb * 2.0f - 1.0f;
        float q = a * a;
        q = q + b * b;
        if (q < 1.0f) return i + 1;
    }
    a = b = 0.0f;
    return kLensTries + 1;
}

// The lens ray of the pinhole ray (p, d) under `key`: its origin o and its
// direction n BEFORE normalisation (the kernels' normalize3 follows; a zero
// length stays zero there).
MIRT_HD void lens_ray(const LensConst& lc, uint64_t key, const float p[3], const float d[3], float o[3], float n[3])
{
    float a, b;
    (void)lens_point(key, a, b);
    o[0] = (p[0] + lc.lx * a) + lc.ux * b;
    o[1] = (p[1] + lc.ly * a) + lc.uy * b;
    o[2] = (p[2] + lc.lz * a) + lc.uz * b;
    const float fx = p[0] + d[0] * lc.focus, fy = p[1] + d[1] * lc.focus, fz = p[2] + d[2] * lc.focus;
    n[0] = fx - o[0];
    n[1] = fy - o[1];
    n[2] = fz - o[2];
}

}  // namespace mirt

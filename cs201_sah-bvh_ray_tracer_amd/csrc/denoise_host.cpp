// mirt_denoise_host: the filter of csrc/denoise.h on the host. No HIP call, no
// ctx: the reference the device form is checked against, byte for byte.
#include <cstring>
#include <new>
#include <vector>

#include "denoise.h"
#include "internal.h"

namespace mirt {

bool denoise_args_valid(int width, int height, const void* rgba, const void* accum, int frames, const void* sphere,
                        const mirt_denoise_params* params, const void* out, const void* out_rgb)
{
    return denoise_params_valid(params) && sphere && (rgba != nullptr) != (accum != nullptr) &&
           (!accum || frames >= 1) && (out || out_rgb) && denoise_size_valid(width, height);
}

namespace {

struct HostAt {
    const DenoiseColour* c;
    const float* n;   // the caller's plane, three floats per pixel, or null
    int width;
    DenoiseColour colour(int x, int y) const { return c[(size_t)y * width + x]; }
    DenoiseNormal normal(int x, int y) const
    {
        if (!n) return DenoiseNormal{};
        const float* p = n + 3 * ((size_t)y * width + x);
        return DenoiseNormal{p[0], p[1], p[2], 0.0f};
    }
};

}  // namespace
}  // namespace mirt

extern "C" {

void mirt_denoise_params_default(mirt_denoise_params* out)
{
    if (!out) return;
    out->passes = 3;
    out->normal_sharpness = 3;
    out->sigma_colour = 0.0f;
}

int mirt_denoise_host(int width, int height, const mirt_rgba8* rgba, const float* accum, int frames,
                      const int32_t* sphere, const float* normal, const mirt_denoise_params* params, mirt_rgba8* out,
                      float* out_rgb)
try {
    using namespace mirt;
    if (!denoise_args_valid(width, height, rgba, accum, frames, sphere, params, out, out_rgb)) {
        set_error("mirt_denoise_host: invalid arguments");
        return MIRT_E_INVALID;
    }
    const size_t n = (size_t)width * height;
    std::vector<DenoiseColour> a(n), b(params->passes > 1 ? n : 0);
    for (size_t i = 0; i < n; i++) {
        if (rgba) {
            uint32_t px;
            std::memcpy(&px, &rgba[i], 4);
            a[i] = denoise_source_rgba(px, sphere[i]);
        } else {
            a[i] = denoise_source_accum(accum + 3 * i, frames, sphere[i]);
        }
    }
    DenoiseColour *src = a.data(), *dst = b.data();
    for (int pass = 0; pass < params->passes; pass++) {
        const bool last = pass == params->passes - 1;
        const HostAt at{src, normal, width};
        const float inv = denoise_inv(params->sigma_colour, pass);
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const DenoiseColour c = denoise_pixel(at, width, height, x, y, 1 << pass, normal != nullptr,
                                                      params->normal_sharpness, inv);
                const size_t i = (size_t)y * width + x;
                if (!last) {
                    dst[i] = c;
                    continue;
                }
                if (out_rgb) {
                    out_rgb[3 * i] = c.r;
                    out_rgb[3 * i + 1] = c.g;
                    out_rgb[3 * i + 2] = c.b;
                }
                if (out) {
                    const uint32_t px = denoise_display(c);
                    std::memcpy(&out[i], &px, 4);
                }
            }
        DenoiseColour* t = src;
        src = dst;
        dst = t;
    }
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    mirt::set_error("mirt_denoise_host: out of host memory");
    return MIRT_E_NOMEM;
}

}  // extern "C"

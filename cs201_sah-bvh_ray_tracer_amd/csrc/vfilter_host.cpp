// mirt_denoise_var_host: the variance-guided filter of csrc/vfilter.h on the
// host. No HIP call, no ctx: the reference the device form is checked against,
// byte for byte.
#include <cstring>
#include <new>
#include <vector>

#include "internal.h"
#include "vfilter.h"

namespace mirt {

bool vfilter_args_valid(int width, int height, const void* hist, const void* m2, const void* sphere,
                        const mirt_denoise_var_params* params, const void* out, const void* out_rgb)
{
    return vfilter_params_valid(params) && hist && m2 && sphere && (out || out_rgb) && denoise_size_valid(width, height);
}

bool vfilter_params_ok(const mirt_denoise_var_params* params) { return vfilter_params_valid(params); }

namespace {

// the caller's planes, for V1 - V2
struct HostIn {
    const mirt_history_px* h;
    const int32_t* s;
    int width;
    mirt_history_px hist(int x, int y) const { return h[(size_t)y * width + x]; }
    int32_t sphere(int x, int y) const { return s[(size_t)y * width + x]; }
};

struct HostAt {
    const VfColour* c;
    const VfGuide* g;
    int width;
    VfColour colour(int x, int y) const { return c[(size_t)y * width + x]; }
    VfGuide guide(int x, int y) const { return g[(size_t)y * width + x]; }
};

}  // namespace
}  // namespace mirt

extern "C" {

void mirt_denoise_var_params_default(mirt_denoise_var_params* out)
{
    if (!out) return;
    out->passes = 3;
    out->normal_sharpness = 3;
    out->sigma_lum = 8.0f;   // the best of {1, 2, 4, 8} on the CPU quality test: DESIGN.md 9.14 has the four errors
    out->min_history = 4;
}

int mirt_denoise_var_host(int width, int height, const mirt_history_px* hist, const float* m2, const int32_t* sphere,
                          const float* normal, const mirt_denoise_var_params* params, mirt_rgba8* out, float* out_rgb,
                          float* var_out)
try {
    using namespace mirt;
    if (!vfilter_args_valid(width, height, hist, m2, sphere, params, out, out_rgb)) {
        set_error("mirt_denoise_var_host: invalid arguments");
        return MIRT_E_INVALID;
    }
    const size_t n = (size_t)width * height;
    std::vector<VfColour> a(n), b(params->passes > 1 ? n : 0);
    std::vector<VfGuide> g(n);
    const HostIn in{hist, sphere, width};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            const float var = vfilter_variance(in, width, height, x, y, hist[i], m2[i], sphere[i], params->min_history);
            a[i] = VfColour{hist[i].r, hist[i].g, hist[i].b, var};
            g[i] = normal ? VfGuide{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], sphere[i]}
                          : VfGuide{0.0f, 0.0f, 0.0f, sphere[i]};
            if (var_out) var_out[i] = var;
        }
    const float sl2 = vfilter_sl2(params->sigma_lum);
    VfColour *src = a.data(), *dst = b.data();
    for (int pass = 0; pass < params->passes; pass++) {
        const bool last = pass == params->passes - 1;
        const HostAt at{src, g.data(), width};
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const VfColour c =
                    vfilter_pixel(at, width, height, x, y, 1 << pass, normal != nullptr, params->normal_sharpness, sl2);
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
                    const uint32_t px = vfilter_display(c);
                    std::memcpy(&out[i], &px, 4);
                }
            }
        VfColour* t = src;
        src = dst;
        dst = t;
    }
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    mirt::set_error("mirt_denoise_var_host: out of host memory");
    return MIRT_E_NOMEM;
}

}  // extern "C"

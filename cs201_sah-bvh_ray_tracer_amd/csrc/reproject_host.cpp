// mirt_reproject_host: the reprojection of csrc/reproject.h on the host. No
// HIP call, no ctx: the reference the device form is checked against, byte
// for byte.
#include <cstring>

#include "internal.h"
#include "reproject.h"

namespace mirt {

bool reproject_args_valid(int width, int height, const void* cam, const void* cam_prev, const void* rgba, const void* t,
                          const void* sphere, const void* hist, const void* t_prev, const void* sphere_prev,
                          const mirt_reproject_params* params, const void* hist_out)
{
    const int prev = (cam_prev != nullptr) + (hist != nullptr) + (t_prev != nullptr) + (sphere_prev != nullptr);
    return reproject_params_valid(params) && cam && rgba && t && sphere && hist_out && (prev == 0 || prev == 4) &&
           hist_out != hist && denoise_size_valid(width, height);
}

namespace {

struct HostAt {
    const mirt_history_px* h;
    const float* tp;
    const int32_t* sp;
    mirt_history_px hist(size_t q) const { return h[q]; }
    float t(size_t q) const { return tp[q]; }
    int32_t sphere(size_t q) const { return sp[q]; }
};

}  // namespace
}  // namespace mirt

extern "C" {

void mirt_reproject_params_default(mirt_reproject_params* out)
{
    if (!out) return;
    out->max_history = 64;
    out->taps = 4;
    out->t_tolerance = 0.015625f;
}

int mirt_reproject_host(int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                        const mirt_rgba8* rgba, const float* t, const int32_t* sphere, const mirt_history_px* hist,
                        const float* t_prev, const int32_t* sphere_prev, const mirt_reproject_params* params,
                        mirt_history_px* hist_out, mirt_rgba8* out, float* out_rgb)
{
    using namespace mirt;
    if (!reproject_args_valid(width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out)) {
        set_error("mirt_reproject_host: invalid arguments");
        return MIRT_E_INVALID;
    }
    const ReprojectCam cur = reproject_cam(cam, width, height);
    const ReprojectCam prv = cam_prev ? reproject_cam(cam_prev, width, height) : ReprojectCam{};
    const bool prev = cam_prev != nullptr;
    const HostAt at{hist, t_prev, sphere_prev};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            uint32_t px;
            std::memcpy(&px, &rgba[i], 4);
            int kind;
            const mirt_history_px h =
                params->taps == 1
                    ? reproject_pixel<1>(cur, prv, prev, at, width, x, y, px, t[i], sphere[i], params->max_history,
                                         params->t_tolerance, &kind)
                    : reproject_pixel<4>(cur, prv, prev, at, width, x, y, px, t[i], sphere[i], params->max_history,
                                         params->t_tolerance, &kind);
            hist_out[i] = h;
            if (out_rgb) {
                out_rgb[3 * i] = h.r;
                out_rgb[3 * i + 1] = h.g;
                out_rgb[3 * i + 2] = h.b;
            }
            if (out) {
                const uint32_t d = reproject_display(h);
                std::memcpy(&out[i], &d, 4);
            }
        }
    return MIRT_OK;
}

}  // extern "C"

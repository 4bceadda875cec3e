// mirt_reproject_host, mirt_reproject_motion_host and
// mirt_reproject_moments_host: the reprojection of csrc/reproject.h on the host. No HIP call, no ctx: the reference the device
// forms are checked against, byte for byte.
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

bool reproject_moments_valid(const void* hist, const mirt_sphere_motion* motion, bool has_prev, const void* m2_prev,
                             const void* m2_out)
{
    return (!motion || reproject_motion_valid(motion, has_prev)) && (m2_prev != nullptr) == (hist != nullptr) && m2_out &&
           m2_out != m2_prev;
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
// the moments form's: m2_prev too, and where the pixel's new m2 goes
struct HostAtM2 : HostAt {
    const float* m2p;
    float* m2_new;
    float m2(size_t q) const { return m2p[q]; }
};

// a mirt_sphere_motion of host pointers, as reproject_moved reads it
struct HostMotion {
    const float *g, *gp;
    const int32_t* idx;
    int32_t num_spheres, num_prev;
    bool has_index() const { return idx != nullptr; }
    int32_t index(int32_t i) const { return idx[i]; }
    void geo(int32_t i, float out[4]) const { std::memcpy(out, g + 4 * (size_t)i, 16); }
    void geo_prev(int32_t i, float out[4]) const { std::memcpy(out, gp + 4 * (size_t)i, 16); }
};

// the loop of the host forms over VALID arguments (motion: null for the plain one; m2_out: with a HostAtM2)
template <int TAPS, class At>
void reproject_image(int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev, const mirt_rgba8* rgba,
                     const float* t, const int32_t* sphere, At at, const mirt_reproject_params* params,
                     mirt_history_px* hist_out, mirt_rgba8* out, float* out_rgb, const mirt_sphere_motion* motion,
                     float* m2_out = nullptr)
{
    const ReprojectCam cur = reproject_cam(cam, width, height);
    const ReprojectCam prv = cam_prev ? reproject_cam(cam_prev, width, height) : ReprojectCam{};
    const bool prev = cam_prev != nullptr;
    const HostMotion mo = motion ? HostMotion{motion->geo, motion->geo_prev, motion->prev_index, motion->num_spheres,
                                              motion->num_prev}
                                 : HostMotion{};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            uint32_t px;
            std::memcpy(&px, &rgba[i], 4);
            int kind;
            if constexpr (reproject_at_moments<At>::value) at.m2_new = m2_out + i;
            const mirt_history_px h =
                motion ? reproject_pixel<TAPS>(cur, prv, prev, at, width, x, y, px, t[i], sphere[i], params->max_history,
                                               params->t_tolerance, &kind, reproject_moved(mo, sphere[i]))
                       : reproject_pixel<TAPS>(cur, prv, prev, at, width, x, y, px, t[i], sphere[i], params->max_history,
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
}

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
    const HostAt at{hist, t_prev, sphere_prev};
    if (params->taps == 1)
        reproject_image<1>(width, height, cam, cam_prev, rgba, t, sphere, at, params, hist_out, out, out_rgb, nullptr);
    else
        reproject_image<4>(width, height, cam, cam_prev, rgba, t, sphere, at, params, hist_out, out, out_rgb, nullptr);
    return MIRT_OK;
}

int mirt_reproject_motion_host(int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                               const mirt_rgba8* rgba, const float* t, const int32_t* sphere,
                               const mirt_history_px* hist, const float* t_prev, const int32_t* sphere_prev,
                               const mirt_reproject_params* params, mirt_history_px* hist_out, mirt_rgba8* out,
                               float* out_rgb, const mirt_sphere_motion* motion)
{
    using namespace mirt;
    if (!reproject_args_valid(width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out) ||
        !reproject_motion_valid(motion, cam_prev != nullptr)) {
        set_error("mirt_reproject_motion_host: invalid arguments");
        return MIRT_E_INVALID;
    }
    const HostAt at{hist, t_prev, sphere_prev};
    if (params->taps == 1)
        reproject_image<1>(width, height, cam, cam_prev, rgba, t, sphere, at, params, hist_out, out, out_rgb, motion);
    else
        reproject_image<4>(width, height, cam, cam_prev, rgba, t, sphere, at, params, hist_out, out, out_rgb, motion);
    return MIRT_OK;
}

int mirt_reproject_moments_host(int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                                const mirt_rgba8* rgba, const float* t, const int32_t* sphere,
                                const mirt_history_px* hist, const float* t_prev, const int32_t* sphere_prev,
                                const mirt_reproject_params* params, mirt_history_px* hist_out, mirt_rgba8* out,
                                float* out_rgb, const mirt_sphere_motion* motion, const float* m2_prev, float* m2_out)
{
    using namespace mirt;
    if (!reproject_args_valid(width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out) ||
        !reproject_moments_valid(hist, motion, cam_prev != nullptr, m2_prev, m2_out)) {
        set_error("mirt_reproject_moments_host: invalid arguments");
        return MIRT_E_INVALID;
    }
    const HostAtM2 at{{hist, t_prev, sphere_prev}, m2_prev, nullptr};
    if (params->taps == 1)
        reproject_image<1>(width, height, cam, cam_prev, rgba, t, sphere, at, params, hist_out, out, out_rgb,
                                 motion, m2_out);
    else
        reproject_image<4>(width, height, cam, cam_prev, rgba, t, sphere, at, params, hist_out, out, out_rgb,
                                 motion, m2_out);
    return MIRT_OK;
}

}  // extern "C"

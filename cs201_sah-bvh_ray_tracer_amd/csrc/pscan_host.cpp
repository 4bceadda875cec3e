// Host entry points over the arithmetic of pscan.h, which the kernels of the
// primary scan share (mirt_pscan_camera, mirt_pscan_records): what
// tests/test_pscan_host.py checks on the CPU is the code the device compiles.
#include <cmath>
#include <vector>

#include "internal.h"
#include "pscan.h"

using namespace mirt;

namespace {

// The camera of a width x height frame as the frame kernels see it: the
// expressions of render.hip's make_frame_const (ray.c:18-24, main.c:356).
PscanFrame frame_of(const mirt_camera* cam, int width, int height)
{
    PscanFrame f{};
    const float aspect = (float)width / (float)height;
    const float fov_rad = (float)((double)cam->fov * (M_PI / 180.0));
    const float half_h = (float)std::tan((double)(fov_rad / 2.0f));
    const float half_w = aspect * half_h;
    const float sw = 2.0f * half_w, sh = 2.0f * half_h;
    f.p[0] = cam->position.x; f.p[1] = cam->position.y; f.p[2] = cam->position.z;
    f.f[0] = cam->forward.x; f.f[1] = cam->forward.y; f.f[2] = cam->forward.z;
    f.h[0] = cam->right.x * sw; f.h[1] = cam->right.y * sw; f.h[2] = cam->right.z * sw;
    f.v[0] = cam->up.x * sh; f.v[1] = cam->up.y * sh; f.v[2] = cam->up.z * sh;
    f.aspect = aspect;
    f.wf = (float)width;
    f.hf = (float)height;
    f.width = width;
    f.height = height;
    f.fov = cam->fov;
    return f;
}

}  // namespace

extern "C" int mirt_pscan_camera(const mirt_camera* cam, int width, int height, float* g, double* rho)
{
    if (!cam || width < 1 || height < 1) {
        set_error("mirt_pscan_camera: invalid arguments");
        return MIRT_E_INVALID;
    }
    PscanCam c{};
    const int why = pscan_camera(frame_of(cam, width, height), &c);
    if (why != PSCAN_CAM_OK) return why;
    if (g) g[0] = c.g[0], g[1] = c.g[1], g[2] = c.g[2];
    if (rho) *rho = c.rho;
    return PSCAN_CAM_OK;
}

extern "C" int mirt_pscan_records(const mirt_camera* cam, int width, int height, const float* geo, int64_t n, float* z,
                                  int32_t* rect, double* reach)
{
    if (!cam || width < 1 || height < 1 || n < 0 || (n > 0 && (!geo || !z || !rect))) {
        set_error("mirt_pscan_records: invalid arguments");
        return MIRT_E_INVALID;
    }
    PscanCam c{};
    const int why = pscan_camera(frame_of(cam, width, height), &c);
    if (why != PSCAN_CAM_OK) return why;
    std::vector<PscanPlanes> planes((size_t)c.ntx + c.nty);
    for (int i = 0; i < c.ntx; i++) planes[i] = pscan_column(c, i);
    for (int j = 0; j < c.nty; j++) planes[c.ntx + j] = pscan_row(c, j);
    for (int64_t k = 0; k < n; k++) {
        const float* s = geo + 4 * k;
        const PscanRec r = pscan_record(c, planes.data(), planes.data() + c.ntx, (uint32_t)k, s[0], s[1], s[2], s[3]);
        z[k] = r.z;
        rect[4 * k] = (int32_t)(r.cols & 0xffffu);
        rect[4 * k + 1] = (int32_t)(r.cols >> 16);
        rect[4 * k + 2] = (int32_t)(r.rows & 0xffffu);
        rect[4 * k + 3] = (int32_t)(r.rows >> 16);
        if (reach) {
            const double cc[3] = {s[0], s[1], s[2]};
            const double w[3] = {cc[0] - c.o[0], cc[1] - c.o[1], cc[2] - c.o[2]};
            reach[k] = pscan_reach(c, w, cc, s[3]);
        }
    }
    return MIRT_OK;
}

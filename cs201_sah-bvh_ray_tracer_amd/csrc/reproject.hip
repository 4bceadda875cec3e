// mirt_reproject_device / mirt_reproject, and the history a ctx keeps for
// mirt_render_frame_reprojected: the reprojection of csrc/reproject.h on the
// device, byte for byte what mirt_reproject_host gives.
//
// One thread per pixel, 64 x 4 pixels per workgroup with the lanes of a wave
// along x: the pixel's own rgba, t and sphere are loaded together, the hit
// point is carried to the previous camera, and the taps' records (16 B), t and
// sphere (4 B each) are loaded before any is used. Neighbouring lanes reproject
// to neighbouring previous pixels, so the gathers coalesce for any coherent
// motion. A tap's position is data: it is compared with the image as floats
// and becomes an index only when inside (a tap outside reads the pixel's own
// index and is dropped), so whatever t holds no access leaves the buffers.
// The counts of mirt_history_stats are one ballot and popcount per wave and
// kind and one vector atomic add per wave into a three-word device record.
// No loop, no workgroup waits on another.
//
// With a motion (mirt_reproject_motion*; reproject_kernel's MOTION instances)
// a dependent chain stands in front of the gather: sphere[i] -> geo[s] (16 B)
// and prev_index[s] (4 B), issued together -> geo_prev[sp] (one 16-byte load)
// -> the taps. All of it is unconditional, as t's load is: a sky pixel and an
// index out of range read element 0 and are dropped (reproject.h
// reproject_moved), so the chain's loads are in flight while the pixel's
// direction is computed. The sphere arrays are small beside the image (16 B x
// spheres) and neighbouring lanes mostly see the same sphere: after the first
// touch these are L2 / TCP hits. No scratch, no LDS, no loop.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "device_util.h"
#include "internal.h"
#include "reproject.h"

#pragma clang fp contract(off)

namespace mirt {

// The history of mirt_render_frame_reprojected: a ping-pong pair of records
// and planes, the display, and the counts, in one allocation that only grows.
//   [counts: kHead bytes][records 0][records 1][t 0][sphere 0][t 1][sphere 1][display]
struct ReprojectState {
    void* d = nullptr;
    size_t cap = 0;
    bool valid = false;       // half `cur` holds the previous call's frame
    int cur = 0;
    int width = 0, height = 0;
    uint64_t scene_id = 0, frames = 0;
    mirt_camera cam{};        // the previous call's
    uint64_t next_scene_id = 0;   // of the frame between frame_begin and frame_end
    bool carry = false;       // frame_begin kept the history over a link: frame_end reprojects with its motion
    bool carried = false;     // the last mirt_render_frame_reprojected did (mirt_history_motion_get)
    // mirt_render_frame_reprojected_denoised: an allocation of its own, made by the first such call, that only grows
    //   [m2 0][m2 1][normal][filtered display]
    void* dm = nullptr;
    size_t mcap = 0;
    bool moments = false;     // half `cur`'s records have their m2 in m2[cur]
};

void reproject_state_free(ReprojectState* st)
{
    if (!st) return;
    if (st->d) (void)hipFree(st->d);
    if (st->dm) (void)hipFree(st->dm);
    delete st;
}

}  // namespace mirt

namespace {

using namespace mirt;

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 4;   // a wave per row of 64 pixels
constexpr size_t kHead = 256;            // the counts, and the records' alignment

struct ReprojectArgs {
    ReprojectCam cur, prev;
    int has_prev;
    int width, height, tiles_x;
    int max_history;
    float t_tolerance;
    const uint32_t* rgba;   // (may be `out`: a thread reads its pixel before it writes it)
    const float* t;
    const int32_t* sphere;
    const mirt_history_px* hist;
    const float* t_prev;
    const int32_t* sphere_prev;
    mirt_history_px* hist_out;
    uint32_t* out;
    float* out_rgb;
    uint32_t* counts;       // [kReprojectSky, kReprojectFresh, kReprojectReused], or null
};

struct GlobalAt {
    const mirt_history_px* h;
    const float* tp;
    const int32_t* sp;
    __device__ mirt_history_px hist(size_t q) const { return h[q]; }
    __device__ float t(size_t q) const { return tp[q]; }
    __device__ int32_t sphere(size_t q) const { return sp[q]; }
};

// a mirt_sphere_motion of device pointers, as reproject_moved reads it: one 16-byte load per sphere
struct MotionArgs {
    const float4* g;
    const float4* gp;
    const int32_t* idx;
    int32_t num_spheres, num_prev;
    __device__ bool has_index() const { return idx != nullptr; }   // (uniform)
    __device__ int32_t index(int32_t i) const { return idx[i]; }
    __device__ void geo(int32_t i, float out[4]) const
    {
        const float4 v = g[i];
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    }
    __device__ void geo_prev(int32_t i, float out[4]) const
    {
        const float4 v = gp[i];
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    }
};

// MOTION: none (the plain reprojection, whose code the pack leaves as it was), or one MotionArgs
template <int TAPS, class... MOTION>
__global__ void __launch_bounds__(kBlock) reproject_kernel(const ReprojectArgs a, const MOTION... mo)
{
    const int bx = (int)(blockIdx.x % (unsigned)a.tiles_x), by = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int x = bx * kTileW + (int)(threadIdx.x % kTileW), y = by * kTileH + (int)(threadIdx.x / kTileW);
    int kind = -1;   // (a lane outside the image counts as nothing; it stays for the ballots)
    if (x < a.width && y < a.height) {
        const size_t i = (size_t)y * a.width + x;
        const uint32_t px = a.rgba[i];
        float t = a.t[i];
        const int32_t s = a.sphere[i];
        // (t is used by hit pixels only; kept out of their branch so that the three loads are issued together)
        asm volatile("" : "+v"(t));
        const GlobalAt at{a.hist, a.t_prev, a.sphere_prev};
        // (MOTION: the sphere's loads follow s at once, for every lane)
        const mirt_history_px h = reproject_pixel<TAPS>(a.cur, a.prev, a.has_prev != 0, at, a.width, x, y, px, t, s,
                                                        a.max_history, a.t_tolerance, &kind, reproject_moved(mo, s)...);
        a.hist_out[i] = h;
        if (a.out_rgb) {
            a.out_rgb[3 * i] = h.r;
            a.out_rgb[3 * i + 1] = h.g;
            a.out_rgb[3 * i + 2] = h.b;
        }
        if (a.out) a.out[i] = reproject_display(h);
    }
    if (!a.counts) return;   // (uniform)
    const bool first = (threadIdx.x & 63u) == 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned long long m = __ballot(kind == k);
        if (first && m) atomicAdd(&a.counts[k], (uint32_t)__popcll(m));
    }
}

// With MOMENTS (mirt_reproject_moments*): the same thread per pixel; a tap's
// m2_prev[q] (4 B) is issued with its record, t and sphere, and the pixel's
// m2_out is one more 4-byte store. Kernels of their own, so that the
// instances above stay the code they were.
struct MomentArgs {
    const float* m2_prev;
    float* m2_out;
};

struct GlobalAtM2 {
    const mirt_history_px* h;
    const float* tp;
    const int32_t* sp;
    const float* m2p;
    float* m2_new;   // the pixel's new m2 (a register of the calling thread)
    __device__ mirt_history_px hist(size_t q) const { return h[q]; }
    __device__ float t(size_t q) const { return tp[q]; }
    __device__ int32_t sphere(size_t q) const { return sp[q]; }
    __device__ float m2(size_t q) const { return m2p[q]; }
};

template <int TAPS, class... MOTION>
__global__ void __launch_bounds__(kBlock)
reproject_moments_kernel(const ReprojectArgs a, const MomentArgs mm, const MOTION... mo)
{
    const int bx = (int)(blockIdx.x % (unsigned)a.tiles_x), by = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int x = bx * kTileW + (int)(threadIdx.x % kTileW), y = by * kTileH + (int)(threadIdx.x / kTileW);
    int kind = -1;
    if (x < a.width && y < a.height) {
        const size_t i = (size_t)y * a.width + x;
        const uint32_t px = a.rgba[i];
        float t = a.t[i];
        const int32_t s = a.sphere[i];
        asm volatile("" : "+v"(t));
        float m2_new;
        const GlobalAtM2 at{a.hist, a.t_prev, a.sphere_prev, mm.m2_prev, &m2_new};
        const mirt_history_px h = reproject_pixel<TAPS>(a.cur, a.prev, a.has_prev != 0, at, a.width, x, y, px, t, s,
                                                        a.max_history, a.t_tolerance, &kind, reproject_moved(mo, s)...);
        a.hist_out[i] = h;
        mm.m2_out[i] = m2_new;
        if (a.out_rgb) {
            a.out_rgb[3 * i] = h.r;
            a.out_rgb[3 * i + 1] = h.g;
            a.out_rgb[3 * i + 2] = h.b;
        }
        if (a.out) a.out[i] = reproject_display(h);
    }
    if (!a.counts) return;   // (uniform)
    const bool first = (threadIdx.x & 63u) == 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned long long m = __ballot(kind == k);
        if (first && m) atomicAdd(&a.counts[k], (uint32_t)__popcll(m));
    }
}

unsigned tile_count(int width, int height, int* tiles_x)
{
    // (width * height <= 2^31, so the count fits an unsigned and a grid's x)
    const uint64_t tx = ((uint64_t)width + kTileW - 1) / kTileW, ty = ((uint64_t)height + kTileH - 1) / kTileH;
    *tiles_x = (int)tx;
    return (unsigned)(tx * ty);
}

// the reprojection of VALID arguments, all in device memory, enqueued on `s`
int reproject_enqueue(mirt_ctx* c, int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                      const uint32_t* d_rgba, const float* d_t, const int32_t* d_sphere, const mirt_history_px* d_hist,
                      const float* d_t_prev, const int32_t* d_sphere_prev, const mirt_reproject_params* p,
                      mirt_history_px* d_hist_out, uint32_t* d_out, float* d_out_rgb, uint32_t* d_counts, hipStream_t s,
                      const mirt_sphere_motion* motion = nullptr,   // (valid, device pointers; null: the plain form)
                      const float* d_m2_prev = nullptr, float* d_m2_out = nullptr)   // (d_m2_out: the moments form)
{
    HIP_TRY(hipSetDevice(ctx_device(c)));
    if (int rc = ctx_launch_begin(c, s, false)) return rc;
    ReprojectArgs a{};
    a.cur = reproject_cam(cam, width, height);
    a.has_prev = cam_prev != nullptr;
    if (cam_prev) a.prev = reproject_cam(cam_prev, width, height);
    a.width = width;
    a.height = height;
    a.max_history = p->max_history;
    a.t_tolerance = p->t_tolerance;
    a.rgba = d_rgba;
    a.t = d_t;
    a.sphere = d_sphere;
    a.hist = d_hist;
    a.t_prev = d_t_prev;
    a.sphere_prev = d_sphere_prev;
    a.hist_out = d_hist_out;
    a.out = d_out;
    a.out_rgb = d_out_rgb;
    a.counts = d_counts;
    if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, 3 * sizeof(uint32_t), s));
    const unsigned g = tile_count(width, height, &a.tiles_x);
    if (d_m2_out) {
        const MomentArgs mm{d_m2_prev, d_m2_out};
        if (motion) {
            const MotionArgs mo{(const float4*)motion->geo, (const float4*)motion->geo_prev, motion->prev_index,
                                motion->num_spheres, motion->num_prev};
            if (p->taps == 1)
                reproject_moments_kernel<1><<<g, kBlock, 0, s>>>(a, mm, mo);
            else
                reproject_moments_kernel<4><<<g, kBlock, 0, s>>>(a, mm, mo);
        } else if (p->taps == 1)
            reproject_moments_kernel<1><<<g, kBlock, 0, s>>>(a, mm);
        else
            reproject_moments_kernel<4><<<g, kBlock, 0, s>>>(a, mm);
    } else if (motion) {
        const MotionArgs mo{(const float4*)motion->geo, (const float4*)motion->geo_prev, motion->prev_index,
                            motion->num_spheres, motion->num_prev};
        if (p->taps == 1)
            reproject_kernel<1><<<g, kBlock, 0, s>>>(a, mo);
        else
            reproject_kernel<4><<<g, kBlock, 0, s>>>(a, mo);
    } else if (p->taps == 1)
        reproject_kernel<1><<<g, kBlock, 0, s>>>(a);
    else
        reproject_kernel<4><<<g, kBlock, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return ctx_launch_end(c, s);
}

// the parts of a state's allocation for an image of n pixels
struct Parts {
    uint32_t* counts;
    mirt_history_px* rec[2];
    float* t[2];
    int32_t* sphere[2];
    uint32_t* display;
};
size_t state_bytes(size_t n) { return kHead + 2 * sizeof(mirt_history_px) * n + 4 * 4 * n + 4 * n; }
Parts state_parts(const ReprojectState* st, size_t n)
{
    char* const b = (char*)st->d;
    Parts p;
    p.counts = (uint32_t*)b;
    p.rec[0] = (mirt_history_px*)(b + kHead);
    p.rec[1] = p.rec[0] + n;
    p.t[0] = (float*)(p.rec[1] + n);
    p.sphere[0] = (int32_t*)(p.t[0] + n);
    p.t[1] = (float*)(p.sphere[0] + n);
    p.sphere[1] = (int32_t*)(p.t[1] + n);
    p.display = (uint32_t*)(p.sphere[1] + n);
    return p;
}
// the parts of the moments' allocation
struct MomentParts {
    float* m2[2];
    float* normal;
    uint32_t* filtered;
};
size_t moment_bytes(size_t n) { return 2 * 4 * n + 12 * n + 4 * n; }
MomentParts moment_parts(const ReprojectState* st, size_t n)
{
    float* const b = (float*)st->dm;
    return MomentParts{{b, b + n}, b + 2 * n, (uint32_t*)(b + 5 * n)};
}

}  // namespace

// ---- the ctx's history (render.hip's mirt_render_frame_reprojected drives these two around its frame)

int mirt::reproject_frame_begin(mirt_ctx* c, int width, int height, uint64_t scene_id, uint64_t link_from, float** d_t,
                                int32_t** d_sphere, const char* fn, bool moments, float** d_normal)
{
    ReprojectState** slot = ctx_reproject_state(c);
    if (!*slot) *slot = new (std::nothrow) ReprojectState();
    ReprojectState* st = *slot;
    if (!st) {
        set_error("%s: out of host memory", fn);
        return MIRT_E_NOMEM;
    }
    // (a history without moments cannot feed a frame that carries them: it empties first)
    if (moments && st->valid && !st->moments) {
        st->valid = false;
        st->frames = 0;
    }
    // (link_from: the scene the slot's link to `scene_id` starts at, 0 without one the ctx may use)
    st->carry = st->valid && st->width == width && st->height == height && st->scene_id != scene_id && link_from != 0 &&
                st->scene_id == link_from;
    st->carried = false;
    if (st->valid && !st->carry && (st->width != width || st->height != height || st->scene_id != scene_id)) {
        st->valid = false;
        st->frames = 0;
    }
    const size_t n = (size_t)width * height, bytes = state_bytes(n);
    if (bytes > st->cap) {
        // (a change of size emptied the history; the calls that use the buffer are blocking: nothing of it is in flight)
        if (st->d) (void)hipFree(st->d);
        st->d = nullptr;
        st->cap = 0;
        st->valid = false;
        st->carry = false;
        st->frames = 0;
        HIP_TRY(hipMalloc(&st->d, bytes));
        st->cap = bytes;
    }
    if (moments && moment_bytes(n) > st->mcap) {
        // (a change of size emptied the history, and m2 with it; otherwise this is the first such call on records
        // without moments, emptied above)
        if (st->dm) (void)hipFree(st->dm);
        st->dm = nullptr;
        st->mcap = 0;
        if (st->moments) {
            st->valid = false;
            st->carry = false;
            st->frames = 0;
        }
        HIP_TRY(hipMalloc(&st->dm, moment_bytes(n)));
        st->mcap = moment_bytes(n);
    }
    st->width = width;
    st->height = height;
    // (a carried history keeps its own scene's id until the frame has been reprojected: should the frame fail, the
    // next call meets the same link again, not records that index another scene's spheres)
    st->next_scene_id = scene_id;
    if (!st->carry) st->scene_id = scene_id;
    const Parts p = state_parts(st, n);
    const int dst = st->valid ? st->cur ^ 1 : 0;
    *d_t = p.t[dst];
    *d_sphere = p.sphere[dst];
    if (moments) *d_normal = moment_parts(st, n).normal;
    return MIRT_OK;
}

int mirt::reproject_frame_end(mirt_ctx* c, const mirt_camera* cam, const uint32_t* d_rgba,
                              const mirt_reproject_params* params, const mirt_sphere_motion* link_motion,
                              const uint32_t** d_shown, hipStream_t s, bool moments)
{
    ReprojectState* st = *ctx_reproject_state(c);
    const Parts p = state_parts(st, (size_t)st->width * st->height);
    const MomentParts mp = moments ? moment_parts(st, (size_t)st->width * st->height) : MomentParts{};
    const int src = st->cur, dst = st->valid ? st->cur ^ 1 : 0;
    const bool prev = st->valid;
    const bool carry = prev && st->carry && link_motion;
    st->carry = false;
    st->valid = false;   // (until the launch below is enqueued)
    if (int rc = reproject_enqueue(c, st->width, st->height, cam, prev ? &st->cam : nullptr, d_rgba, p.t[dst],
                                   p.sphere[dst], prev ? p.rec[src] : nullptr, prev ? p.t[src] : nullptr,
                                   prev ? p.sphere[src] : nullptr, params, p.rec[dst], p.display, nullptr, p.counts, s,
                                   carry ? link_motion : nullptr, moments && prev ? mp.m2[src] : nullptr,
                                   moments ? mp.m2[dst] : nullptr))
        return rc;
    st->moments = moments;
    st->carried = carry;
    st->scene_id = st->next_scene_id;
    st->cur = dst;
    st->valid = true;
    st->cam = *cam;
    st->frames = prev ? st->frames + 1 : 1;
    *d_shown = p.display;
    return MIRT_OK;
}

extern "C" {

int mirt_reproject_device(mirt_ctx* c, int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                          const uint32_t* d_rgba, const float* d_t, const int32_t* d_sphere,
                          const mirt_history_px* d_hist, const float* d_t_prev, const int32_t* d_sphere_prev,
                          const mirt_reproject_params* params, mirt_history_px* d_hist_out, uint32_t* d_out,
                          float* d_out_rgb, void* stream)
{
    const char* fn = "mirt_reproject_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!reproject_args_valid(width, height, cam, cam_prev, d_rgba, d_t, d_sphere, d_hist, d_t_prev, d_sphere_prev,
                              params, d_hist_out)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return reproject_enqueue(c, width, height, cam, cam_prev, d_rgba, d_t, d_sphere, d_hist, d_t_prev, d_sphere_prev,
                             params, d_hist_out, d_out, d_out_rgb, nullptr, (hipStream_t)stream);
}

int mirt_reproject_motion_device(mirt_ctx* c, int width, int height, const mirt_camera* cam,
                                 const mirt_camera* cam_prev, const uint32_t* d_rgba, const float* d_t,
                                 const int32_t* d_sphere, const mirt_history_px* d_hist, const float* d_t_prev,
                                 const int32_t* d_sphere_prev, const mirt_reproject_params* params,
                                 mirt_history_px* d_hist_out, uint32_t* d_out, float* d_out_rgb, void* stream,
                                 const mirt_sphere_motion* motion)
{
    const char* fn = "mirt_reproject_motion_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!reproject_args_valid(width, height, cam, cam_prev, d_rgba, d_t, d_sphere, d_hist, d_t_prev, d_sphere_prev,
                              params, d_hist_out) ||
        !reproject_motion_valid(motion, cam_prev != nullptr)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return reproject_enqueue(c, width, height, cam, cam_prev, d_rgba, d_t, d_sphere, d_hist, d_t_prev, d_sphere_prev,
                             params, d_hist_out, d_out, d_out_rgb, nullptr, (hipStream_t)stream, motion);
}

int mirt_reproject_moments_device(mirt_ctx* c, int width, int height, const mirt_camera* cam,
                                  const mirt_camera* cam_prev, const uint32_t* d_rgba, const float* d_t,
                                  const int32_t* d_sphere, const mirt_history_px* d_hist, const float* d_t_prev,
                                  const int32_t* d_sphere_prev, const mirt_reproject_params* params,
                                  mirt_history_px* d_hist_out, uint32_t* d_out, float* d_out_rgb, void* stream,
                                  const mirt_sphere_motion* motion, const float* d_m2_prev, float* d_m2_out)
{
    const char* fn = "mirt_reproject_moments_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!reproject_args_valid(width, height, cam, cam_prev, d_rgba, d_t, d_sphere, d_hist, d_t_prev, d_sphere_prev,
                              params, d_hist_out) ||
        !reproject_moments_valid(d_hist, motion, cam_prev != nullptr, d_m2_prev, d_m2_out)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return reproject_enqueue(c, width, height, cam, cam_prev, d_rgba, d_t, d_sphere, d_hist, d_t_prev, d_sphere_prev,
                             params, d_hist_out, d_out, d_out_rgb, nullptr, (hipStream_t)stream, motion, d_m2_prev,
                             d_m2_out);
}

}  // extern "C"

namespace {

// the blocking forms: host pointers staged through one allocation (motion: null for mirt_reproject)
int reproject_blocking(mirt_ctx* c, int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                       const mirt_rgba8* rgba, const float* t, const int32_t* sphere, const mirt_history_px* hist,
                       const float* t_prev, const int32_t* sphere_prev, const mirt_reproject_params* params,
                       mirt_history_px* hist_out, mirt_rgba8* out, float* out_rgb, const mirt_sphere_motion* motion,
                       const char* fn, const float* m2_prev = nullptr, float* m2_out = nullptr)   // (m2_out: moments)
{
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!reproject_args_valid(width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    // staging freed on the way out: the records in and out first (16 B each), then the 4-byte planes and the outputs
    const size_t n = (size_t)width * height;
    const size_t b_prev = hist ? n : 0, b_out = out ? 4 * n : 0, b_rgb = out_rgb ? 12 * n : 0;
    DevMem m;
    // (the motion's arrays last: 16-byte elements behind a multiple of 16 bytes, then the 4-byte map)
    const size_t b_img = (16 * n + 16 * b_prev + 12 * n + 8 * b_prev + b_out + b_rgb + 15) & ~(size_t)15;
    const size_t b_geo = motion ? 16 * (size_t)motion->num_spheres : 0, b_gp = motion ? 16 * (size_t)motion->num_prev : 0;
    const size_t b_idx = motion && motion->prev_index ? 4 * (size_t)motion->num_spheres : 0;
    // (the moments' planes behind everything else: 4-byte elements)
    const size_t b_m2p = m2_out ? 4 * b_prev : 0, b_m2o = m2_out ? 4 * n : 0;
    HIP_TRY(hipMalloc(&m.p, b_img + b_geo + b_gp + b_idx + b_m2p + b_m2o));
    char* const d_ho = (char*)m.p;
    char* const d_h = d_ho + 16 * n;
    char* const d_px = d_h + 16 * b_prev;
    char* const d_t = d_px + 4 * n;
    char* const d_s = d_t + 4 * n;
    char* const d_tp = d_s + 4 * n;
    char* const d_sp = d_tp + 4 * b_prev;
    char* const d_o = d_sp + 4 * b_prev;
    char* const d_rgb = d_o + b_out;
    char* const d_geo = d_ho + b_img;
    char* const d_gp = d_geo + b_geo;
    char* const d_idx = d_gp + b_gp;
    char* const d_m2p = d_idx + b_idx;
    char* const d_m2o = d_m2p + b_m2p;
    mirt_sphere_motion d_motion{};
    if (motion) {
        d_motion = mirt_sphere_motion{(const float*)d_geo, (const float*)d_gp, b_idx ? (const int32_t*)d_idx : nullptr,
                                      motion->num_spheres, motion->num_prev};
        HIP_TRY(hipMemcpyAsync(d_geo, motion->geo, b_geo, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_gp, motion->geo_prev, b_gp, hipMemcpyHostToDevice, s));
        if (b_idx) HIP_TRY(hipMemcpyAsync(d_idx, motion->prev_index, b_idx, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(d_px, rgba, 4 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_t, t, 4 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_s, sphere, 4 * n, hipMemcpyHostToDevice, s));
    if (hist) {
        HIP_TRY(hipMemcpyAsync(d_h, hist, 16 * n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_tp, t_prev, 4 * n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_sp, sphere_prev, 4 * n, hipMemcpyHostToDevice, s));
        if (m2_out) HIP_TRY(hipMemcpyAsync(d_m2p, m2_prev, 4 * n, hipMemcpyHostToDevice, s));
    }
    const int rc = reproject_enqueue(c, width, height, cam, cam_prev, (const uint32_t*)d_px, (const float*)d_t,
                                     (const int32_t*)d_s, hist ? (const mirt_history_px*)d_h : nullptr,
                                     hist ? (const float*)d_tp : nullptr, hist ? (const int32_t*)d_sp : nullptr, params,
                                     (mirt_history_px*)d_ho, out ? (uint32_t*)d_o : nullptr,
                                     out_rgb ? (float*)d_rgb : nullptr, nullptr, s, motion ? &d_motion : nullptr,
                                     m2_out && hist ? (const float*)d_m2p : nullptr, m2_out ? (float*)d_m2o : nullptr);
    if (rc) {
        (void)hipStreamSynchronize(s);   // the copies in still read the caller's memory and write the staging
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(hist_out, d_ho, 16 * n, hipMemcpyDeviceToHost, s));
    if (m2_out) HIP_TRY(hipMemcpyAsync(m2_out, d_m2o, 4 * n, hipMemcpyDeviceToHost, s));
    if (out) HIP_TRY(hipMemcpyAsync(out, d_o, b_out, hipMemcpyDeviceToHost, s));
    if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, d_rgb, b_rgb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MIRT_OK;
}

}  // namespace

int mirt::reproject_frame_filter(mirt_ctx* c, const mirt_denoise_var_params* vp, const uint32_t** d_filtered,
                                 hipStream_t s, const char* fn)
{
    const ReprojectState* st = *ctx_reproject_state(c);
    const size_t n = (size_t)st->width * st->height;
    const Parts p = state_parts(st, n);
    const MomentParts mp = moment_parts(st, n);
    *d_filtered = mp.filtered;
    return vfilter_enqueue(c, st->width, st->height, p.rec[st->cur], mp.m2[st->cur], p.sphere[st->cur], mp.normal, vp,
                           mp.filtered, nullptr, nullptr, s, fn);
}

bool mirt::reproject_last_carried(mirt_ctx* c)
{
    const ReprojectState* st = *ctx_reproject_state(c);
    return st && st->valid && st->carried;
}

extern "C" {

int mirt_reproject(mirt_ctx* c, int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                   const mirt_rgba8* rgba, const float* t, const int32_t* sphere, const mirt_history_px* hist,
                   const float* t_prev, const int32_t* sphere_prev, const mirt_reproject_params* params,
                   mirt_history_px* hist_out, mirt_rgba8* out, float* out_rgb)
{
    return reproject_blocking(c, width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out, out, out_rgb, nullptr, "mirt_reproject");
}

int mirt_reproject_motion(mirt_ctx* c, int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                          const mirt_rgba8* rgba, const float* t, const int32_t* sphere, const mirt_history_px* hist,
                          const float* t_prev, const int32_t* sphere_prev, const mirt_reproject_params* params,
                          mirt_history_px* hist_out, mirt_rgba8* out, float* out_rgb, const mirt_sphere_motion* motion)
{
    const char* fn = "mirt_reproject_motion";
    if (c && !mirt::reproject_motion_valid(motion, cam_prev != nullptr)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return reproject_blocking(c, width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out, out, out_rgb, motion, fn);
}

int mirt_reproject_moments(mirt_ctx* c, int width, int height, const mirt_camera* cam, const mirt_camera* cam_prev,
                           const mirt_rgba8* rgba, const float* t, const int32_t* sphere, const mirt_history_px* hist,
                           const float* t_prev, const int32_t* sphere_prev, const mirt_reproject_params* params,
                           mirt_history_px* hist_out, mirt_rgba8* out, float* out_rgb, const mirt_sphere_motion* motion,
                           const float* m2_prev, float* m2_out)
{
    const char* fn = "mirt_reproject_moments";
    if (c && !mirt::reproject_moments_valid(hist, motion, cam_prev != nullptr, m2_prev, m2_out)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return reproject_blocking(c, width, height, cam, cam_prev, rgba, t, sphere, hist, t_prev, sphere_prev, params,
                              hist_out, out, out_rgb, motion, fn, m2_prev, m2_out);
}

int mirt_history_reset(mirt_ctx* c)
{
    if (!c) {
        set_error("mirt_history_reset: null context");
        return MIRT_E_INVALID;
    }
    if (ReprojectState* st = *ctx_reproject_state(c)) {
        st->valid = false;
        st->carry = false;
        st->carried = false;
        st->frames = 0;
    }
    return MIRT_OK;
}

int mirt_history_stats_get(mirt_ctx* c, mirt_history_stats* out)
{
    const char* fn = "mirt_history_stats_get";
    if (!c || !out) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    *out = mirt_history_stats{};
    const ReprojectState* st = *ctx_reproject_state(c);
    if (!st) return MIRT_OK;
    out->bytes = st->cap + st->mcap;
    if (!st->valid) return MIRT_OK;
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    uint32_t counts[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(counts, st->d, sizeof counts, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->frames = st->frames;
    out->scene_id = st->scene_id;
    out->width = st->width;
    out->height = st->height;
    out->sky = counts[kReprojectSky];
    out->fresh = counts[kReprojectFresh];
    out->reused = counts[kReprojectReused];
    return MIRT_OK;
}

int mirt_history_read(mirt_ctx* c, mirt_history_px* hist, size_t n)
{
    const char* fn = "mirt_history_read";
    if (!c || !hist) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    const ReprojectState* st = *ctx_reproject_state(c);
    if (!st || !st->valid || n != (size_t)st->width * st->height) {
        set_error("%s: no history of %zu pixels", fn, n);
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    HIP_TRY(hipMemcpyAsync(hist, state_parts(st, n).rec[st->cur], n * sizeof *hist, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MIRT_OK;
}

int mirt_history_moments_read(mirt_ctx* c, float* m2, size_t n)
{
    const char* fn = "mirt_history_moments_read";
    if (!c || !m2) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    const ReprojectState* st = *ctx_reproject_state(c);
    if (!st || !st->valid || !st->moments || n != (size_t)st->width * st->height) {
        set_error("%s: no history with moments of %zu pixels", fn, n);
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    HIP_TRY(hipMemcpyAsync(m2, moment_parts(st, n).m2[st->cur], n * sizeof *m2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MIRT_OK;
}

}  // extern "C"

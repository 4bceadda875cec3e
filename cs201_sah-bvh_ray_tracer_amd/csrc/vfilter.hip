// mirt_denoise_var_device / mirt_denoise_var: the variance-guided filter of
// csrc/vfilter.h on the device, byte for byte what mirt_denoise_var_host gives.
//
//   ingest   one thread per pixel, 64 x 4 pixels per workgroup with the lanes
//            of a wave along x: the pixel's record, m2, sphere and normal are
//            loaded together; V1 for a record of min_history samples or more,
//            and only the lanes with a shorter history walk V2's 7 x 7 window
//            (49 taps of a 16-byte record and a 4-byte sphere by direct loads,
//            a row's seven issued together; a wave's tap is 1 KiB
//            contiguous). It writes the 16-byte records
//            the passes read, VfColour {r, g, b, var} and VfGuide {normal,
//            sphere}, so that a tap is two dwordx4 loads.
//   pass     one thread per pixel, vfilter_pixel on the records the ingest or
//            the pass before wrote; the colours ping-pong between two images,
//            the guides stay. The last pass stores the caller's outputs. Two
//            forms, as denoise.hip's:
//              direct  every tap from global memory, 64 x 4 pixels per
//                      workgroup;
//              tile    spacings 1 and 2 only: the workgroup's 32 x 8 pixels
//                      and their halo of 2 s first go to LDS.
//            MIRT_OPT_DENOISE_TILE picks; either gives the same bytes.
// Tap positions are computed from the pixel's coordinates alone and checked
// against the image before the load (a tap outside reads the pixel itself),
// and the tile's records outside the image are never read: whatever the data
// holds, no access leaves the image, the scratch or the tile. Every loop is
// bounded at compile time or at launch; no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "device_util.h"
#include "internal.h"
#include "vfilter.h"

#pragma clang fp contract(off)

namespace mirt {

// The records of the largest image filtered so far: two colour images and the
// guides, in one allocation that only ever grows.
struct VfilterState {
    void* d = nullptr;
    size_t cap = 0;
};

void vfilter_state_free(VfilterState* st)
{
    if (!st) return;
    if (st->d) (void)hipFree(st->d);
    delete st;
}

}  // namespace mirt

namespace {

using namespace mirt;

constexpr int kBlock = 256;
constexpr int kDirectW = 64, kDirectH = 4;   // ingest and the direct pass: a wave per row of 64 pixels
constexpr int kTileW = 32, kTileH = 8;       // the tile pass

struct Image {
    int width, height;
    int tiles_x;   // workgroup b covers tile (b % tiles_x, b / tiles_x)
};

struct IngestArgs {
    Image im;
    const mirt_history_px* hist;
    const float* m2;
    const int32_t* sphere;
    const float* normal;   // null: no normal plane
    int min_history;
    VfColour* colour;
    VfGuide* guide;
    float* var_out;        // may be null
};

struct PassArgs {
    Image im;
    const VfColour* src;
    const VfGuide* guide;
    int spacing, sharpness;
    float sl2;
    VfColour* dst;     // every pass but the last
    uint32_t* out;     // the last pass: either may be null
    float* out_rgb;
};

struct PlanesAt {
    const mirt_history_px* h;
    const int32_t* s;
    int width;
    __device__ mirt_history_px hist(int x, int y) const { return h[(size_t)y * width + x]; }
    __device__ int32_t sphere(int x, int y) const { return s[(size_t)y * width + x]; }
};

__global__ void __launch_bounds__(kBlock) vfilter_ingest_kernel(const IngestArgs a)
{
    const int bx = (int)(blockIdx.x % (unsigned)a.im.tiles_x), by = (int)(blockIdx.x / (unsigned)a.im.tiles_x);
    const int x = bx * kDirectW + (int)(threadIdx.x % kDirectW), y = by * kDirectH + (int)(threadIdx.x / kDirectW);
    if (x >= a.im.width || y >= a.im.height) return;
    const size_t i = (size_t)y * a.im.width + x;
    const mirt_history_px hp = a.hist[i];
    const float m2p = a.m2[i];
    const int32_t sp = a.sphere[i];
    VfGuide g{0.0f, 0.0f, 0.0f, sp};
    if (a.normal) {   // (uniform)
        g.nx = a.normal[3 * i];
        g.ny = a.normal[3 * i + 1];
        g.nz = a.normal[3 * i + 2];
    }
    const PlanesAt at{a.hist, a.sphere, a.im.width};
    const float var = vfilter_variance(at, a.im.width, a.im.height, x, y, hp, m2p, sp, a.min_history);
    a.colour[i] = VfColour{hp.r, hp.g, hp.b, var};
    a.guide[i] = g;
    if (a.var_out) a.var_out[i] = var;
}

__device__ __forceinline__ void store_pixel(const PassArgs& a, int x, int y, const VfColour& c)
{
    const size_t i = (size_t)y * a.im.width + x;
    if (a.dst) {
        a.dst[i] = c;
        return;
    }
    if (a.out_rgb) {
        a.out_rgb[3 * i] = c.r;
        a.out_rgb[3 * i + 1] = c.g;
        a.out_rgb[3 * i + 2] = c.b;
    }
    if (a.out) a.out[i] = vfilter_display(c);
}

struct GlobalAt {
    const VfColour* c;
    const VfGuide* g;
    int width;
    __device__ VfColour colour(int x, int y) const { return c[(size_t)y * width + x]; }
    __device__ VfGuide guide(int x, int y) const { return g[(size_t)y * width + x]; }
};

// (NORMAL: with a normal plane. A template parameter, as denoise.hip's.)
template <bool NORMAL>
__global__ void __launch_bounds__(kBlock) vfilter_pass_kernel(const PassArgs a)
{
    const int bx = (int)(blockIdx.x % (unsigned)a.im.tiles_x), by = (int)(blockIdx.x / (unsigned)a.im.tiles_x);
    const int x = bx * kDirectW + (int)(threadIdx.x % kDirectW), y = by * kDirectH + (int)(threadIdx.x / kDirectW);
    if (x >= a.im.width || y >= a.im.height) return;
    const GlobalAt at{a.src, a.guide, a.im.width};
    store_pixel(a, x, y, vfilter_pixel(at, a.im.width, a.im.height, x, y, a.spacing, NORMAL, a.sharpness, a.sl2));
}

// The tile of spacing S: (kTileW + 4 S) x (kTileH + 4 S) records, record
// (lx, ly) being pixel (x0 - 2 S + lx, y0 - 2 S + ly).
template <int S>
struct TileAt {
    static constexpr int kW = kTileW + 4 * S, kH = kTileH + 4 * S;
    const VfColour* c;
    const VfGuide* g;
    int x0, y0;   // the pixel of record (0, 0)
    __device__ VfColour colour(int x, int y) const { return c[(y - y0) * kW + (x - x0)]; }
    __device__ VfGuide guide(int x, int y) const { return g[(y - y0) * kW + (x - x0)]; }
};

template <int S, bool NORMAL>
__global__ void __launch_bounds__(kBlock) vfilter_tile_pass_kernel(const PassArgs a)
{
    using T = TileAt<S>;
    __shared__ VfColour sc[T::kW * T::kH];
    __shared__ VfGuide sg[T::kW * T::kH];
    const int bx = (int)(blockIdx.x % (unsigned)a.im.tiles_x), by = (int)(blockIdx.x / (unsigned)a.im.tiles_x);
    // (x0, y0 may be negative; the image's extent plus the halo stays far inside int: a tile starts inside the image)
    const int x0 = bx * kTileW - 2 * S, y0 = by * kTileH - 2 * S;
    for (int r = (int)threadIdx.x; r < T::kW * T::kH; r += kBlock) {
        const int lx = r % T::kW, ly = r / T::kW;
        // (unsigned: a record left of or above the image, or past INT_MAX, is outside)
        const uint32_t gx = (uint32_t)x0 + (uint32_t)lx, gy = (uint32_t)y0 + (uint32_t)ly;
        if (gx < (uint32_t)a.im.width && gy < (uint32_t)a.im.height) {
            const size_t i = (size_t)gy * a.im.width + gx;
            sc[r] = a.src[i];
            sg[r] = a.guide[i];
        }
    }
    __syncthreads();
    const int x = bx * kTileW + (int)(threadIdx.x % kTileW), y = by * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= a.im.width || y >= a.im.height) return;
    const T at{sc, sg, x0, y0};
    store_pixel(a, x, y, vfilter_pixel(at, a.im.width, a.im.height, x, y, S, NORMAL, a.sharpness, a.sl2));
}

unsigned tile_count(int width, int height, int tw, int th, int* tiles_x)
{
    // (width * height <= 2^31, so the count fits an unsigned and a grid's x)
    const uint64_t tx = ((uint64_t)width + tw - 1) / tw, ty = ((uint64_t)height + th - 1) / th;
    *tiles_x = (int)tx;
    return (unsigned)(tx * ty);
}

}  // namespace

// the filter of VALID arguments, all in device memory, enqueued on `s`
int mirt::vfilter_enqueue(mirt_ctx* c, int width, int height, const mirt_history_px* d_hist, const float* d_m2,
                    const int32_t* d_sphere, const float* d_normal, const mirt_denoise_var_params* p, uint32_t* d_out,
                    float* d_out_rgb, float* d_var_out, hipStream_t s, const char* fn)
{
    HIP_TRY(hipSetDevice(ctx_device(c)));
    VfilterState** slot = ctx_vfilter_state(c);
    if (!*slot) *slot = new (std::nothrow) VfilterState();
    VfilterState* st = *slot;
    if (!st) {
        set_error("%s: out of host memory", fn);
        return MIRT_E_NOMEM;
    }
    static_assert(sizeof(VfColour) == 16 && sizeof(VfGuide) == 16, "16-byte records");
    const size_t n = (size_t)width * height;
    const size_t images = (p->passes > 1 ? 2 : 1) + 1;
    const size_t bytes = images * n * sizeof(VfColour);
    const bool grow = bytes > st->cap;
    if (int rc = ctx_launch_begin(c, s, grow)) return rc;
    if (grow) {
        if (st->d) (void)hipFree(st->d);
        st->d = nullptr;
        st->cap = 0;
        HIP_TRY(hipMalloc(&st->d, bytes));
        st->cap = bytes;
    }
    VfColour* img[2] = {(VfColour*)st->d, (VfColour*)st->d + (p->passes > 1 ? n : 0)};
    VfGuide* guide = (VfGuide*)st->d + (images - 1) * n;

    IngestArgs in{};
    in.im.width = width;
    in.im.height = height;
    in.hist = d_hist;
    in.m2 = d_m2;
    in.sphere = d_sphere;
    in.normal = d_normal;
    in.min_history = p->min_history;
    in.colour = img[0];
    in.guide = guide;
    in.var_out = d_var_out;
    const unsigned gi = tile_count(width, height, kDirectW, kDirectH, &in.im.tiles_x);
    vfilter_ingest_kernel<<<gi, kBlock, 0, s>>>(in);
    HIP_TRY(hipGetLastError());
    const int tile = ctx_denoise_tile(c);
    const bool nrm = d_normal != nullptr;
    for (int pass = 0; pass < p->passes; pass++) {
        const bool last = pass == p->passes - 1;
        PassArgs a{};
        a.im.width = width;
        a.im.height = height;
        a.src = img[pass & 1];
        a.guide = guide;
        a.spacing = 1 << pass;
        a.sharpness = p->normal_sharpness;
        a.sl2 = vfilter_sl2(p->sigma_lum);
        a.dst = last ? nullptr : img[(pass + 1) & 1];
        a.out = last ? d_out : nullptr;
        a.out_rgb = last ? d_out_rgb : nullptr;
        if (tile && pass < 2) {
            const unsigned g = tile_count(width, height, kTileW, kTileH, &a.im.tiles_x);
            if (pass == 0 && nrm)
                vfilter_tile_pass_kernel<1, true><<<g, kBlock, 0, s>>>(a);
            else if (pass == 0)
                vfilter_tile_pass_kernel<1, false><<<g, kBlock, 0, s>>>(a);
            else if (nrm)
                vfilter_tile_pass_kernel<2, true><<<g, kBlock, 0, s>>>(a);
            else
                vfilter_tile_pass_kernel<2, false><<<g, kBlock, 0, s>>>(a);
        } else {
            const unsigned g = tile_count(width, height, kDirectW, kDirectH, &a.im.tiles_x);
            if (nrm)
                vfilter_pass_kernel<true><<<g, kBlock, 0, s>>>(a);
            else
                vfilter_pass_kernel<false><<<g, kBlock, 0, s>>>(a);
        }
        HIP_TRY(hipGetLastError());
    }
    return ctx_launch_end(c, s);
}

extern "C" {

int mirt_denoise_var_device(mirt_ctx* c, int width, int height, const mirt_history_px* d_hist, const float* d_m2,
                            const int32_t* d_sphere, const float* d_normal, const mirt_denoise_var_params* params,
                            uint32_t* d_out, float* d_out_rgb, float* d_var_out, void* stream)
{
    const char* fn = "mirt_denoise_var_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!vfilter_args_valid(width, height, d_hist, d_m2, d_sphere, params, d_out, d_out_rgb)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return vfilter_enqueue(c, width, height, d_hist, d_m2, d_sphere, d_normal, params, d_out, d_out_rgb, d_var_out,
                           (hipStream_t)stream, fn);
}

int mirt_denoise_var(mirt_ctx* c, int width, int height, const mirt_history_px* hist, const float* m2,
                     const int32_t* sphere, const float* normal, const mirt_denoise_var_params* params, mirt_rgba8* out,
                     float* out_rgb, float* var_out)
{
    const char* fn = "mirt_denoise_var";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!vfilter_args_valid(width, height, hist, m2, sphere, params, out, out_rgb)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    // staging freed on the way out: the records first (16 B each), then the 4-byte planes and the outputs
    const size_t n = (size_t)width * height;
    const size_t b_nrm = normal ? 12 * n : 0, b_out = out ? 4 * n : 0, b_rgb = out_rgb ? 12 * n : 0,
                 b_var = var_out ? 4 * n : 0;
    DevMem m;
    HIP_TRY(hipMalloc(&m.p, 16 * n + 4 * n + 4 * n + b_nrm + b_out + b_rgb + b_var));
    char* const d_h = (char*)m.p;
    char* const d_m2 = d_h + 16 * n;
    char* const d_sph = d_m2 + 4 * n;
    char* const d_nrm = d_sph + 4 * n;
    char* const d_o = d_nrm + b_nrm;
    char* const d_rgb = d_o + b_out;
    char* const d_var = d_rgb + b_rgb;
    HIP_TRY(hipMemcpyAsync(d_h, hist, 16 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_m2, m2, 4 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_sph, sphere, 4 * n, hipMemcpyHostToDevice, s));
    if (normal) HIP_TRY(hipMemcpyAsync(d_nrm, normal, b_nrm, hipMemcpyHostToDevice, s));
    const int rc = vfilter_enqueue(c, width, height, (const mirt_history_px*)d_h, (const float*)d_m2,
                                   (const int32_t*)d_sph, normal ? (const float*)d_nrm : nullptr, params,
                                   out ? (uint32_t*)d_o : nullptr, out_rgb ? (float*)d_rgb : nullptr,
                                   var_out ? (float*)d_var : nullptr, s, fn);
    if (rc) {
        (void)hipStreamSynchronize(s);   // the copies in still read the caller's memory and write the staging
        return rc;
    }
    if (out) HIP_TRY(hipMemcpyAsync(out, d_o, b_out, hipMemcpyDeviceToHost, s));
    if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, d_rgb, b_rgb, hipMemcpyDeviceToHost, s));
    if (var_out) HIP_TRY(hipMemcpyAsync(var_out, d_var, b_var, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MIRT_OK;
}

}  // extern "C"

// mirt_denoise_device / mirt_denoise: the filter of csrc/denoise.h on the
// device, byte for byte what mirt_denoise_host gives.
//
//   ingest   one thread per pixel packs the source colour with the sphere
//            index, and the normal, into 16-byte records (DenoiseColour,
//            DenoiseNormal), so that a tap is two dwordx4 loads with the lanes
//            of a wave along x.
//   pass     one thread per pixel, denoise_pixel on the records the ingest or
//            the pass before wrote; the records ping-pong between two images.
//            The last pass stores the caller's outputs instead. Two forms:
//              direct  every tap loaded from global memory: 64 x 4 pixels per
//                      workgroup, a wave's tap is 1 KiB contiguous;
//              tile    spacings 1 and 2 only: the workgroup's 32 x 8 pixels
//                      and their halo of 2 s first go to LDS, the taps are
//                      ds_read_b128.
//            MIRT_OPT_DENOISE_TILE picks (MEASUREMENTS.md E has both).
// Tap positions are computed from the pixel's coordinates alone and checked
// against the image before the load (a tap outside reads the pixel itself),
// and the tile's records outside the image are never read: whatever the data
// holds, no access leaves the image, the scratch or the tile. Every loop is
// bounded at launch; no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "denoise.h"
#include "device_util.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace mirt {

// The records of the largest image filtered so far: two colour images and the
// normals, in one allocation that only ever grows.
struct DenoiseState {
    void* d = nullptr;
    size_t cap = 0;
};

void denoise_state_free(DenoiseState* st)
{
    if (!st) return;
    if (st->d) (void)hipFree(st->d);
    delete st;
}

}  // namespace mirt

namespace {

using namespace mirt;

constexpr int kBlock = 256;
constexpr int kDirectW = 64, kDirectH = 4;   // the direct pass: a wave per row of 64 pixels
constexpr int kTileW = 32, kTileH = 8;       // the tile pass

struct Image {
    int width, height;
    int tiles_x;   // workgroup b covers tile (b % tiles_x, b / tiles_x)
};

struct PassArgs {
    Image im;
    const DenoiseColour* src;
    const DenoiseNormal* normal;   // null: no normal plane
    int spacing, sharpness;
    float inv;
    DenoiseColour* dst;            // every pass but the last
    uint32_t* out;                 // the last pass: either may be null
    float* out_rgb;
};

__global__ void __launch_bounds__(kBlock)
denoise_ingest_kernel(size_t n, const uint32_t* __restrict__ rgba, const float* __restrict__ accum, int frames,
                      const int32_t* __restrict__ sphere, const float* __restrict__ normal,
                      DenoiseColour* __restrict__ colour, DenoiseNormal* __restrict__ nrm)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t s = sphere[i];
    colour[i] = rgba ? denoise_source_rgba(rgba[i], s) : denoise_source_accum(accum + 3 * i, frames, s);
    if (normal) nrm[i] = DenoiseNormal{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], 0.0f};
}

__device__ __forceinline__ void store_pixel(const PassArgs& a, int x, int y, const DenoiseColour& c)
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
    if (a.out) a.out[i] = denoise_display(c);
}

// (NORMAL: with a normal plane. A template parameter, so that a tap's loads
// stand in straight-line code and a row's are issued together.)
template <bool NORMAL>
struct GlobalAt {
    const DenoiseColour* c;
    const DenoiseNormal* n;
    int width;
    __device__ DenoiseColour colour(int x, int y) const { return c[(size_t)y * width + x]; }
    __device__ DenoiseNormal normal(int x, int y) const
    {
        return NORMAL ? n[(size_t)y * width + x] : DenoiseNormal{};
    }
};

template <bool NORMAL>
__global__ void __launch_bounds__(kBlock) denoise_pass_kernel(const PassArgs a)
{
    const int bx = (int)(blockIdx.x % (unsigned)a.im.tiles_x), by = (int)(blockIdx.x / (unsigned)a.im.tiles_x);
    const int x = bx * kDirectW + (int)(threadIdx.x % kDirectW), y = by * kDirectH + (int)(threadIdx.x / kDirectW);
    if (x >= a.im.width || y >= a.im.height) return;
    const GlobalAt<NORMAL> at{a.src, a.normal, a.im.width};
    store_pixel(a, x, y, denoise_pixel(at, a.im.width, a.im.height, x, y, a.spacing, NORMAL, a.sharpness, a.inv));
}

// The tile of spacing S: (kTileW + 4 S) x (kTileH + 4 S) records, record
// (lx, ly) being pixel (x0 - 2 S + lx, y0 - 2 S + ly).
template <int S, bool NORMAL>
struct TileAt {
    static constexpr int kW = kTileW + 4 * S, kH = kTileH + 4 * S;
    const DenoiseColour* c;
    const DenoiseNormal* n;
    int x0, y0;   // the pixel of record (0, 0)
    __device__ DenoiseColour colour(int x, int y) const { return c[(y - y0) * kW + (x - x0)]; }
    __device__ DenoiseNormal normal(int x, int y) const
    {
        return NORMAL ? n[(y - y0) * kW + (x - x0)] : DenoiseNormal{};
    }
};

template <int S, bool NORMAL>
__global__ void __launch_bounds__(kBlock) denoise_tile_pass_kernel(const PassArgs a)
{
    using T = TileAt<S, NORMAL>;
    __shared__ DenoiseColour sc[T::kW * T::kH];
    __shared__ DenoiseNormal sn[NORMAL ? T::kW * T::kH : 1];
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
            if (NORMAL) sn[r] = a.normal[i];
        }
    }
    __syncthreads();
    const int x = bx * kTileW + (int)(threadIdx.x % kTileW), y = by * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= a.im.width || y >= a.im.height) return;
    const T at{sc, sn, x0, y0};
    store_pixel(a, x, y, denoise_pixel(at, a.im.width, a.im.height, x, y, S, NORMAL, a.sharpness, a.inv));
}

unsigned tile_count(int width, int height, int tw, int th, int* tiles_x)
{
    // (width * height <= 2^31, so the count fits an unsigned and a grid's x)
    const uint64_t tx = ((uint64_t)width + tw - 1) / tw, ty = ((uint64_t)height + th - 1) / th;
    *tiles_x = (int)tx;
    return (unsigned)(tx * ty);
}

}  // namespace

int mirt::denoise_enqueue(mirt_ctx* c, int width, int height, const uint32_t* d_rgba, const float* d_accum,
                          int frames, const int32_t* d_sphere, const float* d_normal,
                          const mirt_denoise_params* p, uint32_t* d_out, float* d_out_rgb, hipStream_t s,
                          const char* fn)
{
    HIP_TRY(hipSetDevice(ctx_device(c)));
    DenoiseState** slot = ctx_denoise_state(c);
    if (!*slot) *slot = new (std::nothrow) DenoiseState();
    DenoiseState* st = *slot;
    if (!st) {
        set_error("%s: out of host memory", fn);
        return MIRT_E_NOMEM;
    }
    const size_t n = (size_t)width * height;
    const size_t images = (p->passes > 1 ? 2 : 1) + (d_normal ? 1 : 0);
    const size_t bytes = images * n * sizeof(DenoiseColour);
    const bool grow = bytes > st->cap;
    if (int rc = ctx_launch_begin(c, s, grow)) return rc;
    if (grow) {
        if (st->d) (void)hipFree(st->d);
        st->d = nullptr;
        st->cap = 0;
        HIP_TRY(hipMalloc(&st->d, bytes));
        st->cap = bytes;
    }
    DenoiseColour* img[2] = {(DenoiseColour*)st->d, (DenoiseColour*)st->d + (p->passes > 1 ? n : 0)};
    DenoiseNormal* nrm = d_normal ? (DenoiseNormal*)st->d + (images - 1) * n : nullptr;
    static_assert(sizeof(DenoiseColour) == 16 && sizeof(DenoiseNormal) == 16, "16-byte records");

    denoise_ingest_kernel<<<blocks(n, kBlock), kBlock, 0, s>>>(n, d_rgba, d_accum, frames, d_sphere, d_normal, img[0],
                                                                nrm);
    HIP_TRY(hipGetLastError());
    const int tile = ctx_denoise_tile(c);
    for (int pass = 0; pass < p->passes; pass++) {
        const bool last = pass == p->passes - 1;
        PassArgs a{};
        a.im.width = width;
        a.im.height = height;
        a.src = img[pass & 1];
        a.normal = nrm;
        a.spacing = 1 << pass;
        a.sharpness = p->normal_sharpness;
        a.inv = denoise_inv(p->sigma_colour, pass);
        a.dst = last ? nullptr : img[(pass + 1) & 1];
        a.out = last ? d_out : nullptr;
        a.out_rgb = last ? d_out_rgb : nullptr;
        if (tile && pass < 2) {
            const unsigned g = tile_count(width, height, kTileW, kTileH, &a.im.tiles_x);
            if (pass == 0 && nrm)
                denoise_tile_pass_kernel<1, true><<<g, kBlock, 0, s>>>(a);
            else if (pass == 0)
                denoise_tile_pass_kernel<1, false><<<g, kBlock, 0, s>>>(a);
            else if (nrm)
                denoise_tile_pass_kernel<2, true><<<g, kBlock, 0, s>>>(a);
            else
                denoise_tile_pass_kernel<2, false><<<g, kBlock, 0, s>>>(a);
        } else {
            const unsigned g = tile_count(width, height, kDirectW, kDirectH, &a.im.tiles_x);
            if (nrm)
                denoise_pass_kernel<true><<<g, kBlock, 0, s>>>(a);
            else
                denoise_pass_kernel<false><<<g, kBlock, 0, s>>>(a);
        }
        HIP_TRY(hipGetLastError());
    }
    return ctx_launch_end(c, s);
}

extern "C" {

int mirt_denoise_device(mirt_ctx* c, int width, int height, const uint32_t* d_rgba, const float* d_accum, int frames,
                        const int32_t* d_sphere, const float* d_normal, const mirt_denoise_params* params,
                        uint32_t* d_out, float* d_out_rgb, void* stream)
{
    const char* fn = "mirt_denoise_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!denoise_args_valid(width, height, d_rgba, d_accum, frames, d_sphere, params, d_out, d_out_rgb)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    return denoise_enqueue(c, width, height, d_rgba, d_accum, frames, d_sphere, d_normal, params, d_out, d_out_rgb,
                           (hipStream_t)stream, fn);
}

int mirt_denoise(mirt_ctx* c, int width, int height, const mirt_rgba8* rgba, const float* accum, int frames,
                 const int32_t* sphere, const float* normal, const mirt_denoise_params* params, mirt_rgba8* out,
                 float* out_rgb)
{
    const char* fn = "mirt_denoise";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!denoise_args_valid(width, height, rgba, accum, frames, sphere, params, out, out_rgb)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    // staging freed on the way out: source, sphere, normal, then the two outputs
    const size_t n = (size_t)width * height;
    const size_t b_src = rgba ? 4 * n : 12 * n, b_nrm = normal ? 12 * n : 0, b_out = out ? 4 * n : 0,
                 b_rgb = out_rgb ? 12 * n : 0;
    DevMem m;
    HIP_TRY(hipMalloc(&m.p, b_src + 4 * n + b_nrm + b_out + b_rgb));
    char* const d_src = (char*)m.p;
    char* const d_sph = d_src + b_src;
    char* const d_nrm = d_sph + 4 * n;
    char* const d_o = d_nrm + b_nrm;
    char* const d_rgb = d_o + b_out;
    HIP_TRY(hipMemcpyAsync(d_src, rgba ? (const void*)rgba : (const void*)accum, b_src, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_sph, sphere, 4 * n, hipMemcpyHostToDevice, s));
    if (normal) HIP_TRY(hipMemcpyAsync(d_nrm, normal, b_nrm, hipMemcpyHostToDevice, s));
    const int rc = denoise_enqueue(c, width, height, rgba ? (const uint32_t*)d_src : nullptr,
                                   rgba ? nullptr : (const float*)d_src, frames, (const int32_t*)d_sph,
                                   normal ? (const float*)d_nrm : nullptr, params, out ? (uint32_t*)d_o : nullptr,
                                   out_rgb ? (float*)d_rgb : nullptr, s, fn);
    if (rc) {
        (void)hipStreamSynchronize(s);   // the copies in still read the caller's memory and write the staging
        return rc;
    }
    if (out) HIP_TRY(hipMemcpyAsync(out, d_o, b_out, hipMemcpyDeviceToHost, s));
    if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, d_rgb, b_rgb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MIRT_OK;
}

}  // extern "C"

// HIP kernels and the device half of the C ABI (include/mirt.h).
//
// Frame kernel: one wave64 per 8x8 pixel tile (coherent primary rays share
// their BVH walk), 4 waves per 256-thread workgroup. Each lane traces one
// pixel through trace_path (trace.h); the wave walks the skip-threaded tree
// with a wave-uniform cursor, so node and sphere reads are scalar loads of
// an L2-resident array. Output is packed RGBA8 (one dword per pixel).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <map>
#include <mutex>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "coop.h"
#include "denoise.h"
#include "internal.h"
#include "lens.h"
#include "pscan.h"
#include "reproject.h"
#include "shard.h"
#include "trace.h"

using namespace mirt;

namespace {

// Per-frame constants computed on the host with the reference's expressions
// (ray.c:18-24, main.c:356) -- libm tan stays on the host.
struct FrameConst {
    float px, py, pz;  // camera position (ray origin)
    float fx, fy, fz;  // forward
    float hx, hy, hz;  // horizontal = right * (2 half_width)
    float vx, vy, vz;  // vertical = up * (2 half_height)
    float aspect, wf, hf;
    int width, height, depth, use_bvh;
    uint64_t seed;
    uint32_t sample;
    int accumulate;
    float frames;
    int row_block, shard, num_shards, lead_skip;
    int jitter;        // sub-pixel jitter of camera rays from the RNG contract (camera_ray)
    int num_rows;      // rows of this launch: shard_rows x samples (frame j's rows follow frame j-1's)
    int shard_rows;    // rows of one frame of this shard
    int samples;       // frames in this launch (RNG samples sample .. sample + samples - 1)
    RowMagic magic;    // width, shard_rows and row_block as multiply-high divisors (coop.h)
};

FrameConst make_frame_const(const mirt_camera* cam, const mirt_frame_desc* fd)
{
    FrameConst f{};
    const float aspect = (float)fd->width / (float)fd->height;                    // ray.c:18
    const float fov_rad = (float)((double)cam->fov * (M_PI / 180.0));             // ray.c:19
    const float half_h = (float)std::tan((double)(fov_rad / 2.0f));               // ray.c:20
    const float half_w = aspect * half_h;                                         // ray.c:21
    const float sw = 2.0f * half_w, sh = 2.0f * half_h;
    f.px = cam->position.x; f.py = cam->position.y; f.pz = cam->position.z;
    f.fx = cam->forward.x; f.fy = cam->forward.y; f.fz = cam->forward.z;
    f.hx = cam->right.x * sw; f.hy = cam->right.y * sw; f.hz = cam->right.z * sw;  // ray.c:23
    f.vx = cam->up.x * sh; f.vy = cam->up.y * sh; f.vz = cam->up.z * sh;          // ray.c:24
    f.aspect = aspect;                                                            // main.c:356
    f.wf = (float)fd->width;
    f.hf = (float)fd->height;
    f.width = fd->width;
    f.height = fd->height;
    f.depth = fd->max_depth;
    f.use_bvh = fd->use_bvh;
    f.seed = fd->seed;
    f.sample = fd->sample;
    f.accumulate = fd->accumulate;
    f.frames = (float)fd->frames;
    f.row_block = fd->row_block;
    f.shard = fd->shard;
    f.num_shards = fd->num_shards;
    f.lead_skip = fd->lead_skip;
    f.shard_rows = shard_row_count(fd);
    f.samples = fd->samples > 1 ? fd->samples : 1;
    f.jitter = fd->jitter != 0;
    f.num_rows = f.shard_rows * f.samples;
    f.magic = row_magic_make(f.width, f.shard_rows, f.row_block);
    return f;
}

// Image row of launch row r (compacted shard row r % shard_rows of frame r / shard_rows).
__device__ __forceinline__ int shard_row_to_y(const FrameConst& f, int r)
{
    return magic_row_to_y(f.magic, r, f.samples, f.shard_rows, f.row_block, f.shard, f.num_shards, f.lead_skip);
}

// RNG contract sample of launch row r (one sample per frame).
__device__ __forceinline__ uint32_t row_sample(const FrameConst& f, int r)
{
    return f.samples > 1 ? f.sample + magic_div((uint32_t)r, (uint32_t)f.shard_rows, f.magic.shard_rows) : f.sample;
}

// main.c:362-365 + ray.c:26-31 for pixel (x, y) of RNG sample `sample`.
// Jittered frames (mirt_frame_desc.jitter; BASELINE configs[4] "4 spp
// jittered" -- the reference has no jitter, so the build defines it): the
// sample point moves by (jx, jy) in [0, 1)^2, two draws of the pixel's RNG
// contract stream at indices its bounce sampling never reaches (rng.h).
__device__ __forceinline__ Ray camera_ray(const FrameConst& f, int x, int y, uint32_t sample)
{
    float xf = (float)x, yf = (float)y;
    if (f.jitter) {
        const uint64_t key = pixel_key(f.seed, (uint32_t)(y * f.width + x), sample);
        xf = xf + (float)draw(key, kJitterDrawX) / 2147483648.0f;
        yf = yf + (float)draw(key, kJitterDrawY) / 2147483648.0f;
    }
    const float u = (xf / f.wf - 0.5f) * f.aspect;
    const float v = -(yf / f.hf - 0.5f);
    float dx = f.fx + f.hx * u, dy = f.fy + f.hy * u, dz = f.fz + f.hz * u;
    dx = dx + f.vx * v;
    dy = dy + f.vy * v;
    dz = dz + f.vz * v;
    normalize3(dx, dy, dz);
    return {f.px, f.py, f.pz, dx, dy, dz};
}

__device__ __forceinline__ void add_counts(mirt_counts* out, const Counters& c)
{
    atomicAdd((unsigned long long*)&out->rays, (unsigned long long)c.rays);
    atomicAdd((unsigned long long*)&out->nodes, (unsigned long long)c.nodes);
    atomicAdd((unsigned long long*)&out->spheres, (unsigned long long)c.spheres);
    atomicAdd((unsigned long long*)&out->hits, (unsigned long long)c.hits);
    atomicAdd((unsigned long long*)&out->lane_steps, (unsigned long long)c.steps);
    atomicAdd((unsigned long long*)&out->nodes_primary, (unsigned long long)c.nodes0);
    atomicAdd((unsigned long long*)&out->spheres_primary, (unsigned long long)c.spheres0);
    atomicAdd((unsigned long long*)&out->hits_primary, (unsigned long long)c.hits0);
}

// Pixels whose camera ray has a zero or tiny direction component (the image
// centre row / column under an axis-aligned camera) ignore a slab
// (hit.c:54-57) and walk a large part of the tree. A pre-pass lists them
// (mark_deferred_kernel); the first `blocks` workgroups of the frame kernel
// trace them one pixel per wave (the node-parallel walk of trace.h) while
// the other workgroups trace the 8x8 tiles and skip them, so the long walks
// start first and overlap the bulk instead of trailing it.
struct Deferred {
    const uint32_t* list;   // r * width + x
    const uint32_t* count;
    int blocks;
};

// One pixel of the pixel loop: main.c:362-366 ray, trace_ray, then the
// display/accumulation of main.c:368-372 (fresh) or main.c:394-405.
// PLANES = Planes (a frame with planes, else no such argument): the camera
// ray's closest hit also goes to the pixel's element of `planes`.
template <bool FAST, bool COUNT, class... PLANES>
__device__ __forceinline__ void render_pixel(const DevScene& sc, const FrameConst& f, int x, int r, bool alive,
                                             bool skip_generic, uint32_t* __restrict__ out, float* __restrict__ acc,
                                             Counters& cnt, uint32_t* cstack, int cstride,
                                             uint32_t* wstk = nullptr, PLANES... planes)
{
    const int y = alive ? shard_row_to_y(f, r) : 0;
    const Ray ray = camera_ray(f, alive ? x : 0, y, row_sample(f, r));
    if (skip_generic && alive && slab_ray(ray).generic) alive = false;  // a deferred wave traces it
    const uint64_t key = pixel_key(f.seed, (uint32_t)(y * f.width + x), row_sample(f, r));
    const uint32_t c = trace_path<FAST, COUNT>(sc, ray, alive, f.depth, f.use_bvh != 0, key, cnt, cstack,
                                                     cstride, wstk, PlaneSlot{planes, (size_t)r * f.width + x}...);
    if (!alive) return;
    const size_t i = (size_t)r * f.width + x;
    uint32_t shown = c;
    if (acc) {
        float* a = acc + 3 * i;
        for (int ch = 0; ch < 3; ch++) {
            const float v = (float)((c >> (8 * ch)) & 0xff) / 255.0f;  // main.c:368-370 / 394-396
            if (f.accumulate) {
                a[ch] = a[ch] + v;
                const float avg = a[ch] / f.frames * 255.0f;           // main.c:398-400
                const uint32_t q = (uint32_t)(int)fminf(avg, 255.0f);
                shown = (shown & ~(0xffu << (8 * ch))) | ((q & 0xffu) << (8 * ch));
            } else {
                a[ch] = v;
            }
        }
    }
    out[i] = shown;
}

// The pixel loop of main.c:358-374 (fresh) / main.c:382-407 (accumulate).
// PLANES: no argument at all, or the Planes of a frame with planes
// (mirt_render_frame_planes) -- an instantiation of its own, so that the
// kernel of a frame without planes keeps its arguments and its code. With
// planes each pixel's lane -- the deferred wave's lane 0 for a deferred pixel
// -- also stores the hit trace_path finds at level 0.
template <bool FAST, bool COUNT, class... PLANES>
__global__ __launch_bounds__(512) void render_kernel(DevScene sc, FrameConst f, uint32_t* __restrict__ out,
                                                      float* __restrict__ acc, mirt_counts* counts,
                                                      uint32_t* wave_stats, Deferred dfr, PLANES... planes)
{
    uint64_t t0 = 0;
    if (COUNT) t0 = __builtin_amdgcn_s_memrealtime();
    __shared__ uint32_t cstack[kMaxDepth * 512];
    // the four-wide walk's stack (stride kWideStride: workgroups of up to 256)
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    uint32_t* wstk = blockDim.x <= kWideStride ? wstack + threadIdx.x : nullptr;
    Counters cnt{0, 0, 0, 0, 0};
    const int bw = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < dfr.blocks) {
        const uint32_t n = __builtin_amdgcn_readfirstlane(*dfr.count);
        const uint32_t stride = (uint32_t)(dfr.blocks * bw);
        for (uint32_t j = blockIdx.x * bw + wave; j < n; j += stride) {
            const uint32_t p = __builtin_amdgcn_readfirstlane(dfr.list[j]);
            render_pixel<FAST, COUNT>(sc, f, (int)(p % f.width), (int)(p / f.width), (threadIdx.x & 63) == 0,
                                            false, out, acc, cnt, cstack + threadIdx.x, blockDim.x, wstk, planes...);
        }
        if (COUNT) add_counts(counts, cnt);
        return;
    }
    const int tile = (blockIdx.x - dfr.blocks) * bw + wave;
    const int lane = threadIdx.x & 63;
    const int tiles_x = (f.width + 7) >> 3;
    const int x = (tile % tiles_x) * 8 + (lane & 7);
    const int r = (tile / tiles_x) * 8 + (lane >> 3);
    render_pixel<FAST, COUNT>(sc, f, x, r, x < f.width && r < f.num_rows, dfr.blocks > 0, out, acc, cnt,
                                    cstack + threadIdx.x, blockDim.x, wstk, planes...);
    if (COUNT) {
        add_counts(counts, cnt);
        if (wave_stats && lane == 0) {
            // diagnostic: {tile, traversal steps of this wave, start, end} (100 MHz clock)
            const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
            uint32_t* w = wave_stats + 4 * (size_t)tile;
            w[0] = tile;
            w[1] = cnt.steps;
            w[2] = (uint32_t)t0;
            w[3] = (uint32_t)t1;
        }
    }
}

// MIRT_OPT_DEBUG_STALL_MS (test hook): one wave that waits `ticks` of the
// 100 MHz real-time clock, then exits -- a frame that cannot finish within a
// caller's deadline, bounded so the grid always drains.
__global__ void stall_kernel(uint64_t ticks)
{
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

__global__ void mark_deferred_kernel(FrameConst f, uint32_t* __restrict__ list, uint32_t* __restrict__ count)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= f.width || r >= f.num_rows) return;
    const Ray ray = camera_ray(f, x, shard_row_to_y(f, r), row_sample(f, r));
    if (slab_ray(ray).generic) list[atomicAdd(count, 1u)] = (uint32_t)(r * f.width + x);
}

// main.c:368-372 / 394-405 for one finished pixel i of the shard.
__device__ __forceinline__ void store_pixel(const FrameConst& f, uint32_t* __restrict__ out, float* __restrict__ acc,
                                            size_t i, uint32_t c)
{
    uint32_t shown = c;
    if (acc) {
        float* a = acc + 3 * i;
        for (int ch = 0; ch < 3; ch++) {
            const float v = (float)((c >> (8 * ch)) & 0xff) / 255.0f;
            if (f.accumulate) {
                a[ch] = a[ch] + v;
                const float avg = a[ch] / f.frames * 255.0f;
                const uint32_t q = (uint32_t)(int)fminf(avg, 255.0f);
                shown = (shown & ~(0xffu << (8 * ch))) | ((q & 0xffu) << (8 * ch));
            } else {
                a[ch] = v;
            }
        }
    }
    out[i] = shown;
}

// A launch of f.samples > 1 frames with an accumulation buffer (or any frame
// of a ctx whose accumulation buffer is shared, mirt_ctx_share_accum): the
// kernels wrote each frame's colours to its own slab of `out`; fold them
// into `acc` in frame order, exactly as f.samples successive store_pixel
// calls would (frame j: fresh if j == 0 and !f.accumulate, else divisor
// f.frames + j), leaving in slab j the display main.c:394-405 shows after
// frame j.
__global__ void fold_samples_kernel(FrameConst f, uint32_t* __restrict__ out, float* __restrict__ acc)
{
    const size_t n = (size_t)f.shard_rows * f.width;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* a = acc + 3 * i;
    float a0 = a[0], a1 = a[1], a2 = a[2];
    for (int j = 0; j < f.samples; j++) {
        const uint32_t c = out[(size_t)j * n + i];
        uint32_t shown = c;
        float* ch[3] = {&a0, &a1, &a2};
        for (int k = 0; k < 3; k++) {
            const float v = (float)((c >> (8 * k)) & 0xff) / 255.0f;       // main.c:368-370 / 394-396
            if (j == 0 && !f.accumulate) {
                *ch[k] = v;
            } else {
                *ch[k] = *ch[k] + v;
                const float avg = *ch[k] / (f.frames + (float)j) * 255.0f;  // main.c:398-400
                const uint32_t q = (uint32_t)(int)fminf(avg, 255.0f);
                shown = (shown & ~(0xffu << (8 * k))) | ((q & 0xffu) << (8 * k));
            }
        }
        out[(size_t)j * n + i] = shown;
    }
    a[0] = a0;
    a[1] = a1;
    a[2] = a2;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ------------------------------------------------------------------------
// Wavefront schedule (depth >= 2): the camera rays of 8x8 tiles are walked
// as packets (wave-uniform cursor); the bounce chains that follow are
// scattered, so they go through a queue to persistent waves in which every
// lane owns one pixel's chain and refills from the queue when it ends.

// Measured (scripts/ab_libs.py, 1080p/10k/depth 5, profiles/r02*_ab*.log): 192
// nodes at 4 waves/SIMD 1659 Mrays/s; 96 nodes at 5 waves/SIMD (the LDS of
// five workgroups then fits 160 KB) 1772; 6 waves/SIMD spills: 1587.
#ifndef MIRT_HCACHE
#define MIRT_HCACHE 16
#endif
constexpr uint32_t kHCache = MIRT_HCACHE;
constexpr int kBounceDiag = MIRT_BOUNCE_STATS_WORDS;  // mirt_bounce_stats words per wave  // HNodes staged in LDS per bounce workgroup (64 B each)

// The bounce queue's control words: {records written} in the first 128-B
// line, then one read head per queue SEGMENT, each in its own line. The
// bounce waves read the queue as kQSeg contiguous segments (the primary
// pass fills it in roughly tile order, so a segment is roughly a band of the
// image): the waves of workgroup b start on segment b % kQSeg -- the
// workgroups that share an XCD (dealt round-robin over the 8), so a
// segment's rays, and the nodes near their origins, stay in one XCD's L2 --
// and move on to the next segment when theirs runs dry. Eight heads also
// split the refill atomics that one word would serialise.
#ifndef MIRT_QSEG
#define MIRT_QSEG 8
#endif
constexpr uint32_t kQSeg = MIRT_QSEG;
constexpr uint32_t kQLine = 32;                        // dwords per 128-B line
constexpr size_t kQCtlBytes = 4 * kQLine * (1 + kQSeg);

// First bounce of one pixel, produced by primary_kernel.
struct BounceRec {
    float ox, oy, oz, dx, dy, dz;
    uint32_t pixel;  // r * width + x (shard-compacted row r)
    uint32_t k;      // RNG contract draws consumed so far
    uint32_t base0;  // colour of the camera ray's hit (renderer.c:49)
    uint32_t pad;
};


// ORD: the tree admits the ordered packet walk (DevScene::ordered), which
// also takes zero-component rays -- that build has no deferred waves and no
// other walk, so it keeps the register budget of the packet walk alone.
// BND (ORD only): the camera is within 4C of the origin (DevScene::o_bound):
// the packet walk tests the grown inner-child boxes without margins (trace.h).
// PLANES (as for render_kernel): with planes, the lane that owns a pixel
// stores its closest hit where the walk returns it; a pixel handed to a
// deferred wave is stored by that wave's lane 0 (render_pixel).
// PLANES = CacheFill / CacheRead (ORD only; the primary cache, trace.h): the
// walk's hit of each frame-0 pixel also goes to the cache, or comes from it
// with no walk at all. Tile mapping and queue grouping are the kernel's own, so
// the bounce pass receives the queue a walked frame gives it.
template <bool FAST, bool ORD, bool BND = false, class... PLANES>
// Register budget of the ordered camera-packet kernel (ORD): 8 waves per SIMD (64 VGPRs;
// 67 and 7 waves without the attribute). With four frames in flight
// its waves share the CUs with the bounce passes, and the eighth wave hides
// more of the packet walk's scalar-load latency (1080p/10k +0.3-1.1%,
// 1080p/100k +3.7%, profiles/r02_ab/r02ax_primary_waves8_*).
#ifndef MIRT_BOUNCE_WAVES
#define MIRT_BOUNCE_WAVES 5
#endif
#ifndef MIRT_PRIMARY_WAVES
#define MIRT_PRIMARY_WAVES 8
#endif
// (Round 3: the ordered kernel groups each workgroup's first bounces by
// direction octant in the queue -- scripts/tree_quality.cpp's lockstep model:
// distinct nodes per lane-step -9%, busy lanes per step +13%; measured +1.8%.)
#define MIRT_PRIMARY_ATTR __attribute__((amdgpu_waves_per_eu(ORD ? MIRT_PRIMARY_WAVES : 1)))
__global__ __launch_bounds__(256) MIRT_PRIMARY_ATTR void primary_kernel(DevScene sc, FrameConst f, uint32_t* __restrict__ out,
                                                      float* __restrict__ acc, Deferred dfr,
                                                      BounceRec* __restrict__ queue, uint32_t* __restrict__ qctl,
                                                      int octants = 1, PLANES... planes)
{
    constexpr bool kFill = (std::is_same_v<PLANES, CacheFill> || ... || false);
    constexpr bool kRead = (std::is_same_v<PLANES, CacheRead> || ... || false);
    static_assert(ORD || !(kFill || kRead), "the primary cache belongs to the ordered camera-packet kernel");
    __shared__ uint32_t cstack[ORD ? 1 : kMaxDepth * 256];
    Counters cnt{0, 0, 0, 0, 0};
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    // the workgroup's first bounces, grouped by direction octant before they
    // enter the queue (the last of the four waves to finish writes them)
    __shared__ BounceRec grec[ORD ? 256 : 1];
    __shared__ uint32_t gcount[4], gdone;
    if (ORD) {
        if (threadIdx.x == 0) gdone = 0;
        __syncthreads();
    }
    if constexpr (!ORD) {
        if ((int)blockIdx.x < dfr.blocks) {  // zero-component camera rays: whole path in this wave
            const uint32_t n = __builtin_amdgcn_readfirstlane(*dfr.count);
            const uint32_t stride = (uint32_t)(dfr.blocks * 4);
            for (uint32_t j = blockIdx.x * 4 + wave; j < n; j += stride) {
                const uint32_t p = __builtin_amdgcn_readfirstlane(dfr.list[j]);
                render_pixel<FAST, false>(sc, f, (int)(p % f.width), (int)(p / f.width), lane == 0, false,
                                                         out, acc, cnt, cstack + threadIdx.x, 256, nullptr, planes...);
            }
            return;
        }
    }
    const int tile = (blockIdx.x - dfr.blocks) * 4 + wave;
    int x, r;
    bool alive;
    if (ORD && f.samples >= 4) {
        // four frames in flight or more (frames of one camera, or jittered
        // samples of one pixel): a packet is 4x4 pixels x 4 successive frames,
        // whose camera rays are the same or nearly so -- a quarter of an 8x8
        // tile's footprint, so the packet's walk is the union of fewer paths
        // (launch_render_body's ptiles counts these tiles)
        const int txs = (f.width + 3) >> 2, tys = (f.shard_rows + 3) >> 2;
        const int g = tile / (txs * tys), rem = tile - g * (txs * tys);
        x = (rem % txs) * 4 + (lane & 3);
        const int yr = (rem / txs) * 4 + ((lane >> 2) & 3);
        const int j = g * 4 + (lane >> 4);
        alive = x < f.width && yr < f.shard_rows && j < f.samples;
        r = j * f.shard_rows + yr;
    } else {
        const int tiles_x = (f.width + 7) >> 3;
        x = (tile % tiles_x) * 8 + (lane & 7);
        r = (tile / tiles_x) * 8 + (lane >> 3);
        alive = x < f.width && r < f.num_rows;
    }
    const int y = alive ? shard_row_to_y(f, r) : 0;
    const Ray ray = camera_ray(f, alive ? x : 0, y, row_sample(f, r));
    if (!ORD && dfr.blocks > 0 && alive && slab_ray(ray).generic) alive = false;  // traced by a deferred wave
    float t;
    int s;
    if constexpr (kRead) {
        // the stored hit of the pixel's frame-0 twin: launch row r is row
        // r - j * shard_rows of frame j (8x8 tiles straddle frames; in the
        // 4x4x4 packets that is yr), j by row_sample's division
        t = 0.0f;
        s = -1;
        if (alive) {
            int cr = r;
            if (f.samples > 1) cr -= (int)magic_div((uint32_t)r, (uint32_t)f.shard_rows, f.magic.shard_rows) * f.shard_rows;
            (load_cached(planes, (size_t)cr * f.width + x, t, s), ...);
        }
    } else if constexpr (ORD) {
        closest_packet_ordered<FAST, false, BND>(sc, ray, alive, t, s, cnt);
    } else
        closest_hit<true, FAST, false>(sc, ray, alive, t, s, cnt);
    const size_t i = (size_t)r * f.width + x;
    if constexpr (kFill) {
        // frame 0's lanes only (j == 0 in the 4x4x4 packets): the cache holds one slab
        if (alive && r < f.shard_rows) (store_planes(planes, i, sc, ray, t, s), ...);
    } else if constexpr (!kRead && sizeof...(PLANES) > 0) {
        if (alive) (store_planes(planes, i, sc, ray, t, s), ...);
    }
    bool push = false;
    BounceRec rec;
    if (alive) {
        if (s < 0) {
            store_pixel(f, out, acc, i, sky_rgba(ray.dy));      // renderer.c:65-70
        } else if (f.depth < 2) {
            // depth 1: the bounce would be traced with depth 0 and return
            // black (renderer.c:23-24), so the pixel is base + 0.5 * black
            store_pixel(f, out, acc, i, blend_rgba(sc.color[s], 255u << 24));
        } else {
            // renderer.c:49-55: base colour, then the bounce (depth >= 2 here)
            const float4 g = sc.geo[s];
            float p[3], n[3];
            hit_point_normal(ray, t, g, p, n);
            uint32_t k = 0;
            float bx, by, bz;
            hemisphere(pixel_key(f.seed, (uint32_t)(y * f.width + x), row_sample(f, r)), k, n, bx, by, bz);
            rec = BounceRec{p[0], p[1], p[2], bx, by, bz, (uint32_t)i, k, sc.color[s], 0u};
            push = true;
        }
    }
    const uint64_t pm = __ballot(push);
    if constexpr (ORD) {
        if (push) grec[wave * 64 + lanes_below(pm)] = rec;
        if (lane == 0) gcount[wave] = (uint32_t)__popcll(pm);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        uint32_t prev = 0;
        if (lane == 0) prev = __hip_atomic_fetch_add(&gdone, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_readfirstlane(prev) != (blockDim.x >> 6) - 1) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // the last wave: octant of each record's direction, counts per
        // (wave, octant), then every record to base + its octant's offset.
        // octants == 0 (a frame alone on its ctx: the blocking call): tile
        // order, still one queue atomic per workgroup -- measured (DESIGN
        // §8): the lone frame's bounce pass is 2-4% shorter in tile order,
        // frames in flight are 1% faster grouped
        const int nw = blockDim.x >> 6;
        uint32_t oct[4], tot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, total = 0;
        bool has[4];
        for (int w = 0; w < nw; w++) {
            const uint32_t n = gcount[w];
            has[w] = (uint32_t)lane < n;
            const BounceRec& r = grec[w * 64 + (has[w] ? lane : 0)];
            oct[w] = octants ? (r.dx < 0.0f ? 1u : 0u) | (r.dy < 0.0f ? 2u : 0u) | (r.dz < 0.0f ? 4u : 0u) : 0u;
            for (uint32_t o = 0; o < 8; o++) tot[o] += (uint32_t)__popcll(__ballot(has[w] && oct[w] == o));
            total += n;
        }
        if (!total) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&qctl[0], total);
        base = __builtin_amdgcn_readfirstlane(base);
        uint32_t run[8];
        for (uint32_t o = 0, acc = 0; o < 8; o++) {
            run[o] = base + acc;
            acc += tot[o];
        }
        for (int w = 0; w < nw; w++) {
            uint32_t pos = 0;
            for (uint32_t o = 0; o < 8; o++) {
                const uint64_t m = __ballot(has[w] && oct[w] == o);
                if (has[w] && oct[w] == o) pos = run[o] + lanes_below(m);
                run[o] += (uint32_t)__popcll(m);
            }
            if (has[w]) queue[pos] = grec[w * 64 + lane];
        }
        return;
    }
    if (pm) {  // one atomic per wave; records stay in tile order
        const int leader = __builtin_ctzll(pm);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&qctl[0], (uint32_t)__popcll(pm));
        base = __builtin_amdgcn_readlane(base, leader);
        if (push) queue[base + lanes_below(pm)] = rec;
    }
}

// ------------------------------------------------------------------------
// The primary scan (MIRT_OPT_PRIMARY_SCAN; pscan.h): the camera
// rays' closest hits of one slab found without the packet walk, into a slab of
// the primary cache's format that primary_kernel<true, true, false, CacheRead>
// then shades. For a tree whose boxes nest the closest hit is the least t, a
// tie to the larger sphere index, among the leaves whose sphere_t<true> hits
// and whose exact LeafBox passes slab_box<true> -- leaf_gate's rule,
// whatever the order the leaves are met in.
struct PscanDev {
    const PscanRec* rec;   // nl records by ascending key
    const int* grid;       // records holding tile (i, j) of the image: grid[j * gw + i]
    uint32_t nl;
    int gw;
    float gx, gy, gz;      // G (pscan.h)
    float* t;              // the slab: shard_rows * width each
    int32_t* sphere;
    uint32_t* wlist;       // [0]: tiles listed; then the tiles
    unsigned long long* stats;  // kPscanSlots lines of {tiles done, tiles listed, tiles without a record, chunks, leaves, records holding the listed or done tiles}
    int budget;            // chunks a tile with a lane still without a hit may read before it is listed
};
constexpr int kPscanSlots = 64, kPscanSlotWords = 8;
constexpr uint32_t kPscanHardBudget = 1024;   // chunks any tile may read (64 Ki records: a guard, never met in MEASUREMENTS E)

// One wave per 8x8 tile of the slab (primary_kernel's tiles of one frame),
// lanes as primary_kernel's. The records come 64 at a time, one per lane, in
// key order; the lanes whose rectangle holds the tile are tested one after
// the other against all 64 rays by leaf_gate. Before a chunk the tile is done
// when every live lane holds a hit nearer (strictly, pscan_depth_hi) than the
// chunk's first key -- no record from there on can win or tie -- or when it has
// met all the records that hold it. A tile not done within `budget` chunks
// lists itself for pscan_walk_kernel and stores nothing.
__global__ __launch_bounds__(256) void pscan_tile_kernel(DevScene sc, FrameConst f, PscanDev ps)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles_x = (f.width + 7) >> 3, tiles_y = (f.shard_rows + 7) >> 3;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= tiles_x * tiles_y) return;
    const int ti = tile % tiles_x, tr = tile / tiles_x;
    const int x = ti * 8 + (lane & 7), r = tr * 8 + (lane >> 3);
    const bool alive = x < f.width && r < f.shard_rows;
    const int y = alive ? shard_row_to_y(f, r) : 0;
    const Ray ray = camera_ray(f, alive ? x : 0, y, f.sample);
    // the tile's rows are one band of eight image rows (the classification)
    const uint32_t tj = (uint32_t)__builtin_amdgcn_readfirstlane(y) >> 3;
    const uint32_t want = (uint32_t)ps.grid[tj * ps.gw + ti];
    const SlabRay sr = slab_ray(ray);
    const SphRay sp = sph_ray(ray);
    Prune pr = prune_start(sc, ray.ox, ray.oy, ray.oz);
    const float dg = dot3(ray.dx, ray.dy, ray.dz, ps.gx, ps.gy, ps.gz);
    float best_t = INFINITY;
    int best_s = -1;
    const uint32_t nchunks = (ps.nl + 63) >> 6;
    uint32_t seen = 0, chunk = 0, tested = 0;
    bool done = false;
    for (;; chunk++) {
        if (seen >= want || chunk >= nchunks) {
            done = true;
            break;
        }
        const uint32_t k = chunk * 64 + lane;
        PscanRec rec{INFINITY, 0u, kPscanEmpty, kPscanEmpty};
        if (k < ps.nl) rec = ps.rec[k];
        const float z0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, rec.z)));
        const bool open = alive && !(best_s >= 0 && pscan_depth_hi(best_t, dg) < z0);
        if (!__ballot(open)) {
            done = true;
            break;
        }
        // a tile whose live lanes all hold a hit ends by depth, within a few chunks of its last winner; one
        // with a lane still without a hit (a sky pixel) can only end on its count, as far into the records as
        // its farthest candidate lies: that tile is listed after `budget` chunks, any tile after kPscanHardBudget
        if (chunk >= kPscanHardBudget || (chunk >= (uint32_t)ps.budget && __ballot(alive && best_s < 0))) break;
        uint64_t m = __ballot(pscan_rec_holds(rec, (uint32_t)ti, tj));
        seen += (uint32_t)__popcll(m);
        tested += (uint32_t)__popcll(m);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)rec.leaf, b);
            const float4 g = load_geo_uniform(sc.leaf_geo, (int)li);
            if (alive) leaf_gate(sc, sr, sp, pr, li, g, best_t, best_s);
        }
    }
    if (done) {
        if (alive) {
            const size_t i = (size_t)r * f.width + x;
            ps.t[i] = best_s >= 0 ? best_t : 0.0f;
            ps.sphere[i] = best_s >= 0 ? best_s : -1;
        }
    } else if (lane == 0) {
        ps.wlist[1 + atomicAdd(&ps.wlist[0], 1u)] = (uint32_t)tile;
    }
    if (lane == 0) {
        unsigned long long* st = ps.stats + (size_t)(blockIdx.x % kPscanSlots) * kPscanSlotWords;
        atomicAdd(&st[done ? (want ? 0 : 2) : 1], 1ull);
        if (chunk) atomicAdd(&st[3], (unsigned long long)chunk);
        if (tested) atomicAdd(&st[4], (unsigned long long)tested);
        if (want) atomicAdd(&st[5], (unsigned long long)want);
    }
}

// The listed tiles by the packet walk, into the same slab: a fixed grid
// strided over the list, whose length is read here.
template <bool BND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MIRT_PRIMARY_WAVES))) void pscan_walk_kernel(DevScene sc, FrameConst f, PscanDev ps)
{
    const int lane = threadIdx.x & 63;
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)ps.wlist[0]);
    const int tiles_x = (f.width + 7) >> 3;
    Counters cnt{0, 0, 0, 0, 0};
    for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += gridDim.x * 4) {
        const int tile = __builtin_amdgcn_readfirstlane((int)ps.wlist[1 + j]);
        const int x = (tile % tiles_x) * 8 + (lane & 7), r = (tile / tiles_x) * 8 + (lane >> 3);
        const bool alive = x < f.width && r < f.shard_rows;
        const int y = alive ? shard_row_to_y(f, r) : 0;
        const Ray ray = camera_ray(f, alive ? x : 0, y, f.sample);
        float t;
        int s;
        closest_packet_ordered<true, false, BND>(sc, ray, alive, t, s, cnt);
        if (alive) {
            const size_t i = (size_t)r * f.width + x;
            ps.t[i] = s >= 0 ? t : 0.0f;
            ps.sphere[i] = s >= 0 ? s : -1;
        }
    }
}

// The automatic mode's verdict on a scanned frame, from the frame's own
// counters: a scene whose tiles that hold a record read more than
// kPscanSparseChunks chunks each on average is one where most such tiles keep a
// sky pixel and can only end on their count (MEASUREMENTS E: the walk is then
// the faster camera pass). The scene's id goes to page-locked host memory,
// where ps_classify finds it at a later enqueue without waiting for anything.
constexpr unsigned long long kPscanSparseChunks = 16;
__global__ void pscan_verdict_kernel(const unsigned long long* __restrict__ stats, unsigned long long* verdict,
                                     unsigned long long scene_id)
{
    unsigned long long tiles = 0, chunks = 0;
    for (int k = 0; k < kPscanSlots; k++) {
        tiles += stats[k * kPscanSlotWords] + stats[k * kPscanSlotWords + 1];
        chunks += stats[k * kPscanSlotWords + 3];
    }
    if (chunks > kPscanSparseChunks * tiles)
        __hip_atomic_store(verdict, scene_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------
// Ray frames (mirt_render_rays*): a frame in every respect, except that the
// camera ray of launch pixel i = r * width + x (the index of the colour
// output and of the planes, computed in size_t) is rays[i], a caller's ray
// used as given. The pixel's RNG key stays the frame's (chain_key), so the
// bounce pass, the folds and the accumulation are the plain frame's. The
// kernels are their own, not further instantiations of primary_kernel /
// render_kernel: a frame without rays keeps its kernels' arguments and code.

// One wave per 8x8 pixel tile, as the plain frame kernels: a tile row's eight
// rays are 192 contiguous bytes, and the rays of neighbouring pixels are the
// ones most likely to walk the same nodes.
// (MIRT_RAY_TILE 0, for measurements: 64 successive pixels of a row per wave.)
#ifndef MIRT_RAY_TILE
#define MIRT_RAY_TILE 1
#endif
__device__ __forceinline__ bool ray_tile_pixel(const FrameConst& f, int& x, int& r)
{
    if (!MIRT_RAY_TILE) {   // the grid's lanes (64 per tile) are no fewer than the pixels
        const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        r = (int)(i / (size_t)f.width);
        x = (int)(i - (size_t)r * f.width);
        return i < (size_t)f.num_rows * f.width;
    }
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tiles_x = (f.width + 7) >> 3;
    x = (tile % tiles_x) * 8 + (lane & 7);
    r = (tile / tiles_x) * 8 + (lane >> 3);
    return x < f.width && r < f.num_rows;
}

__device__ __forceinline__ Ray load_ray(const mirt_ray* __restrict__ rays, size_t i)
{
    const mirt_ray& rr = rays[i];
    return Ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
}

// The primary pass of a ray frame on the wavefront schedule (use_bvh, any
// depth). Caller's rays are incoherent for all the kernel knows: each lane
// walks its own (the walk of intersect_kernel, closest_hit<false>: four-wide
// with an LDS stack column where the tree admits it, zero-component rays and
// far origins included), so there are no packets and no deferred waves. Behind
// the walk it is primary_kernel: sky, base + half black below depth 2, else the
// first bounce into the queue (one atomic per wave, tile order) for the
// bounce_kernel the ctx's options select. Depth 0 is black without a walk
// (renderer.c:23-24). PLANES as for primary_kernel.
template <bool FAST, class... PLANES>
__global__ __launch_bounds__(256) void ray_primary_kernel(DevScene sc, FrameConst f, const mirt_ray* __restrict__ rays,
                                                          uint32_t* __restrict__ out, float* __restrict__ acc,
                                                          BounceRec* __restrict__ queue, uint32_t* __restrict__ qctl,
                                                          PLANES... planes)
{
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    int x, r;
    const bool alive = ray_tile_pixel(f, x, r);
    const size_t i = alive ? (size_t)r * f.width + x : 0;
    if (f.depth < 1) {
        if (alive) store_pixel(f, out, acc, i, 255u << 24);
        return;
    }
    const Ray ray = load_ray(rays, i);
    Counters cnt{0, 0, 0, 0, 0};
    float t;
    int s;
    // (zero-component rays: closest_hit hands each to the whole wave in turn.
    // Keeping them in their lanes of the four-wide walk, whose exact box test
    // cannot order or cull by distance, measured 3.3x slower on the pinhole's
    // centre row and column and 7x slower on an orthographic frame)
    closest_hit<false, FAST, false>(sc, ray, alive, t, s, cnt, wstack + threadIdx.x);
    if constexpr (sizeof...(PLANES) > 0) {
        if (alive) (store_planes(planes, i, sc, ray, t, s), ...);
    }
    bool push = false;
    BounceRec rec;
    if (alive) {
        if (s < 0) {
            store_pixel(f, out, acc, i, sky_rgba(ray.dy));      // renderer.c:65-70
        } else if (f.depth < 2) {
            store_pixel(f, out, acc, i, blend_rgba(sc.color[s], 255u << 24));
        } else {
            const float4 g = sc.geo[s];
            float p[3], n[3];
            hit_point_normal(ray, t, g, p, n);
            uint32_t k = 0;
            float bx, by, bz;
            hemisphere(pixel_key(f.seed, (uint32_t)(shard_row_to_y(f, r) * f.width + x), row_sample(f, r)), k, n, bx, by,
                       bz);
            rec = BounceRec{p[0], p[1], p[2], bx, by, bz, (uint32_t)i, k, sc.color[s], 0u};
            push = true;
        }
    }
    const uint64_t pm = __ballot(push);
    if (pm) {
        const int lane = threadIdx.x & 63, leader = __builtin_ctzll(pm);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&qctl[0], (uint32_t)__popcll(pm));
        base = __builtin_amdgcn_readlane(base, leader);
        if (push) queue[base + lanes_below(pm)] = rec;
    }
}

// A ray frame on every other schedule (MIRT_TRAV_TILE, brute force): each lane
// traces its pixel's whole path, as render_kernel does (trace_path, with the
// planes' slot), from the loaded ray. trace_path takes zero-component rays
// itself, so nothing is deferred.
template <bool FAST, class... PLANES>
__global__ __launch_bounds__(256) void ray_path_kernel(DevScene sc, FrameConst f, const mirt_ray* __restrict__ rays,
                                                       uint32_t* __restrict__ out, float* __restrict__ acc,
                                                       PLANES... planes)
{
    __shared__ uint32_t cstack[kMaxDepth * 256];
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    int x, r;
    const bool alive = ray_tile_pixel(f, x, r);
    const size_t i = alive ? (size_t)r * f.width + x : 0;
    const Ray ray = load_ray(rays, i);
    const int y = alive ? shard_row_to_y(f, r) : 0;
    Counters cnt{0, 0, 0, 0, 0};
    const uint32_t c = trace_path<FAST, false>(sc, ray, alive, f.depth, f.use_bvh != 0,
                                               pixel_key(f.seed, (uint32_t)(y * f.width + x), row_sample(f, r)), cnt,
                                               cstack + threadIdx.x, 256, wstack + threadIdx.x, PlaneSlot{planes, i}...);
    if (alive) store_pixel(f, out, acc, i, c);
}

// ------------------------------------------------------------------------
// Lens frames (mirt_render_lens_frame*): a ray frame whose rays the camera pass
// computes itself -- each lane its pixel's thin-lens ray, from the pinhole ray
// and the pixel's RNG contract stream (lens.h has the definition) -- so no ray
// buffer exists anywhere. What follows the ray is the ray frame's, line for
// line; the kernels are their own so that the plain and the ray kernels keep
// their arguments and their code.

// The lens ray of pixel (x, image row y) of RNG sample `sample` under `key`,
// the pixel's own key: what mirt_lens_rays writes and both frame kernels trace.
__device__ __forceinline__ Ray lens_camera_ray(const FrameConst& f, const LensConst& lc, int x, int y, uint32_t sample,
                                               uint64_t key)
{
    const Ray pr = camera_ray(f, x, y, sample);
    const float p[3] = {pr.ox, pr.oy, pr.oz}, d[3] = {pr.dx, pr.dy, pr.dz};
    float o[3], n[3];
    lens_ray(lc, key, p, d, o, n);
    normalize3(n[0], n[1], n[2]);
    return Ray{o[0], o[1], o[2], n[0], n[1], n[2]};
}

// The camera pass of a lens frame on the wavefront schedule: ray_primary_kernel
// with the lane's ray computed in registers from (x, image row, row_sample).
// The origins differ from lane to lane, so the walk is the per-lane one
// (closest_hit<false>), not the pinhole's packets. Depth 0 stores black
// without computing a ray.
template <bool FAST, class... PLANES>
__global__ __launch_bounds__(256) void lens_primary_kernel(DevScene sc, FrameConst f, LensConst lc,
                                                           uint32_t* __restrict__ out, float* __restrict__ acc,
                                                           BounceRec* __restrict__ queue, uint32_t* __restrict__ qctl,
                                                           PLANES... planes)
{
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    int x, r;
    const bool alive = ray_tile_pixel(f, x, r);
    const size_t i = alive ? (size_t)r * f.width + x : 0;
    if (f.depth < 1) {
        if (alive) store_pixel(f, out, acc, i, 255u << 24);
        return;
    }
    if (!alive) x = r = 0;   // a dead lane computes pixel 0's ray and walks nothing
    const int y = shard_row_to_y(f, r);
    const uint64_t key = pixel_key(f.seed, (uint32_t)(y * f.width + x), row_sample(f, r));
    const Ray ray = lens_camera_ray(f, lc, x, y, row_sample(f, r), key);
    Counters cnt{0, 0, 0, 0, 0};
    float t;
    int s;
    closest_hit<false, FAST, false>(sc, ray, alive, t, s, cnt, wstack + threadIdx.x);
    if constexpr (sizeof...(PLANES) > 0) {
        if (alive) (store_planes(planes, i, sc, ray, t, s), ...);
    }
    bool push = false;
    BounceRec rec;
    if (alive) {
        if (s < 0) {
            store_pixel(f, out, acc, i, sky_rgba(ray.dy));      // renderer.c:65-70
        } else if (f.depth < 2) {
            store_pixel(f, out, acc, i, blend_rgba(sc.color[s], 255u << 24));
        } else {
            const float4 g = sc.geo[s];
            float p[3], n[3];
            hit_point_normal(ray, t, g, p, n);
            uint32_t k = 0;
            float bx, by, bz;
            hemisphere(key, k, n, bx, by, bz);
            rec = BounceRec{p[0], p[1], p[2], bx, by, bz, (uint32_t)i, k, sc.color[s], 0u};
            push = true;
        }
    }
    const uint64_t pm = __ballot(push);
    if (pm) {
        const int lane = threadIdx.x & 63, leader = __builtin_ctzll(pm);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&qctl[0], (uint32_t)__popcll(pm));
        base = __builtin_amdgcn_readlane(base, leader);
        if (push) queue[base + lanes_below(pm)] = rec;
    }
}

// A lens frame on every other schedule (MIRT_TRAV_TILE, brute force, the exact
// slab, unordered trees): ray_path_kernel with the computed ray.
template <bool FAST, class... PLANES>
__global__ __launch_bounds__(256) void lens_path_kernel(DevScene sc, FrameConst f, LensConst lc,
                                                        uint32_t* __restrict__ out, float* __restrict__ acc,
                                                        PLANES... planes)
{
    __shared__ uint32_t cstack[kMaxDepth * 256];
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    int x, r;
    const bool alive = ray_tile_pixel(f, x, r);
    const size_t i = alive ? (size_t)r * f.width + x : 0;
    if (!alive) x = r = 0;
    const int y = shard_row_to_y(f, r);
    const uint64_t key = pixel_key(f.seed, (uint32_t)(y * f.width + x), row_sample(f, r));
    const Ray ray = lens_camera_ray(f, lc, x, y, row_sample(f, r), key);
    Counters cnt{0, 0, 0, 0, 0};
    const uint32_t c = trace_path<FAST, false>(sc, ray, alive, f.depth, f.use_bvh != 0, key, cnt, cstack + threadIdx.x,
                                               256, wstack + threadIdx.x, PlaneSlot{planes, i}...);
    if (alive) store_pixel(f, out, acc, i, c);
}

// mirt_lens_rays: the rays a lens frame traces, indexed as its colour output.
__global__ void lens_rays_kernel(FrameConst f, LensConst lc, mirt_ray* __restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= f.width || r >= f.num_rows) return;
    const int y = shard_row_to_y(f, r);
    const Ray ray = lens_camera_ray(f, lc, x, y, row_sample(f, r),
                                    pixel_key(f.seed, (uint32_t)(y * f.width + x), row_sample(f, r)));
    out[(size_t)r * f.width + x] = {{ray.ox, ray.oy, ray.oz}, {ray.dx, ray.dy, ray.dz}};
}

// The bounce kernel's walks test the HNode slot boxes without
// slab_cons_fast's margins (trace.h, BND): the boxes are grown by 2^-19
// DevScene::o_bound at upload, and a bounce ray whose origin lies within that
// bound -- a hit point in the scene -- needs no more; an origin beyond it (or
// NaN) takes the exact test, and so does every ray of a scene without a bound
// (o_bound == 0: its boxes were never grown, and an origin of exactly zero
// would otherwise pass max|o| <= 0). Round 6: serial bounce pass 0.84-0.86 ->
// 0.83 ms, 1080p/10k +1.5-3%, 1080p/100k +3.5% (MEASUREMENTS.md §D).
constexpr bool kBoundedSlab = true;
__device__ __forceinline__ SlabRay bounce_slab_ray(const DevScene& sc, const Ray& ray)
{
    SlabRay s = slab_ray(ray);
    s.generic = s.generic ||
                !(sc.o_bound > 0.0f && fmaxf(fabsf(ray.ox), fmaxf(fabsf(ray.oy), fabsf(ray.oz))) <= sc.o_bound);
    return s;
}

// The camera rays' form of that rule (trace.h slab_cons_fast<BND>: an origin
// within 4C still fits the growth), decided once per frame on the host
// (camera_bounded).
__host__ __device__ inline bool origin_within_4c(float o_bound, float o_inf)
{
    return o_bound > 0.0f && o_inf <= 4.0f * o_bound;
}

// The walk of one bounce ray: WALK 0 = reference DFS order (any tree),
// 2 = ordered four-wide (HNode, LDS stack).
template <int WALK>
struct BounceWalk;
template <>
struct BounceWalk<0> {
    DfsWalk w;
    __device__ void start(const DevScene& sc) { w = DfsWalk{0u, sc.num_nodes}; }
    __device__ void stop() { w = DfsWalk{kPNone, 0u}; }
    __device__ bool walking() const { return w.cur != kPNone; }
    template <bool FAST>
    __device__ void step(const DevScene& sc, const SlabRay& sr, const SphRay& sp, Prune& pr, uint32_t*, float& bt,
                         int& bs, Counters& cnt)
    {
        lane_step<FAST, false>(sc, sr, sp, pr, w.cur, bt, bs, cnt);
        if (w.cur >= w.end) w.cur = kPNone;
    }
};
template <int WALK>
struct WideBounceWalk {  // WALK 2: four-wide; 4: four-wide, a step's leaf spheres loaded together
    WideWalk w;
    lds_uint4* hc = nullptr;  // the top HNodes staged in LDS (bounce_kernel)
    uint32_t hc_n = 0;
    __device__ void start(const DevScene& sc) { w = wide_walk_start(sc, true); }
    __device__ void stop() { w = WideWalk{kPNone, 0u, 0u}; }
    __device__ bool walking() const { return wide_walking(w); }
    template <bool FAST, bool GD = false, bool DEFER = false>
    __device__ void step(const DevScene& sc, const SlabRay& sr, const SphRay& sp, Prune& pr, uint32_t* stk,
                         float& bt, int& bs, Counters& cnt, GateDiag* gd = nullptr, int* lvl = nullptr)
    {
        // the bounded test in WALK 2; WALK 4 (trees past the L2) keeps the
        // margins: with its batched leaf loads the bounded form spills more
        // (4K/1M: -8%, MEASUREMENTS.md §D)
        wide_lane_step<FAST, false, WALK == 4, kBoundedSlab && WALK != 4, GD, DEFER>(sc, sr, sp, pr, w, stk, bt, bs,
                                                                                     cnt, hc, hc_n, gd, lvl);
    }
};
template <>
struct BounceWalk<2> : WideBounceWalk<2> {};
template <>
struct BounceWalk<4> : WideBounceWalk<4> {};

// DIAG (mirt_bounce_stats): per wave {loop iterations, walking lanes summed
// over them, the same two after the queue ran dry, start / queue-dry / end
// time (100 MHz clock), longest chain << 32 | longest walk (in steps)}, and
// of the lane loop's leaf gates (trace.h GateDiag; WALK 2, the lane loop
// only): gate executions, those in which any lane ran the f64 t / loaded the
// LeafBox, the lanes that did, and the loop iterations that held a gate / an
// f64 t / a LeafBox load; then the closest hits confirmed, the confirmations
// that failed, and the walks restarted in exact mode for a DFS segment.

// Dynamic LDS of a bounce launch: the colour stack's rows for a frame of
// `depth` levels (bounce levels 1 .. depth - 1 store a colour each).
inline size_t bounce_lds_bytes(int depth) { return sizeof(uint32_t) * 256 * (size_t)std::max(depth - 1, 1); }

// The RNG key of the pixel a bounce chain belongs to (rng.h: the per-pixel
// stream of its full-frame index and sample), recomputed where a level is
// shaded rather than held in two registers for the whole walk.
__device__ __forceinline__ uint64_t chain_key(const FrameConst& f, uint32_t pixel)
{
    const int r = (int)magic_div(pixel, (uint32_t)f.width, f.magic.width), x = (int)(pixel - (uint32_t)r * (uint32_t)f.width);
    return pixel_key(f.seed, (uint32_t)(shard_row_to_y(f, r) * f.width + x), row_sample(f, r));
}

// The shading of one lane whose walk for this level is done (renderer.c:46-77
// for that level): returns true if the chain goes on (ray re-aimed); else the
// pixel's colour is folded from the colour stack and stored (if `store`).
__device__ __forceinline__ bool shade_level(const DevScene& sc, const FrameConst& f, Ray& ray, float best_t,
                                            int best_s, int& level, uint32_t& k, uint64_t key, uint32_t* cs,
                                            int cstride, uint32_t base0, uint32_t pixel, uint32_t* __restrict__ out,
                                            float* __restrict__ acc, bool store)
{
    uint32_t tail = 255u << 24;  // depth exhausted: black (renderer.c:23-24)
    int stored = level - 1;
    if (best_s < 0) {
        tail = sky_rgba(ray.dy);
    } else {
        cs[(level - 1) * cstride] = sc.color[best_s];
        stored = level;
        if (level + 1 < f.depth) {  // trace_ray(bounce, depth - 1) still has depth
            const float4 g = sc.geo[best_s];
            float p[3], nn[3];
            hit_point_normal(ray, best_t, g, p, nn);
            float bx, by, bz;
            hemisphere(key, k, nn, bx, by, bz);
            ray = Ray{p[0], p[1], p[2], bx, by, bz};
            level++;
            return true;
        }
    }
    uint32_t c = tail;
    for (int l = stored - 1; l >= 0; l--) c = blend_rgba(cs[l * cstride], c);
    if (store) store_pixel(f, out, acc, pixel, blend_rgba(base0, c));
    return false;
}


// The rest of the chain of the wave's one remaining ray (held by the quad of
// lane l0), every lane of the wave taking part: its state broadcast from l0,
// its stack moved from its source lane's column to the wave layout of
// solo_step, each level walked with solo_step and shaded as shade_level
// (lane 0 stores the pixel).
template <bool FAST, bool BND>
__device__ __forceinline__ void solo_chain(const DevScene& sc, const FrameConst& f, int l0, Ray ray, float best_t,
                                        int best_s, Prune pr, QuadWalk qw, int level, uint32_t k, uint32_t pixel,
                                        uint32_t base0, uint32_t src, uint32_t* wst, uint32_t* wcs,
                                        uint32_t* __restrict__ out, float* __restrict__ acc, lds_uint4* hc,
                                        uint32_t hc_n, uint32_t lane = threadIdx.x & 63)
{
    auto bu = [&](uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l0); };
    auto bf = [&](float v) { return __uint_as_float(bu(__float_as_uint(v))); };
    ray = Ray{bf(ray.ox), bf(ray.oy), bf(ray.oz), bf(ray.dx), bf(ray.dy), bf(ray.dz)};
    best_t = bf(best_t);
    best_s = (int)bu((uint32_t)best_s);
    pr = Prune{bf(pr.m), bf(pr.lim)};
    level = (int)bu((uint32_t)level);
    k = bu(k);
    pixel = bu(pixel);
    base0 = bu(base0);
    src = bu(src);
    const uint32_t cur = bu(qw.cur), end = bu(qw.end), top = bu(qw.top);
    // the stack (top <= kWideStack entries, column src) to the wave layout
    uint32_t v = 0;
    if (lane < top) v = wst[lane * kWideStride + src];
    __builtin_amdgcn_wave_barrier();
    if (lane < top) *solo_slot(wst, lane) = v;
    uint32_t* cs = wcs + src;  // the colour stack stays in the source column
    SlabRay sr = bounce_slab_ray(sc, ray);
    SphRay sp = sph_ray(ray);
    SoloWalk w{lane < 4 ? cur : kPNone, lane < 4 ? end : 0u, top};
    for (;;) {
        while (solo_step<FAST, kWideStack * 64, BND>(sc, sr, sp, pr, w, wst, best_t, best_s, hc, hc_n, lane)) {
        }
        if (!shade_level(sc, f, ray, best_t, best_s, level, k, chain_key(f, pixel), cs, kWideStride, base0, pixel, out,
                         acc, lane == 0))
            return;
        sr = bounce_slab_ray(sc, ray);
        sp = sph_ray(ray);
        w = SoloWalk{lane < 4 ? sc.wide_root : kPNone, 0u, 0u};
        best_t = INFINITY;
        best_s = -1;
        pr = prune_off();
    }
}

// Persistent bounce pass: each lane owns one pixel's chain of bounces,
// refilled from the primary pass's queue. WALK 2 (default) ends with a QUAD
// DRAIN: once the queue is dry and at most 16 of
// a wave's lanes are still busy, their chains move to quads (registers by
// ds_bpermute; the LDS stacks stay in the source lane's columns) and are
// finished four lanes per ray -- a sparse wave costs full issue slots per
// step, so four lanes per ray make the drain's steps about four times
// shorter at no extra cost.
// Register budget of the bounce kernel: 5 waves per SIMD (<= 96 VGPRs; 4
// without the attribute, at 114). The pipelined frames gain most: the
// co-running primary pass gets the issue slots the fifth wave hides.
#define MIRT_BOUNCE_ATTR __attribute__((amdgpu_waves_per_eu(MIRT_BOUNCE_WAVES)))
template <bool FAST, int WALK, bool DIAG = false>
__global__ __launch_bounds__(256) MIRT_BOUNCE_ATTR void bounce_kernel(DevScene sc, FrameConst f, uint32_t* __restrict__ out,
                                                     float* __restrict__ acc, const BounceRec* __restrict__ queue,
                                                     uint32_t* __restrict__ qctl, int threshold, int quad_drain,
                                                     int lvl_mode, int fail_n,
                                                     uint64_t* __restrict__ diag = nullptr)
{
    uint64_t dg_it = 0, dg_lanes = 0, dg_it_x = 0, dg_lanes_x = 0, dg_tx = 0, dg_qit = 0, dg_tq = 0;
    const uint64_t dg_t0 = DIAG ? __builtin_amdgcn_s_memrealtime() : 0;
    uint32_t dg_steps = 0, dg_chain = 0, dg_walk_max = 0, dg_chain_max = 0;
    uint64_t dg_seg = 0, dg_fb = 0, dg_it_gate = 0, dg_it_t = 0, dg_it_box = 0;
    uint32_t dg_conf = 0, dg_conf_fail = 0, dg_fb_exact = 0;
    GateDiag gd{0, 0, 0, 0, 0, false, false, false};
    constexpr bool LANE4 = WALK == 2 || WALK == 4;  // four-wide, one ray per lane
    // the lane loop's walks confirm their closest hit once, when the level is
    // shaded (trace.h wide_leaf_once); a lane whose `level` holds kExactWalk
    // confirms every candidate at once -- every lane when lvl_mode is
    // kExactWalk (MIRT_OPT_CONFIRM_ONCE 0) instead of 0
    constexpr bool DEFER = FAST && WALK == 2;
    constexpr int cstride = 256;
    // the colour stack: one row per bounce level that can store a colour
    // (levels 1 .. depth - 1), sized at launch (bounce_lds_bytes): a depth-5
    // frame needs 4 of kMaxDepth's 8 rows, and the 4 KB it leaves free per
    // workgroup is room for the co-running frames' workgroups
    extern __shared__ uint32_t cstack[];
    __shared__ uint32_t wstack[LANE4 ? kWideStack * kWideStride : 1];
    __shared__ uint32_t qsrc[LANE4 ? 4 * 16 : 1];  // quad drain: source lane of each quad, per wave
    // the tree's top levels (the first kHCache HNodes, breadth-first) in LDS:
    // every bounce walk starts there, so those steps skip the vector-memory
    // path (TD, the kernel's busiest unit)
    __shared__ uint4 hcache[LANE4 ? 4 * kHCache : 1];
    uint32_t hc_n = 0;
    if constexpr (LANE4) {
        hc_n = min((uint32_t)kHCache, sc.num_hnodes);
        const uint4* src = (const uint4*)sc.hnodes;
        for (uint32_t i = threadIdx.x; i < 4 * hc_n; i += blockDim.x) hcache[i] = src[i];
        __syncthreads();
    }
    // DEFER: the thread's index is held once, as the byte offset of its LDS
    // columns, and every later use derives from that (the compiler otherwise
    // keeps the index, its offset and its lane in a register each, and the
    // deferred kernel has exactly none to spare: 96 VGPRs, no scratch)
    uint32_t tid4 = threadIdx.x << 2;
    if (DEFER) asm volatile("" : "+v"(tid4));
    const uint32_t tid = DEFER ? tid4 >> 2 : threadIdx.x;
    uint32_t* cs = DEFER ? (uint32_t*)((char*)cstack + tid4) : cstack + threadIdx.x;
    uint32_t* stk = DEFER ? (uint32_t*)((char*)wstack + tid4) : wstack + (LANE4 ? threadIdx.x : 0);
    Counters cnt{0, 0, 0, 0, 0};
    const uint32_t n = __builtin_amdgcn_readfirstlane(qctl[0]);
    uint32_t seg = blockIdx.x % kQSeg, segs_left = kQSeg;  // wave-uniform
    bool has = false, exhausted = false;
    Ray ray{0, 0, 0, 0, 0, 0};
    SlabRay sr = bounce_slab_ray(sc, ray);
    SphRay sp = sph_ray(ray);
    Prune pr = prune_off();
    BounceWalk<WALK> w;
    if constexpr (LANE4) {
        w.hc = (lds_uint4*)hcache;
        w.hc_n = hc_n;
    }
    w.stop();
    uint32_t pixel = 0, k = 0, base0 = 0;
    int level = 0, best_s = -1;
    float best_t = INFINITY;
    for (;;) {
        // refill lanes that own no chain (one atomic per wave, tile order
        // kept), from the next segment while the current one is dry
        const uint64_t need = __ballot(!has);
        while (need && !exhausted) {
            const int leader = __builtin_ctzll(need);
            const uint32_t lo = (uint32_t)((uint64_t)n * seg / kQSeg);
            const uint32_t sz = (uint32_t)((uint64_t)n * (seg + 1) / kQSeg) - lo;
            uint32_t b = 0;
            if ((tid & 63) == leader) b = atomicAdd(&qctl[kQLine * (1 + seg)], (uint32_t)__popcll(need));
            b = __builtin_amdgcn_readlane(b, leader);
            if (b + (uint32_t)__popcll(need) >= sz) {  // this segment is dry: the next one
                seg = seg + 1 == kQSeg ? 0 : seg + 1;
                if (--segs_left == 0) exhausted = true;
            }
            if (!has) {
                const uint32_t lane0 = tid & 63;
                const uint32_t idx = b + (uint32_t)__popcll(need & ((1ull << lane0) - 1));
                if (idx < sz) {
                    const BounceRec rec = queue[lo + idx];
                    ray = Ray{rec.ox, rec.oy, rec.oz, rec.dx, rec.dy, rec.dz};
                    sr = bounce_slab_ray(sc, ray);
                    sp = sph_ray(ray);
                    pixel = rec.pixel;
                    k = rec.k;
                    base0 = rec.base0;
                    level = DEFER ? 1 | lvl_mode : 1;
                    w.start(sc);
                    best_t = INFINITY;
                    best_s = -1;
                    pr = prune_off();
                    has = true;
                }
            }
            if (b < sz) break;
        }
        if (!__ballot(has)) break;
        if (DIAG && exhausted && !dg_tx) dg_tx = __builtin_amdgcn_s_memrealtime();
        // -> quad drain (wave-uniform; DEFER: after the confirmations below,
        // where the test is made again rather than held in scalar registers
        // across the walk loop, which has none to spare)
        auto to_drain = [&]() {
            uint32_t busy = (uint32_t)__popcll(__ballot(has));
            asm volatile("" : "+s"(busy));
            return quad_drain && exhausted && busy <= 16;
        };
        bool skip_walk = false;
        if constexpr (DEFER) {
            skip_walk = to_drain();
        } else {
            if (LANE4 && quad_drain && exhausted && __popcll(__ballot(has)) <= 16) break;
        }
        // walk until few lanes are still walking and the others can make progress
        if (!skip_walk) for (;;) {
            const uint64_t walking = __ballot(has && w.walking());
            if (!walking) break;
            if (__popcll(walking) < threshold &&
                (__ballot(has && !w.walking()) || (!exhausted && __ballot(!has))))
                break;
            if (DIAG) {
                dg_it++;
                dg_lanes += __popcll(walking);
                if (exhausted) {
                    dg_it_x++;
                    dg_lanes_x += __popcll(walking);
                }
                if (has && w.walking()) dg_steps++;
            }
            if constexpr (DIAG && LANE4) {
                // lane-steps spent in a DFS-segment fallback (the lane stack
                // would have overflowed), and the fallbacks entered
                const bool seg0 = has && w.walking() && w.w.end != 0;
                gd.st_gate = gd.st_t = gd.st_box = false;
                const int lvl0 = level;
                if (has && w.walking())
                    w.template step<FAST, true, DEFER>(sc, sr, sp, pr, stk, best_t, best_s, cnt, &gd, &level);
                dg_fb_exact += (level != lvl0) ? 1u : 0u;
                dg_seg += seg0 ? 1u : 0u;
                dg_fb += (!seg0 && has && w.w.end != 0) ? 1u : 0u;
                dg_it_gate += __ballot(gd.st_gate) ? 1u : 0u;
                dg_it_t += __ballot(gd.st_t) ? 1u : 0u;
                dg_it_box += __ballot(gd.st_box) ? 1u : 0u;
            } else if constexpr (DEFER) {
                if (has && w.walking())
                    w.template step<FAST, false, true>(sc, sr, sp, pr, stk, best_t, best_s, cnt, nullptr, &level);
            } else {
                if (has && w.walking()) w.template step<FAST>(sc, sr, sp, pr, stk, best_t, best_s, cnt);
            }
        }
        // shade every lane whose ray is done: shade_level in three steps, so
        // that the wave samples the new directions together (hemisphere_wave;
        // the lanes still walking only help). (a) per lane: the level's colour,
        // and either the end of the chain (pixel folded and stored) or the hit
        // point (into the ray's origin), the normal and the pixel's RNG key
        //
        // WALK 4 (batched leaf loads, trees past the L2) keeps the per-lane
        // shade_level: it already spills at 96 VGPRs, and the wave form's
        // temporaries put three more registers into scratch (44 -> 56 B) with
        // reloads inside the walk.
        //
        // First the winner of a deferred walk against its exact box (trace.h
        // wide_leaf_once): a failure walks the level again in exact mode
        // instead of shading it. At the hand-over to the quad drain, whose
        // gates confirm every candidate at once and hold sphere indices, a
        // lane still walking confirms its tentative best here as well (what
        // it shut out loses to it) and, should that fail, walks the level
        // again from the root in the drain.
        if constexpr (DEFER) {
            const bool handover = to_drain();
            if (has && (handover || !w.walking()) && !(level & kExactWalk) && best_s >= 0) {
                best_s = confirm_leaf(sc, sr, best_s);
                // MIRT_OPT_DEBUG_FAIL_CONFIRM: a failure reported whatever the box says
                if (fail_n) {
                    uint32_t fn = (uint32_t)fail_n;
                    asm volatile("" : "+s"(fn));  // the division stays here: no reciprocal held across the walks
                    if (pixel % fn == 0) best_s = -1;
                }
                if (DIAG) {
                    dg_conf++;
                    dg_conf_fail += best_s < 0 ? 1u : 0u;
                }
                if (best_s < 0) {
                    level |= kExactWalk;
                    w.start(sc);
                    best_t = INFINITY;
                    pr = prune_off();
                }
            }
            if (handover) break;
        }
        bool go = false;  // this lane's chain goes on: it needs a direction
        float nn[3] = {0.0f, 0.0f, 0.0f};
        uint64_t key = 0;
        if constexpr (WALK == 4) {
            if (has && !w.walking()) {
                go = shade_level(sc, f, ray, best_t, best_s, level, k, chain_key(f, pixel), cs, cstride, base0, pixel,
                                 out, acc, true);
                has = go;
            }
        } else if (has && !w.walking()) {
            if (DEFER) level &= ~kExactWalk;  // this level's walk is over
            if (DIAG) {
                dg_walk_max = max(dg_walk_max, dg_steps);
                dg_chain += dg_steps;
                dg_steps = 0;
            }
            uint32_t tail = 255u << 24;  // depth exhausted: black (renderer.c:23-24)
            int stored = level - 1;
            if (best_s < 0) {
                tail = sky_rgba(ray.dy);
            } else {
                cs[(level - 1) * cstride] = sc.color[best_s];
                stored = level;
                if (level + 1 < f.depth) {  // trace_ray(bounce, depth - 1) still has depth
                    float p[3];
                    hit_point_normal(ray, best_t, sc.geo[best_s], p, nn);
                    ray.ox = p[0];
                    ray.oy = p[1];
                    ray.oz = p[2];
                    key = chain_key(f, pixel);
                    level++;
                    go = true;
                }
            }
            if (!go) {
                uint32_t c = tail;
                for (int l = stored - 1; l >= 0; l--) c = blend_rgba(cs[l * cstride], c);
                store_pixel(f, out, acc, pixel, blend_rgba(base0, c));
                has = false;
                if (DIAG) {
                    dg_chain_max = max(dg_chain_max, dg_chain);
                    dg_chain = 0;
                }
            }
        }
        // (b) the wave-uniform sampling, (c) per lane: the walk of the next level
        if (WALK != 4 && __ballot(go)) hemisphere_wave(key, k, nn, go, ray.dx, ray.dy, ray.dz, tid & 63);
        if (go) {
            sr = bounce_slab_ray(sc, ray);
            sp = sph_ray(ray);
            w.start(sc);
            best_t = INFINITY;
            best_s = -1;
            pr = prune_off();
            if (DEFER) level |= lvl_mode;
        }
    }
    if constexpr (DEFER) level &= ~kExactWalk;  // the drain's walks are all exact
    if constexpr (LANE4) {
        // quad drain (uniform control flow here: every lane is active)
        const uint64_t busy = __ballot(has);
        if (busy) {
            const uint32_t lane = tid & 63, wv = tid >> 6;
            if (has) qsrc[wv * 16 + lanes_below(busy)] = lane;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t q = lane >> 2;
            const bool qhas = q < (uint32_t)__popcll(busy);
            const uint32_t src = qsrc[wv * 16 + (qhas ? q : 0)];
            auto pull = [&](uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v); };
            auto pullf = [&](float v) { return __uint_as_float(pull(__float_as_uint(v))); };
            ray = Ray{pullf(ray.ox), pullf(ray.oy), pullf(ray.oz), pullf(ray.dx), pullf(ray.dy), pullf(ray.dz)};
            pixel = pull(pixel);
            k = pull(k);
            level = (int)pull((uint32_t)level);
            base0 = pull(base0);
            best_t = pullf(best_t);
            best_s = (int)pull((uint32_t)best_s);
            pr = Prune{pullf(pr.m), pullf(pr.lim)};
            const WideWalk& lw = w.w;
            QuadWalk qw{pull(lw.cur), pull(lw.end), pull(lw.top)};
            has = qhas;
            if (!qhas) qw.cur = kPNone;
            sr = bounce_slab_ray(sc, ray);
            sp = sph_ray(ray);
            // the ray's LDS stacks stay in its source lane's columns
            uint32_t* qstk = wstack + (tid & ~63u) + src;
            uint32_t* qcs = cstack + (tid & ~63u) + src;
            if (DIAG) dg_tq = __builtin_amdgcn_s_memrealtime();
            while (__ballot(has)) {
                if (DIAG) dg_qit++;
                if (!DIAG) {
                    // one ray left in the wave: every quad of the wave walks it
                    const uint64_t rays = __ballot(has && (lane & 3) == 0);
                    if (__popcll(rays) == 1) {
                        solo_chain<FAST, kBoundedSlab && WALK != 4>(sc, f, __builtin_ctzll(rays), ray, best_t, best_s, pr,
                                                                    qw, level, k, pixel,
                                         base0, src, wstack + (tid & ~63u), cstack + (tid & ~63u),
                                         out, acc, (lds_uint4*)hcache, hc_n, lane);
                        break;
                    }
                }
                if (has && qw.cur != kPNone)
                    quad_step<FAST, kWideStride, kWideStack, kBoundedSlab && WALK != 4>(sc, sr, sp, pr, qw, qstk, best_t,
                                                                                        best_s,
                                                             (lds_uint4*)hcache, hc_n, lane);
                if (has && qw.cur == kPNone) {
                    if (shade_level(sc, f, ray, best_t, best_s, level, k, chain_key(f, pixel), qcs, kWideStride, base0, pixel, out,
                                    acc, (lane & 3) == 0)) {
                        sr = bounce_slab_ray(sc, ray);
                        sp = sph_ray(ray);
                        qw = QuadWalk{sc.wide_root, 0u, 0u};
                        best_t = INFINITY;
                        best_s = -1;
                        pr = prune_off();
                    } else {
                        has = false;
                    }
                }
            }
        }
    }
    if (DIAG) {
        for (int o = 32; o; o >>= 1) {
            dg_walk_max = max(dg_walk_max, (uint32_t)__shfl_xor((int)dg_walk_max, o));
            dg_chain_max = max(dg_chain_max, (uint32_t)__shfl_xor((int)dg_chain_max, o));
        }
        if ((tid & 63) == 0) {
            uint64_t* d = diag + kBounceDiag * (blockIdx.x * (blockDim.x >> 6) + (tid >> 6));
            d[0] = dg_it;
            d[1] = dg_lanes;
            d[2] = dg_it_x;
            d[3] = dg_lanes_x;
            d[4] = dg_t0;
            d[5] = dg_tx;
            d[6] = __builtin_amdgcn_s_memrealtime();
            d[7] = ((uint64_t)dg_chain_max << 32) | dg_walk_max;
            d[8] = dg_qit;
            d[9] = dg_tq;
        }
        // per-lane sums reduced over the wave
        for (int o = 32; o; o >>= 1) {
            dg_seg += (uint64_t)__shfl_xor((long long)dg_seg, o);
            dg_fb += (uint64_t)__shfl_xor((long long)dg_fb, o);
            gd.gates += (uint32_t)__shfl_xor((int)gd.gates, o);
            gd.gates_t += (uint32_t)__shfl_xor((int)gd.gates_t, o);
            gd.gates_box += (uint32_t)__shfl_xor((int)gd.gates_box, o);
            gd.lanes_t += (uint32_t)__shfl_xor((int)gd.lanes_t, o);
            gd.lanes_box += (uint32_t)__shfl_xor((int)gd.lanes_box, o);
            dg_conf += (uint32_t)__shfl_xor((int)dg_conf, o);
            dg_conf_fail += (uint32_t)__shfl_xor((int)dg_conf_fail, o);
            dg_fb_exact += (uint32_t)__shfl_xor((int)dg_fb_exact, o);
        }
        if ((tid & 63) == 0) {
            uint64_t* d = diag + kBounceDiag * (blockIdx.x * (blockDim.x >> 6) + (tid >> 6));
            d[10] = dg_seg;
            d[11] = dg_fb;
            d[12] = gd.gates;
            d[13] = gd.gates_t;
            d[14] = gd.lanes_t;
            d[15] = gd.gates_box;
            d[16] = gd.lanes_box;
            d[17] = dg_it_gate;
            d[18] = dg_it_t;
            d[19] = dg_it_box;
            d[20] = dg_conf;
            d[21] = dg_conf_fail;
            d[22] = dg_fb_exact;
        }
    }
}

// trace_ray on explicit rays (renderer.c:21); ray i uses contract pixel i.
template <bool FAST>
__global__ __launch_bounds__(256) void trace_rays_kernel(DevScene sc, const mirt_ray* __restrict__ rays, int n,
                                                         int depth, int use_bvh, uint64_t seed, uint32_t sample,
                                                         uint32_t pixel0, uint32_t* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = i < n;
    const mirt_ray& rr = rays[alive ? i : 0];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    Counters cnt{0, 0, 0, 0, 0};
    __shared__ uint32_t cstack[kMaxDepth * 256];
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    const uint32_t c = trace_path<FAST, false>(sc, ray, alive, depth, use_bvh != 0,
                                                  pixel_key(seed, pixel0 + (uint32_t)i, sample), cnt, cstack + threadIdx.x, 256,
                                                  wstack + threadIdx.x);
    if (alive) out[i] = c;
}

__device__ __forceinline__ void store_hit(const Ray& ray, float t, int s, const DevScene& sc, mirt_hit* o)
{
    mirt_hit h;
    memset(&h, 0, sizeof h);
    h.sphere = -1;
    if (s >= 0) {
        float p[3], nn[3];
        hit_point_normal(ray, t, sc.geo[s], p, nn);
        h.t = t;
        h.point = {p[0], p[1], p[2]};
        h.normal = {nn[0], nn[1], nn[2]};
        h.hit = 1;
        h.sphere = s;
    }
    *o = h;
}

// Brute force (renderer.c:36-43, benchmark.c:190-199) split over sphere
// chunks so that a few thousand rays still fill the chip: workgroup (bx, by)
// runs rays [256 bx, 256 bx + 256) against spheres [chunk by, chunk (by + 1)),
// every lane reading the same sphere (scalar loads, one fetch per wave).
// The chunk's best (t, index) joins keys[ray] by a 64-bit atomicMin of
// (bits(t) << 32 | index) -- t > 0 orders as its bit pattern, and on equal t
// the smaller index (the first sphere in array order) wins, as the loop's
// strict `<` does. Any-hit flags are keys != ~0: every sphere is still
// tested, as benchmark.c:190-199 does (an early exit measured slower: the
// per-sphere vote costs more than the rare hit saves).
template <bool FAST>
__global__ __launch_bounds__(256) void brute_chunk_kernel(DevScene sc, const mirt_ray* __restrict__ rays, int n,
                                                          int chunk, unsigned long long* __restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = i < n;
    const mirt_ray& rr = rays[active ? i : 0];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const SphRay sp = sph_ray(ray);
    const int s0 = (int)blockIdx.y * chunk;
    const int s1 = min(s0 + chunk, sc.num_spheres);
    float best_t = INFINITY;
    int best_s = -1;
    if (FAST && s0 < s1 && __ballot(active)) {
        brute_range_packed(sc, sp, active, s0, s1, best_t, best_s);
    } else if (s0 < s1 && __ballot(active)) {
        float4 g = load_geo_uniform(sc.geo, s0);
        for (int k = s0; k < s1; k++) {
            const float4 gn = load_geo_uniform(sc.geo, k + 1);  // [num_spheres] is the sentinel: in bounds
            if (active) {
                const float t = sphere_t<FAST>(sp, g, best_t);
                if (t > 0.0f && t < best_t) {
                    best_t = t;
                    best_s = k;
                }
            }
            g = gn;
        }
    }
    if (best_s >= 0) atomicMin(&keys[i], ((unsigned long long)__float_as_uint(best_t) << 32) | (unsigned)best_s);
}

// The hit records of brute_chunk_kernel (hit.c:32-33 for the winner).
__global__ __launch_bounds__(256) void brute_finish_kernel(DevScene sc, const mirt_ray* __restrict__ rays, int n,
                                                           const unsigned long long* __restrict__ keys,
                                                           mirt_hit* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mirt_ray& rr = rays[i];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const unsigned long long k = keys[i];
    const bool hit = k != ~0ull;
    store_hit(ray, hit ? __uint_as_float((uint32_t)(k >> 32)) : INFINITY, hit ? (int)(uint32_t)k : -1, sc, &out[i]);
}

// ray_bvh_intersect(...).hit_something per ray (benchmark.c:239-241).
template <bool FAST>
__global__ __launch_bounds__(256) void bvh_any_kernel(DevScene sc, const mirt_ray* __restrict__ rays, int n,
                                                      int32_t* __restrict__ out)
{
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = i < n;
    const mirt_ray& rr = rays[alive ? i : 0];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    Counters cnt{0, 0, 0, 0, 0};
    float t;
    int s;
    closest_hit<false, FAST, false>(sc, ray, alive, t, s, cnt, wstack + threadIdx.x);
    if (alive) out[i] = s >= 0 ? 1 : 0;
}

__global__ void keys_to_flags_kernel(const unsigned long long* __restrict__ keys, int n, int32_t* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = keys[i] != ~0ull ? 1 : 0;
}

// ray_bvh_intersect (hit.c:91) / brute-force closest hit (renderer.c:36-43)
template <bool FAST>
__global__ __launch_bounds__(256) void intersect_kernel(DevScene sc, const mirt_ray* __restrict__ rays, int n,
                                                        int use_bvh, mirt_hit* __restrict__ out)
{
    __shared__ uint32_t wstack[kWideStack * kWideStride];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = i < n;
    const mirt_ray& rr = rays[alive ? i : 0];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    Counters cnt{0, 0, 0, 0, 0};
    float t;
    int s;
    // arbitrary rays are incoherent: per-lane walks (four-wide where the
    // tree admits it, each lane with its LDS stack column), not packets
    if (use_bvh)
        closest_hit<false, FAST, false>(sc, ray, alive, t, s, cnt, wstack + threadIdx.x);
    else
        closest_brute<FAST, false>(sc, ray, alive, t, s, cnt);
    if (alive) store_hit(ray, t, s, sc, &out[i]);
}

// ray_bvh_intersect (hit.c:91-109) for a batch too small to fill the chip
// one ray per lane (benchmark.c's 10,000 rays): one ray per QUAD of lanes,
// lane j testing slot j of every four-wide node (quad_step, the bounce
// kernel's drain walk), so each ray's dependent chain of node fetches is
// walked by four lanes and the batch occupies four times the lanes. The
// tree's top HNodes are staged in LDS; rays with a zero/tiny direction
// component take the exact wave-cooperative walk afterwards (closest_hit).
// ANY: the hit flag (benchmark.c:239-241), else the hit record.
constexpr int kQuadBatchThreads = 64;  // 16 rays per workgroup: a small batch spreads over the CUs
template <bool ANY>
__global__ __launch_bounds__(kQuadBatchThreads) void intersect_quad_kernel(DevScene sc, const mirt_ray* __restrict__ rays,
                                                                          int n, mirt_hit* __restrict__ out,
                                                                          int32_t* __restrict__ flags)
{
    constexpr int kRays = kQuadBatchThreads / 4;
    __shared__ uint32_t qstack[kWideStack * kRays];
    __shared__ uint4 hcache[4 * kHCache];
    const uint32_t hc_n = min((uint32_t)kHCache, sc.num_hnodes);
    for (uint32_t i = threadIdx.x; i < 4 * hc_n; i += blockDim.x) hcache[i] = ((const uint4*)sc.hnodes)[i];
    __syncthreads();
    const int q = (int)(threadIdx.x >> 2);
    const int i = (int)blockIdx.x * kRays + q;
    const bool alive = i < n;
    const mirt_ray& rr = rays[alive ? i : 0];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const SlabRay sr = slab_ray(ray);
    const SphRay sp = sph_ray(ray);
    Prune pr = prune_off();
    const bool gen = alive && sr.generic;
    float best_t = INFINITY;
    int best_s = -1;
    QuadWalk qw{alive && !gen ? sc.wide_root : kPNone, 0u, 0u};
    while (__ballot(qw.cur != kPNone)) {
        if (qw.cur != kPNone)
            quad_step<true, kRays, kWideStack>(sc, sr, sp, pr, qw, qstack + q, best_t, best_s, (lds_uint4*)hcache, hc_n);
    }
    uint64_t gm = __ballot(gen && (threadIdx.x & 3) == 0);
    while (gm) {  // zero-component rays: the exact chunked walk, one ray per wave pass
        const int l = __builtin_ctzll(gm);
        gm &= gm - 1;
        const Ray g{readlane_f(ray.ox, l), readlane_f(ray.oy, l), readlane_f(ray.oz, l),
                    readlane_f(ray.dx, l), readlane_f(ray.dy, l), readlane_f(ray.dz, l)};
        float t;
        int s2;
        Counters c2{0, 0, 0, 0, 0};
        closest_bvh_chunked<true, false>(sc, g, t, s2, c2);
        if ((int)(threadIdx.x & 63) >> 2 == l >> 2) {
            best_t = t;
            best_s = s2;
        }
    }
    if (alive && (threadIdx.x & 3) == 0) {
        if (ANY)
            flags[i] = best_s >= 0 ? 1 : 0;
        else
            store_hit(ray, best_t, best_s, sc, &out[i]);
    }
}

// element-wise ray_sphere_intersect (hit.c:19-39)
__global__ void sphere_pairs_kernel(const mirt_ray* __restrict__ rays, const mirt_sphere* __restrict__ sph, int n,
                                    mirt_hit* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mirt_ray rr = rays[i];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const float4 g = make_float4(sph[i].center.x, sph[i].center.y, sph[i].center.z, sph[i].radius);
    const float t = sphere_t<false>(sph_ray(ray), g, INFINITY);
    mirt_hit h;
    memset(&h, 0, sizeof h);
    h.sphere = -1;
    if (t > 0.0f) {
        float p[3], nn[3];
        hit_point_normal(ray, t, g, p, nn);
        h.t = t;
        h.point = {p[0], p[1], p[2]};
        h.normal = {nn[0], nn[1], nn[2]};
        h.hit = 1;
        h.sphere = i;
    }
    out[i] = h;
}

// element-wise ray_aabb_intersect (hit.c:49-82)
__global__ void aabb_pairs_kernel(const mirt_ray* __restrict__ rays, const mirt_aabb* __restrict__ boxes, int n,
                                  int32_t* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mirt_ray rr = rays[i];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const mirt_aabb b = boxes[i];
    out[i] = slab_test(slab_ray(ray), b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z) ? 1 : 0;
}

// hemisphere_wave on caller-given lanes (mirt_hemisphere_probe): the grid
// covers the lanes exactly, so every wave is whole and calls it uniformly.
__global__ void hemisphere_probe_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ k0,
                                        const float* __restrict__ normals, const int32_t* __restrict__ need,
                                        float* __restrict__ dir, uint32_t* __restrict__ kout)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float n[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    float x = dir[3 * i], y = dir[3 * i + 1], z = dir[3 * i + 2];
    uint32_t k = k0[i];
    hemisphere_wave(keys[i], k, n, need[i] != 0, x, y, z);
    dir[3 * i] = x;
    dir[3 * i + 1] = y;
    dir[3 * i + 2] = z;
    kout[i] = k;
}

// The walks' filtered box tests on pairs (mirt_box_form_pairs): the Prune
// state a walk holds with a best hit at best[i] (none yet: +inf), then the
// call the walk makes for that kind of box.
__global__ void box_form_pairs_kernel(DevScene sc, const mirt_ray* __restrict__ rays,
                                      const mirt_aabb* __restrict__ boxes, const float* __restrict__ best, int n,
                                      int form, int32_t* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mirt_ray rr = rays[i];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const mirt_aabb b = boxes[i];
    const float bt = best[i];
    Prune pr = prune_start(sc, ray.ox, ray.oy, ray.oz);
    if (sc.prune && bt < INFINITY) prune_update(pr, sc, ray.ox, ray.oy, ray.oz, sph_ray(ray).a4(), bt);
    SlabRay sr = slab_ray(ray);
    float near = 0.0f;
    bool pass = false;
    switch (form) {
    case MIRT_BOX_FORM_SLAB: {
        NodeV nd;
        nd.b0 = b.min.x; nd.b1 = b.min.y; nd.b2 = b.min.z; nd.b3 = b.max.x; nd.b4 = b.max.y; nd.b5 = b.max.z;
        nd.sphere = -1;
        nd.skip = 0;
        nd.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        pass = slab<true>(sr, pr, nd);
        break;
    }
    case MIRT_BOX_FORM_SLAB_BOX:
        pass = slab_box<true>(sr, pr, b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z, near);
        break;
    case MIRT_BOX_FORM_CONS:
        pass = slab_cons<false>(sr, pr, b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z, near);
        break;
    case MIRT_BOX_FORM_CONS_BOUNCE:
        sr = bounce_slab_ray(sc, ray);
        pass = slab_cons<true>(sr, pr, b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z, near);
        break;
    default:  // MIRT_BOX_FORM_CONS_CAMERA
        sr.generic = sr.generic ||
                     !origin_within_4c(sc.o_bound, fmaxf(fabsf(ray.ox), fmaxf(fabsf(ray.oy), fabsf(ray.oz))));
        pass = slab_cons<true>(sr, pr, b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z, near);
        break;
    }
    out[i] = pass ? 1 : 0;
}

// sphere_t on pairs (mirt_sphere_form_pairs): the returned float's bits.
// MODE 0: the exact form; 1: the filtered form of the walks; 2: the filtered
// form with the float-pair certification off (every pair the filter leaves
// takes the f64 branch, which the walks reach once in some thousands of hits);
// 3: not t but whether MODE 1 ran the f64 branch for the pair.
template <int MODE>
__global__ void sphere_form_pairs_kernel(const mirt_ray* __restrict__ rays, const mirt_sphere* __restrict__ sph,
                                         const float* __restrict__ best, int n, uint32_t* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mirt_ray rr = rays[i];
    const Ray ray{rr.origin.x, rr.origin.y, rr.origin.z, rr.direction.x, rr.direction.y, rr.direction.z};
    const float4 g = make_float4(sph[i].center.x, sph[i].center.y, sph[i].center.z, sph[i].radius);
    if constexpr (MODE == 3) {
        bool f64 = false;
        (void)sphere_t<true>(sph_ray(ray), g, best[i], &f64);
        out[i] = f64 ? 1u : 0u;
    } else {
        out[i] = __float_as_uint(sphere_t<MODE != 0, MODE != 2>(sph_ray(ray), g, best[i]));
    }
}

// normalize3's binary32 root (sqrt_rn32) against vec3.c:22's binary64 form on
// every non-negative finite float (mirt_sqrt_form_sweep): res[0] = mismatches,
// res[1] = the least mismatching bit pattern (~0: none).
__global__ void sqrt_form_sweep_kernel(unsigned long long* __restrict__ res)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t bad = 0, first = ~0u;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < 0x7f800000ull; i += stride) {
        const float x = __uint_as_float((uint32_t)i);
        if (__float_as_uint(sqrt_rn32(x)) != __float_as_uint((float)__dsqrt_rn((double)x))) {
            bad++;
            first = min(first, (uint32_t)i);
        }
    }
    if (bad) {
        atomicAdd(&res[0], (unsigned long long)bad);
        atomicMin(&res[1], (unsigned long long)first);
    }
}

__global__ void camera_rays_kernel(FrameConst f, mirt_ray* __restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= f.width || r >= f.num_rows) return;
    const Ray ray = camera_ray(f, x, shard_row_to_y(f, r), row_sample(f, r));
    out[(size_t)r * f.width + x] = {{ray.ox, ray.oy, ray.oz}, {ray.dx, ray.dy, ray.dz}};
}

// get_camera_ray (ray.c:17-32) at caller-given (u, v): the batched form of
// the per-ray call, for callers that build their own pixel loop.
__global__ void camera_uv_kernel(FrameConst f, const float2* __restrict__ uv, int n, mirt_ray* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float u = uv[i].x, v = uv[i].y;
    float dx = f.fx + f.hx * u, dy = f.fy + f.hy * u, dz = f.fz + f.hz * u;
    dx = dx + f.vx * v;
    dy = dy + f.vy * v;
    dz = dz + f.vz * v;
    normalize3(dx, dy, dz);
    out[i] = {{f.px, f.py, f.pz}, {dx, dy, dz}};
}

// ---------------------------------------------------------------- BVH overlay
// The debug view of bvh_visualiser.c:16-126 ('o' in main.c:323-327): every
// node's box (pre-order, bvh_visualiser.c:110-116) as 12 projected edges
// (draw_aabb :71-99), each drawn 5 times offset by one pixel (draw_debug_line
// :45-68), coloured by depth (:107-110) over a cleared black screen. Later
// lines overwrite earlier ones, so a pixel shows the LAST line (in draw
// order) that covers it: pass 1 rasterises every line and keeps the largest
// draw index per pixel (atomicMax), pass 2 colours. Rasterisation (SDL's
// depends on the backend; the reference marks the view "NOT WORKING") is the
// build's definition: Bresenham over integer endpoints, both inclusive,
// pixels off screen skipped.
struct OverlayConst {
    float px, py, pz, fx, fy, fz, rx, ry, rz, ux, uy, uz;
    float half_w, half_h;  // host: tanf (glibc) as bvh_visualiser.c:27-30
    int width, height, max_levels;
};

// (int)x of x86 (cvttss2si): NaN and out-of-range values give INT_MIN.
__device__ __forceinline__ int x86_trunc(float x)
{
    return (x > -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN;
}

// world_to_screen, bvh_visualiser.c:16-41 (float arithmetic, no contraction)
__device__ __forceinline__ int2 world_to_screen(const OverlayConst& o, float x, float y, float z)
{
    const float tx = x - o.px, ty = y - o.py, tz = z - o.pz;
    const float zz = tx * o.fx + ty * o.fy + tz * o.fz;
    if (zz <= 0.1f) return make_int2(-1, -1);
    const float xx = tx * o.rx + ty * o.ry + tz * o.rz;
    const float yy = tx * o.ux + ty * o.uy + tz * o.uz;
    const float sx = (xx / (zz * o.half_w * 2.0f) + 0.5f) * (float)o.width;
    const float sy = (-yy / (zz * o.half_h * 2.0f) + 0.5f) * (float)o.height;
    if (sx < (float)-o.width || sx > (float)(o.width * 2) || sy < (float)-o.height || sy > (float)(o.height * 2))
        return make_int2(-1, -1);
    return make_int2(x86_trunc(sx), x86_trunc(sy));
}

__constant__ int kBoxEdge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6},
                                    {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
__constant__ int kLineOffset[5][2] = {{0, 0}, {1, 0}, {0, 1}, {-1, 0}, {0, -1}};

// A node's depth. The resident byte (MIRT_LAYOUT_NDEPTH) is exact below 255
// and clamped there; a node that carries 255 finds its depth by the descent
// from the root: the left child of inner node j is j + 1, the right one the
// left one's skip, and `node` lies in the right subtree iff it is not before
// it. cur only grows and stays <= node (an upload validates skip > index and
// the nesting), so the walk ends after depth steps -- on trees deeper than 254
// only.
__device__ __forceinline__ uint32_t overlay_depth(const mirt_node* __restrict__ nodes,
                                                  const uint8_t* __restrict__ ndepth, uint32_t node)
{
    uint32_t d = ndepth[node];
    if (d < 255) return d;
    d = 0;
    for (uint32_t cur = 0; cur < node; d++) {
        const uint32_t right = nodes[cur + 1].skip & MIRT_SKIP_MASK;
        cur = node >= right ? right : cur + 1;
    }
    return d;
}

// one thread per (node, edge, offset): draw index (node * 12 + edge) * 5 + offset
__global__ void overlay_lines_kernel(OverlayConst o, const mirt_node* __restrict__ nodes,
                                     const uint8_t* __restrict__ ndepth, uint32_t count, uint32_t* __restrict__ last)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= count) return;
    const uint32_t node = id / 60, edge = (id / 5) % 12, off = id % 5;
    if (o.max_levels >= 0) {  // (the byte decides every level up to 255: the descent only past it)
        const uint32_t d = o.max_levels > 255 ? overlay_depth(nodes, ndepth, node) : ndepth[node];
        if (d >= (uint32_t)o.max_levels) return;
    }
    const mirt_node nd = nodes[node];
    auto corner = [&](int k) {  // draw_aabb's corner order (:73-82)
        const int hx = (k == 1 || k == 2 || k == 5 || k == 6), hy = (k == 2 || k == 3 || k == 6 || k == 7), hz = k >= 4;
        return world_to_screen(o, hx ? nd.bmax[0] : nd.bmin[0], hy ? nd.bmax[1] : nd.bmin[1],
                               hz ? nd.bmax[2] : nd.bmin[2]);
    };
    const int2 a = corner(kBoxEdge[edge][0]), b = corner(kBoxEdge[edge][1]);
    if (a.x == -1 || b.x == -1) return;  // :49 (tests x only)
    const int W = o.width, H = o.height;
    if (!(a.x >= -W && a.x <= W * 2 && a.y >= -H && a.y <= H * 2 && b.x >= -W && b.x <= W * 2 && b.y >= -H &&
          b.y <= H * 2))
        return;  // :51-54
    int x0 = a.x + kLineOffset[off][0], y0 = a.y + kLineOffset[off][1];
    const int x1 = b.x + kLineOffset[off][0], y1 = b.y + kLineOffset[off][1];
    const uint32_t tag = id + 1;
    const int dx = abs(x1 - x0), dy = -abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    int err = dx + dy;
    for (;;) {
        if (x0 >= 0 && x0 < W && y0 >= 0 && y0 < H) atomicMax(&last[(size_t)y0 * W + x0], tag);
        if (x0 == x1 && y0 == y1) break;
        const int e2 = 2 * err;
        if (e2 >= dy) {
            err += dy;
            x0 += sx;
        }
        if (e2 <= dx) {
            err += dx;
            y0 += sy;
        }
    }
}

__global__ void overlay_colour_kernel(const uint32_t* __restrict__ last, const mirt_node* __restrict__ nodes,
                                      const uint8_t* __restrict__ ndepth, size_t n, uint32_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = last[i];
    uint32_t c = 0xff000000u;  // SDL_RenderClear with (0, 0, 0, 255), main.c:342-343
    if (v) {
        const uint32_t d = overlay_depth(nodes, ndepth, (v - 1) / 60);
        const uint32_t r = 255 - (d * 40) % 200, g = (d * 80) % 200, b = (d * 120) % 200;  // :107-110
        c = r | g << 8 | b << 16 | 180u << 24;
    }
    out[i] = c;
}

}  // namespace

// ------------------------------------------------------------------ context

constexpr int kPhaseRing = 64;  // frames of pass timings kept per ctx (mirt_phase_log)

// The float accumulation buffer of main.c:241-273 (x-major there, row-major
// float3 here). One per ctx by default; mirt_ctx_share_accum lets the ctxs
// that keep frames of one display loop in flight (main.c:379-408, one ctx
// per hardware queue) use ONE buffer: every frame's colours then go to its
// own slab and a fold kernel adds them to the buffer, the folds of
// successive calls ordered across the ctxs' streams by `folded` (the event
// of the last fold enqueued, on whichever stream) -- the tracing overlaps,
// only the folds (a few microseconds each) run in call order.
struct AccumShare {
    int refs = 1;
    int device = 0;
    float* d_acc = nullptr;
    size_t cap = 0;          // bytes allocated
    size_t pixels = 0;       // pixels of the running accumulation (0: none yet)
    hipEvent_t folded = nullptr;
    bool has_fold = false;   // `folded` was recorded at least once
    // Lazy fold (round 5): the display slab of the last FRESH
    // frame issued on the share and not yet folded into d_acc. A fresh
    // frame's accumulation state is its colours / 255 (main.c:368-370), which
    // its slab holds exactly, so it is folded only when a frame or a read
    // needs d_acc (accum_materialize) -- fresh frames in flight no longer wait
    // for each other's folds, and a fresh frame superseded by a later one is
    // never folded at all.
    const uint32_t* pend = nullptr;
    mirt_ctx* pend_ctx = nullptr;   // the ctx that rendered it (its slab must outlive the read)
    hipEvent_t pend_ev = nullptr;   // recorded after that frame's render
};
// (A launch of several fresh frames, mirt_multi at N >= 4, keeps its ordered
// fold: the lanes then finish in the order the caller rotates through them;
// its last display left pending ran the slowest shard of an 8-way split 2-4%
// slower, profiles/r05_logs/r05bc/.)



// One resident scene: the nine device arrays and the scalars that go with
// them. Immutable once installed; freed only when no slot holds it and every
// stream that may still read it has passed the events in `readers`.
struct Scene {
    int refs = 0;               // slots that hold it
    uint64_t id = 0;            // mirt_ctx_scene_id: stamped at install, process-wide
    DNode* d_nodes = nullptr;
    mirt_node* d_nodes32 = nullptr;
    float4* d_geo = nullptr;
    uint32_t* d_color = nullptr;
    int num_nodes = 0, num_spheres = -1;
    bool prune_ok = false;      // the uploaded tree's boxes enclose their subtrees
    PNode* d_pnodes = nullptr;  // ordered-walk layout of the tree
    bool ordered_ok = false;    // leaves in DFS order hold increasing sphere indices, depth < 63
    HNode* d_hnodes = nullptr;  // four-wide layout (per-lane walks)
    HAux* d_haux = nullptr;
    char* d_leaves = nullptr;   // leaf spheres (float4 each), then at leaf_box_off the leaf boxes (LeafBox each)
    size_t leaf_box_off = 0;
    uint32_t num_hnodes = 0;
    uint32_t num_pnodes = 0, num_leaves = 0;  // read back by mirt_scene_resident_layout
    uint32_t wide_root = 0;     // HNode a four-wide walk starts at (DevScene::wide_root)
    uint8_t* d_ndepth = nullptr;  // depth of every flat node (BVH overlay colours)
    float r_max = 0.0f, c_max = 0.0f;
    float o_bound = 0.0f;       // the bounce walks' origin bound the HNode boxes were grown for
    bool leaf_big = false;      // the four-wide tree (HNodes + leaves) exceeds the chip's L2
    // one event per member stream of every slot that gave the scene up,
    // recorded behind the frames that slot's members had enqueued on it
    std::vector<hipEvent_t> readers;
};

// The scene slot of a ctx: one per ctx by default;
// mirt_ctx_share_scene lets the ctxs of one device render ONE resident scene.
// An install through any member replaces `cur` for all of them; the replaced
// scene waits in `retired` until its readers' events have passed (checked at
// the slot's later installs, waited for when the slot itself goes).
// The link of a scene slot (MIRT_OPT_HISTORY_MOTION): what a
// history of the scene `from` needs to be carried to the scene `to` that a
// refit or an update installed over it. One allocation of two halves, each
// [Geo4 x n: the replaced scene's geo][int32 x n: the rebuild's permutation];
// an install stages into the half that is not the link and the commit flips,
// so a failed install leaves the link as it was. The allocation only grows
// and goes with the slot: no hipFree per install (MEASUREMENTS.md E).
// No event: the only reader is mirt_render_frame_reprojected, a blocking call
// that has waited for its kernel when it returns, and the only writers are
// installs, blocking calls too that wait for their copies before they return
// -- all of them made by the group's one host thread, so a write never meets
// a read in flight, whichever member's stream either ran on.
struct HistoryLink {
    void* d = nullptr;
    size_t cap = 0;             // of both halves together
    int half = 0;               // the half the link reads
    bool valid = false;
    uint64_t from = 0, to = 0;
    int n = 0;                  // spheres of `from` (and of `to`: refits and updates keep the count)
    bool rebuilt = false;       // the half holds a permutation
    bool staged = false;        // the other half holds the install in progress: staged_from, staged_n, staged_rebuilt
    uint64_t staged_from = 0;
    int staged_n = 0;
    bool staged_rebuilt = false;
    char* base(int h) const { return (char*)d + (size_t)h * (cap / 2); }
    const float* geo_prev(int h) const { return (const float*)base(h); }
    const int32_t* perm(int h) const { return (const int32_t*)(base(h) + sizeof(float4) * (size_t)n); }
};

struct SceneSlot {
    Scene* cur = nullptr;
    std::vector<mirt_ctx*> members;
    std::vector<Scene*> retired;
    double base_cost = 0.0;     // mirt_scene_update_device: the cost of the tree it last installed
    bool have_base_cost = false;  // dropped by every install of a scene
    HistoryLink link;           // set by a refit / update of an option-1 ctx, cleared by every other install
};

// What the camera rays of a frame and its pixel -> row map are computed from:
// the FrameConst fields camera_ray and shard_row_to_y read (jitter aside: a
// jittered frame never meets the cache), and the identity of the scene.
// Compared bitwise, so -0.0 and +0.0 differ: a miss, the safe side.
struct PrimaryKey {
    float cam[12];               // px .. vz
    float aspect, wf, hf;
    int width, height, row_block, shard, num_shards, lead_skip, shard_rows;
    uint64_t scene_id;           // mirt_ctx_scene_id at enqueue
};

// The primary cache of a ctx (MIRT_OPT_PRIMARY_CACHE): one slab of
// (t, sphere), t first, in one allocation that only ever grows.
// No events of its own: frames of one ctx never overlap -- a launch on another
// stream than the previous one first waits for `done` (launch_render) -- so a
// fill's stores, a hit's loads and the next fill's stores are ordered as the
// frames are, whichever streams they run on.
struct PrimaryCache {
    int on = 0;
    void* d = nullptr;
    size_t cap = 0;
    bool valid = false;          // d holds the hits of `key`
    PrimaryKey key{};
    mirt_camera cam{};           // the caller's camera of the key: tells CAMERA from GEOMETRY (reason only)
    uint64_t hits = 0, fills = 0, bypassed = 0;
    int last = MIRT_PCACHE_BYPASS, reason = MIRT_PCACHE_OFF;
    size_t pixels() const { return (size_t)key.shard_rows * key.width; }
};

// The primary scan of a ctx (MIRT_OPT_PRIMARY_SCAN): the
// per-camera data of `key` (pscan.hip) and the per-frame slab, walk list and
// counters, carved from one allocation that only ever grows (the rule of
// d_planes: grown after waiting for the ctx's frames, never while they are in
// flight). No events of its own, as the primary cache: frames of one ctx never
// overlap.
struct PrimaryScan {
    int opt = 2;                 // 0 off, 1 on, 2 automatic
    int budget = 256;            // MIRT_OPT_PRIMARY_SCAN_BUDGET: chunks of 64 records a tile with a sky pixel reads before it takes the walk
    int always_rebuild = 0;      // MIRT_OPT_PRIMARY_SCAN_REBUILD: measurement hook, the per-camera data rebuilt every frame
    void* d = nullptr;
    size_t cap = 0;
    bool valid = false;          // the per-camera data are those of `key`
    PrimaryKey key{};
    PscanCam cam{};
    PscanBuild b{};
    uint32_t nl = 0;
    size_t sort_bytes = 0;       // pscan_sort_bytes(sort_nl)
    uint32_t sort_nl = ~0u;
    float* t = nullptr;
    int32_t* sphere = nullptr;
    uint32_t* wlist = nullptr;
    unsigned long long* stats = nullptr;
    // automatic mode: the id of the scene pscan_verdict_kernel found sparse (0: none), in page-locked host memory
    // the device writes and ps_classify reads without a wait; d_verdict is its device address
    unsigned long long* h_verdict = nullptr;
    unsigned long long* d_verdict = nullptr;
    uint64_t scanned = 0, bypassed = 0, rebuilds = 0;
    int last = MIRT_PSCAN_BYPASS, reason = MIRT_PSCAN_NONE;
};

struct mirt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed_recorded = false;  // ev0/ev1 bracket a launch (mirt_last_kernel_ms)
    float last_ms = 0.0f;
    // wavefront phase boundaries of the last frame (any API)
    // (a ring of kPhaseRing frames: mirt_phase_log reads back the passes of
    // frames that ran overlapped with other ctxs' frames, without a sync
    // between them)
    hipEvent_t ph0[kPhaseRing] = {}, ph1[kPhaseRing] = {}, ph2[kPhaseRing] = {};
    uint32_t ph_next = 0;   // ring slot of the next wavefront frame
    uint32_t ph_count = 0;  // wavefront frames recorded (saturates at kPhaseRing)
    bool phases_valid = false;
    // the frame scratch (queue, deferral list, phase events) is per ctx: a
    // launch on another stream than the previous one waits for it
    hipEvent_t done = nullptr;
    // Lazy fold: another stream read this ctx's display slab for the
    // share's pending fold; the ctx's next write to it waits for `slab_free`
    hipEvent_t slab_free = nullptr;
    bool slab_guard = false;
    hipStream_t last_stream = nullptr;
    bool launched = false;
    SceneSlot* slot = nullptr;  // the scene it renders (own, or shared: mirt_ctx_share_scene)
    // frame buffers owned by the ctx (blocking API)
    uint32_t* d_out = nullptr;
    size_t out_cap = 0;
    AccumShare* acc = nullptr;  // accumulation buffer (own, or shared: mirt_ctx_share_accum)
    // staging for batch calls
    void* d_in = nullptr;
    void* d_res = nullptr;
    size_t in_cap = 0, res_cap = 0;
    mirt_counts* d_counts = nullptr;
    // kernel schedule (mirt_set_option)
    int trav = kTravWavefront;
    int fast_slab = 1;
    int block_waves = 4;  // waves (8x8 tiles) per workgroup
    int defer = 1;        // trace zero-component camera rays in leading waves
    int prune = 1;              // closest-hit pruning (trace.h Prune), FAST slab only
    int ordered = 1;            // ordered (nearer-child-first) walks where the tree admits them
    uint32_t* d_overlay = nullptr;  // BVH overlay: per-pixel last line in draw order
    size_t overlay_cap = 0;
    int bounce_threshold = 20;  // wavefront: shade finished rays once fewer lanes walk (swept: profiles/r02thr_threshold_sweep.txt)
    int bounce_blocks = 0;      // wavefront: persistent workgroups (set in mirt_create)
    int bounce_blocks_opt = 0;  // MIRT_OPT_BOUNCE_BLOCKS override (0: occupancy x CUs)
    int quad_drain = 1;         // four-wide bounce walk: finish the drain four lanes per ray
    int quad_batch = 1;                          // small BVH batches one ray per quad (intersect_quad_kernel)
    int leaf_batch_opt = 2;                        // MIRT_OPT_LEAF_BATCH: 0 off, 1 on, 2 auto (leaf_big)
    int zero_copy = 1;          // MIRT_OPT_ZERO_COPY: blocking frames into page-locked memory written in place
    void* d_queue = nullptr;    // wavefront: {count, head} + bounce records
    size_t queue_cap = 0;
    bool lone_frame = false;    // mirt_render_frame's frame: the first bounces queued in tile order
    Planes planes;              // mirt_render_frame_planes*: the planes of the frame being enqueued
    const mirt_ray* rays = nullptr;  // mirt_render_rays*: the camera rays of the frame being enqueued (device memory)
    void* d_rays = nullptr;     // rays of the blocking form, copied from the host ahead of the frame
    size_t rays_cap = 0;
    const LensConst* lens = nullptr;  // mirt_render_lens_frame*: the lens of the frame being enqueued (aperture > 0)
    void* d_planes = nullptr;   // planes of the blocking / async forms, copied to the host behind the frame
    size_t planes_cap = 0;
    PrimaryCache pc;            // MIRT_OPT_PRIMARY_CACHE: the camera rays' hits of a still camera
    PrimaryScan ps;             // MIRT_OPT_PRIMARY_SCAN: the camera rays' hits by a depth-sorted tile scan
    mirt_camera frame_cam{};    // the camera of the frame being enqueued (pc's reason)
    int queue_order = 0;        // MIRT_OPT_QUEUE_ORDER: 0 auto (tile order for lone_frame), 1 octants, 2 tile order
    uint32_t* d_defer = nullptr;  // [count, list...]
    size_t defer_cap = 0;
    unsigned long long* d_keys = nullptr;  // chunked brute force: per-ray (t, index) keys
    size_t keys_cap = 0;
    int num_cus = 0;
    int debug_stall_ms = 0;     // MIRT_OPT_DEBUG_STALL_MS: test hook, each frame starts behind a bounded wait
    int confirm_once = 2;       // MIRT_OPT_CONFIRM_ONCE: the bounce lane loop confirms a walk's closest hit once: 0 off, 1 on, 2 auto
    int debug_fail_confirm = 0; // MIRT_OPT_DEBUG_FAIL_CONFIRM: test hook, confirmations of pixels % N == 0 fail
    int build_finish = 1;       // MIRT_OPT_BUILD_FINISH: the device build's one-wave-per-subtree finish: 0 off, 1 auto, 2..64 = F
    mirt::BuildState* build = nullptr;  // mirt_bvh_build_flat_device's scratch (bvh_device.hip)
    mirt_scene_build_stats scene_stats{};  // of the last mirt_scene_build_device
    bool have_scene_stats = false;
    mirt_refit_stats refit_stats{};  // of the last mirt_scene_refit_device[_ptr]
    bool have_refit_stats = false;
    mirt::DenoiseState* denoise = nullptr;  // mirt_denoise*'s scratch (denoise.hip)
    int denoise_tile = 1;       // MIRT_OPT_DENOISE_TILE: passes of spacing 1 and 2 from an LDS tile (1) or by direct loads (0)
    void* d_guides = nullptr;   // mirt_render_frame_denoised: the frame's sphere and normal planes
    size_t guides_cap = 0;
    mirt::ReprojectState* reproject = nullptr;  // mirt_render_frame_reprojected's history (reproject.hip)
    mirt::VfilterState* vfilter = nullptr;  // mirt_denoise_var*'s scratch (vfilter.hip)
    int history_motion = 0;     // MIRT_OPT_HISTORY_MOTION: installs record a link, reprojected frames carry over it
    // the install a refit / update is about to make (ctx_link_intent): what its link holds
    bool link_intent = false, link_rebuilt = false;
    const int32_t *link_d_perm = nullptr, *link_h_perm = nullptr;
};

namespace {

int hip_fail(hipError_t e, const char* what)
{
    set_error("%s: %s", what, hipGetErrorString(e));
    return MIRT_E_DEVICE;
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

int ensure(void** p, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return MIRT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(p, bytes));
    *cap = bytes;
    return MIRT_OK;
}

// The scene a ctx renders: its slot's, or the empty one (num_spheres < 0: no
// scene) before the first install.
const Scene kNoScene{};
const Scene* scene_of(const mirt_ctx* c)
{
    return c->slot && c->slot->cur ? c->slot->cur : &kNoScene;
}

void scene_free(Scene* sn)
{
    for (void* p : {(void*)sn->d_nodes, (void*)sn->d_nodes32, (void*)sn->d_geo, (void*)sn->d_color, (void*)sn->d_pnodes,
                    (void*)sn->d_hnodes, (void*)sn->d_haux, (void*)sn->d_leaves, (void*)sn->d_ndepth})
        if (p) (void)hipFree(p);
    for (hipEvent_t ev : sn->readers) (void)hipEventDestroy(ev);
    delete sn;
}

// Frees the slot's retired scenes whose readers have all passed (wait: waits
// for them first -- a bounded wait, the frames were enqueued long ago).
void slot_reap(SceneSlot* sl, bool wait)
{
    size_t kept = 0;
    for (Scene* sn : sl->retired) {
        bool idle = true;
        for (hipEvent_t ev : sn->readers) {
            if (wait) (void)hipEventSynchronize(ev);
            else if (hipEventQuery(ev) != hipSuccess) idle = false;
        }
        if (!idle) (void)hipGetLastError();  // hipErrorNotReady is no error of a later launch
        if (idle) scene_free(sn);
        else sl->retired[kept++] = sn;
    }
    sl->retired.resize(kept);
}

// The slot gives up its scene: every frame its members have enqueued so far
// (on their own streams, or on a caller's stream -- `done` follows those) may
// still read it, so each member's stream gets an event behind them. The scene
// no slot holds any longer moves to this slot's retired list.
void slot_drop_scene(SceneSlot* sl)
{
    Scene* sn = sl->cur;
    sl->cur = nullptr;
    sl->have_base_cost = false;
    if (!sn) return;
    for (mirt_ctx* m : sl->members) {
        // a member with nothing in flight reads nothing: no event (the loop of
        // blocking frames then frees the replaced scene at once, as it always has)
        bool busy = hipStreamQuery(m->stream) != hipSuccess;
        if (m->launched && m->last_stream != m->stream && hipEventQuery(m->done) != hipSuccess) {
            (void)hipStreamWaitEvent(m->stream, m->done, 0);
            busy = true;
        }
        if (!busy) continue;
        (void)hipGetLastError();  // hipErrorNotReady is no error of a later launch
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess &&
            hipEventRecord(ev, m->stream) == hipSuccess) {
            sn->readers.push_back(ev);
        } else {
            if (ev) (void)hipEventDestroy(ev);
            (void)hipStreamSynchronize(m->stream);  // no event to be had: the frames themselves
        }
    }
    if (--sn->refs == 0) sl->retired.push_back(sn);
}

// The ctx leaves its slot (its own enqueued frames have been waited for). The
// last member takes the slot with it.
void slot_leave(mirt_ctx* c)
{
    SceneSlot* sl = c->slot;
    c->slot = nullptr;
    if (!sl) return;
    sl->members.erase(std::remove(sl->members.begin(), sl->members.end(), c), sl->members.end());
    if (!sl->members.empty()) return;
    slot_drop_scene(sl);
    slot_reap(sl, true);
    if (sl->link.d) (void)hipFree(sl->link.d);
    delete sl;
}

uint64_t next_scene_id()
{
    static std::mutex mu;
    static uint64_t last = 0;
    std::lock_guard<std::mutex> lock(mu);
    return ++last;
}

// Before an install gives up the slot's scene: when the ctx has
// MIRT_OPT_HISTORY_MOTION 1 and the install is a refit's or an update's
// (ctx_link_intent), the resident scene's geo array and the rebuild's
// permutation are copied into the link's free half and waited for -- the
// scene may be freed by the install itself. Nothing of the link proper
// changes here; slot_install commits or clears it. With the option at 0, or
// outside a refit / update, no device call is made.
int link_stage(mirt_ctx* c)
{
    SceneSlot* sl = c->slot;
    HistoryLink& lk = sl->link;
    lk.staged = false;
    const Scene* sn = sl->cur;
    if (c->history_motion != 1 || !c->link_intent || !sn || sn->num_spheres < 1) return MIRT_OK;
    const size_t n = (size_t)sn->num_spheres;
    const size_t half = ((sizeof(float4) + sizeof(int32_t)) * n + 255) & ~(size_t)255;
    if (2 * half > lk.cap) {
        // (a link in force holds as many spheres as the resident scene: it fits, and is not lost here)
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, 2 * half));
        if (lk.d) (void)hipFree(lk.d);
        lk.d = d;
        lk.cap = 2 * half;
        lk.valid = false;
    }
    const int h = lk.half ^ 1;   // (slot_install flips)
    char* const dst = lk.base(h);
    HIP_TRY(hipMemcpyAsync(dst, sn->d_geo, sizeof(float4) * n, hipMemcpyDeviceToDevice, c->stream));
    if (c->link_rebuilt) {
        if (c->link_d_perm)
            HIP_TRY(hipMemcpyAsync(dst + sizeof(float4) * n, c->link_d_perm, sizeof(int32_t) * n,
                                   hipMemcpyDeviceToDevice, c->stream));
        else
            HIP_TRY(hipMemcpyAsync(dst + sizeof(float4) * n, c->link_h_perm, sizeof(int32_t) * n,
                                   hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    lk.staged = true;
    lk.staged_from = sn->id;
    lk.staged_n = sn->num_spheres;
    lk.staged_rebuilt = c->link_rebuilt;
    return MIRT_OK;
}

// `sn` (complete on the device, refs == 0) becomes the scene of the ctx's
// slot, for every member. The link link_stage staged for this install comes
// into force; any other install clears the slot's link.
void slot_install(mirt_ctx* c, Scene* sn)
{
    SceneSlot* sl = c->slot;
    slot_drop_scene(sl);
    slot_reap(sl, false);
    sn->id = next_scene_id();
    sn->refs = 1;
    sl->cur = sn;
    HistoryLink& lk = sl->link;
    if (lk.staged && lk.staged_n == sn->num_spheres) {
        lk.half ^= 1;
        lk.valid = true;
        lk.from = lk.staged_from;
        lk.to = sn->id;
        lk.n = lk.staged_n;
        lk.rebuilt = lk.staged_rebuilt;
    } else {
        lk.valid = false;
    }
    lk.staged = false;
}

// MIRT_OPT_CONFIRM_ONCE in effect for the uploaded scene. Automatic (2): on up
// to kConfirmOnceLeaves leaves. Measured (MEASUREMENTS.md §D, round 8): at
// 10k spheres (1080p and 4K) every round is ahead of the parent; at 100k the
// bounce pass alone and the device-resident frames are ahead too, but the
// rounds of the frames-in-flight headline scatter -5% .. +5% around it (31.7%
// of the wave's loop iterations hold a confirmation at 10k, 15.2% at 100k).
// The line is the geometric middle of the two measured sizes; nothing in
// between has been measured.
constexpr uint32_t kConfirmOnceLeaves = 1u << 15;
static bool confirm_once(const mirt_ctx* c)
{
    return c->confirm_once == 1 || (c->confirm_once == 2 && scene_of(c)->num_leaves <= kConfirmOnceLeaves);
}

// MIRT_OPT_LEAF_BATCH: the bounce walk loads a step's passing leaf spheres
// together (bounce_kernel WALK 4) -- by default when the four-wide tree is
// larger than the chip's L2 (32 MiB over the 8 XCDs), where the leaf loads
// miss: 4K/1M +9%, 1080p/10k and 100k -9% / -6%
bool leaf_batch(const mirt_ctx* c)
{
    return c->leaf_batch_opt == 1 || (c->leaf_batch_opt == 2 && scene_of(c)->leaf_big);
}

DevScene dev_scene(const mirt_ctx* c)
{
    const Scene* sn = scene_of(c);
    const bool prune = c->prune && sn->prune_ok;
    const bool ordered = prune && c->ordered && sn->ordered_ok && c->fast_slab;
    return DevScene{sn->d_nodes, sn->d_nodes32, sn->d_geo, sn->d_color, (uint32_t)sn->num_nodes, sn->num_spheres,
                    prune, sn->r_max, sn->c_max, sn->d_pnodes, ordered, sn->d_hnodes, sn->d_haux,
                    (const float4*)sn->d_leaves, (const LeafBox*)(sn->d_leaves + sn->leaf_box_off), ordered,
                    ordered ? sn->num_hnodes : 0u, sn->wide_root, sn->o_bound};
}

AccumShare* accum_new(int device)
{
    AccumShare* a = new (std::nothrow) AccumShare();
    if (!a) return nullptr;
    a->device = device;
    if (hipEventCreateWithFlags(&a->folded, hipEventDisableTiming) != hipSuccess) {
        delete a;
        return nullptr;
    }
    if (hipEventCreateWithFlags(&a->pend_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipEventDestroy(a->folded);
        delete a;
        return nullptr;
    }
    return a;
}

void accum_release(AccumShare* a)
{
    if (!a || --a->refs > 0) return;
    if (a->d_acc) (void)hipFree(a->d_acc);
    if (a->folded) (void)hipEventDestroy(a->folded);
    if (a->pend_ev) (void)hipEventDestroy(a->pend_ev);
    delete a;
}

// A fresh frame's accumulation state from its display: acc = c / 255 per
// channel, exactly store_pixel's fresh branch (main.c:368-370).
__global__ void acc_from_display_kernel(const uint32_t* __restrict__ disp, float* __restrict__ acc, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = disp[i];
    for (int ch = 0; ch < 3; ch++) acc[3 * i + ch] = (float)((c >> (8 * ch)) & 0xff) / 255.0f;
}

// The share's pending fresh frame folded into d_acc on stream s, behind the
// share's last fold and that frame's render; the slab's ctx then waits for
// this read before writing its slab again.
int accum_materialize(AccumShare* a, hipStream_t s)
{
    if (!a || !a->pend) return MIRT_OK;
    if (a->has_fold) HIP_TRY(hipStreamWaitEvent(s, a->folded, 0));
    HIP_TRY(hipStreamWaitEvent(s, a->pend_ev, 0));
    const size_t n = a->pixels;
    acc_from_display_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a->pend, a->d_acc, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(a->folded, s));
    a->has_fold = true;
    mirt_ctx* pc = a->pend_ctx;
    HIP_TRY(hipEventRecord(pc->slab_free, s));
    pc->slab_guard = true;
    a->pend = nullptr;
    a->pend_ctx = nullptr;
    return MIRT_OK;
}

// A fresh frame's display left pending on its share (the lazy fold): the
// newest fresh frame supersedes any earlier one.
int accum_set_pending(AccumShare* a, mirt_ctx* c, const uint32_t* disp, hipStream_t s)
{
    HIP_TRY(hipEventRecord(a->pend_ev, s));
    a->pend = disp;
    a->pend_ctx = c;
    return MIRT_OK;
}

// The accumulation buffer for frames of `pixels` pixels, enqueued on stream
// s: (re)allocated if too small, cleared when the frame geometry changes
// (a new accumulation starts). Ordered behind the share's last fold.
int accum_prepare(AccumShare* a, size_t pixels, hipStream_t s)
{
    if (a->cap < pixels * 12 + 4) {
        // other ctxs' streams may still fold into the old buffer
        if (a->d_acc) HIP_TRY(hipDeviceSynchronize());
        int rc = ensure((void**)&a->d_acc, &a->cap, pixels * 12 + 4);
        if (rc) return rc;
        a->pixels = 0;
    }
    if (a->pixels != pixels) {
        a->pend = nullptr;   // a frame of the old geometry: a new accumulation starts
        a->pend_ctx = nullptr;
        if (a->has_fold) HIP_TRY(hipStreamWaitEvent(s, a->folded, 0));
        if (pixels) HIP_TRY(hipMemsetAsync(a->d_acc, 0, pixels * 12, s));   // 0: an empty shard (mirt.h)
        HIP_TRY(hipEventRecord(a->folded, s));
        a->has_fold = true;
        a->pixels = pixels;
    }
    return MIRT_OK;
}

bool ctx_ok(mirt_ctx* c, bool need_scene, const char* fn)
{
    if (!c) {
        set_error("%s: null context", fn);
        return false;
    }
    if (need_scene && scene_of(c)->num_spheres < 0) {
        set_error("%s: no scene uploaded", fn);
        return false;
    }
    return hipSetDevice(c->device) == hipSuccess;
}

bool has_planes(const Planes& pl) { return pl.t || pl.sphere || pl.normal; }

// How one frame meets the ctx's primary cache: MIRT_PCACHE_*, and the slab.
struct PrimaryUse {
    int how = MIRT_PCACHE_BYPASS;
    float* t = nullptr;
    int32_t* sphere = nullptr;
};

// The camera-packet kernel of a frame, with the planes' stores if it has any.
// pcu: how the frame meets the ctx's primary cache (pc_classify) -- a hit runs
// the one cached form (no walk: bounded and unbounded are the same kernel), a
// fill the walk that also stores frame 0's hits.
template <bool FAST, bool ORD, bool BND>
void launch_primary(int blocks, hipStream_t s, const DevScene& sc, const FrameConst& f, uint32_t* d_out, float* d_acc,
                    Deferred dfr, BounceRec* queue, uint32_t* qctl, int octants, const Planes& pl,
                    const PrimaryUse& pcu = PrimaryUse{})
{
    if constexpr (FAST && ORD) {
        if (pcu.how == MIRT_PCACHE_HIT) {
            primary_kernel<true, true, false><<<blocks, 256, 0, s>>>(sc, f, d_out, d_acc, dfr, queue, qctl, octants,
                                                                     CacheRead{pcu.t, pcu.sphere});
            return;
        }
        if (pcu.how == MIRT_PCACHE_FILL) {
            primary_kernel<true, true, BND><<<blocks, 256, 0, s>>>(sc, f, d_out, d_acc, dfr, queue, qctl, octants,
                                                                   CacheFill{pcu.t, pcu.sphere});
            return;
        }
    }
    if (has_planes(pl))
        primary_kernel<FAST, ORD, BND><<<blocks, 256, 0, s>>>(sc, f, d_out, d_acc, dfr, queue, qctl, octants, pl);
    else
        primary_kernel<FAST, ORD, BND><<<blocks, 256, 0, s>>>(sc, f, d_out, d_acc, dfr, queue, qctl, octants);
}

// The kernels of a ray frame (c->rays), with the planes' stores if it has any.
void launch_ray_primary(bool fast, int blocks, hipStream_t s, const DevScene& sc, const FrameConst& f,
                        const mirt_ray* rays, uint32_t* d_out, float* d_acc, BounceRec* queue, uint32_t* qctl,
                        const Planes& pl)
{
    if (fast && has_planes(pl))
        ray_primary_kernel<true><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc, queue, qctl, pl);
    else if (fast)
        ray_primary_kernel<true><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc, queue, qctl);
    else if (has_planes(pl))
        ray_primary_kernel<false><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc, queue, qctl, pl);
    else
        ray_primary_kernel<false><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc, queue, qctl);
}

void launch_ray_path(bool fast, int blocks, hipStream_t s, const DevScene& sc, const FrameConst& f,
                     const mirt_ray* rays, uint32_t* d_out, float* d_acc, const Planes& pl)
{
    if (fast && has_planes(pl))
        ray_path_kernel<true><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc, pl);
    else if (fast)
        ray_path_kernel<true><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc);
    else if (has_planes(pl))
        ray_path_kernel<false><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc, pl);
    else
        ray_path_kernel<false><<<blocks, 256, 0, s>>>(sc, f, rays, d_out, d_acc);
}

// The kernels of a lens frame (c->lens), with the planes' stores if it has any.
void launch_lens_primary(bool fast, int blocks, hipStream_t s, const DevScene& sc, const FrameConst& f,
                         const LensConst& lc, uint32_t* d_out, float* d_acc, BounceRec* queue, uint32_t* qctl,
                         const Planes& pl)
{
    if (fast && has_planes(pl))
        lens_primary_kernel<true><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc, queue, qctl, pl);
    else if (fast)
        lens_primary_kernel<true><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc, queue, qctl);
    else if (has_planes(pl))
        lens_primary_kernel<false><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc, queue, qctl, pl);
    else
        lens_primary_kernel<false><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc, queue, qctl);
}

void launch_lens_path(bool fast, int blocks, hipStream_t s, const DevScene& sc, const FrameConst& f,
                      const LensConst& lc, uint32_t* d_out, float* d_acc, const Planes& pl)
{
    if (fast && has_planes(pl))
        lens_path_kernel<true><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc, pl);
    else if (fast)
        lens_path_kernel<true><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc);
    else if (has_planes(pl))
        lens_path_kernel<false><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc, pl);
    else
        lens_path_kernel<false><<<blocks, 256, 0, s>>>(sc, f, lc, d_out, d_acc);
}

template <bool COUNT>
void dispatch_render(bool fast, const DevScene& sc, const FrameConst& f, uint32_t* d_out, float* d_acc, hipStream_t s,
                     int blocks, int bw, mirt_counts* d_counts, uint32_t* d_ws, Deferred dfr, const Planes& pl)
{
    if (!COUNT && has_planes(pl) && fast)
        render_kernel<true, false><<<blocks + dfr.blocks, 64 * bw, 0, s>>>(sc, f, d_out, d_acc, nullptr, nullptr, dfr, pl);
    else if (!COUNT && has_planes(pl))
        render_kernel<false, false><<<blocks + dfr.blocks, 64 * bw, 0, s>>>(sc, f, d_out, d_acc, nullptr, nullptr, dfr, pl);
    else if (fast)
        render_kernel<true, COUNT><<<blocks + dfr.blocks, 64 * bw, 0, s>>>(sc, f, d_out, d_acc, d_counts, d_ws, dfr);
    else
        render_kernel<false, COUNT><<<blocks + dfr.blocks, 64 * bw, 0, s>>>(sc, f, d_out, d_acc, d_counts, d_ws, dfr);
}

int launch_render_body(mirt_ctx* c, const FrameConst& f, uint32_t* d_out, float* d_acc, hipStream_t s, bool timed,
                       mirt_counts* d_counts, uint32_t* d_wave_stats, uint64_t* d_bdiag, AccumShare* chain);

// The accumulation chain of a frame of ctx c: its share when other ctxs hold
// it too (their folds must be ordered), else none.
AccumShare* accum_chain(const mirt_ctx* c)
{
    return c->acc && c->acc->refs > 1 ? c->acc : nullptr;
}

// The first bounces grouped by direction octant in the queue (frames in
// flight) or in tile order (a frame alone: the blocking call), or as
// MIRT_OPT_QUEUE_ORDER forces.
int octant_queue(const mirt_ctx* c)
{
    return c->queue_order == 1 || (c->queue_order == 0 && !c->lone_frame) ? 1 : 0;
}

int launch_render(mirt_ctx* c, const FrameConst& f, uint32_t* d_out, float* d_acc, hipStream_t s, bool timed,
                  mirt_counts* d_counts, uint32_t* d_wave_stats = nullptr, uint64_t* d_bdiag = nullptr)
{
    if (c->launched && c->last_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->done, 0));
    if (c->slab_guard) {   // another stream still reads this ctx's slab (a pending fold)
        HIP_TRY(hipStreamWaitEvent(s, c->slab_free, 0));
        c->slab_guard = false;
    }
    const int rc = launch_render_body(c, f, d_out, d_acc, s, timed, d_counts, d_wave_stats, d_bdiag,
                                      d_counts ? nullptr : accum_chain(c));
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->done, s));
    c->last_stream = s;
    c->launched = true;
    // a fill is the cache's content once every call of its launch has succeeded
    if (c->pc.on && c->pc.last == MIRT_PCACHE_FILL) c->pc.valid = true;
    return MIRT_OK;
}

// The frame's camera rays may test the grown PNode inner-child boxes without
// margins (trace.h slab_cons_fast<BND>): the camera within 4C.
bool camera_bounded(const mirt_ctx* c, const FrameConst& f)
{
    const float o = std::max(std::fabs(f.px), std::max(std::fabs(f.py), std::fabs(f.pz)));
    return origin_within_4c(scene_of(c)->o_bound, o);
}

// MIRT_OPT_PRIMARY_CACHE: the frame being enqueued is a bypass, a hit or a
// fill, decided here on the host. diag: a counting or diagnostic
// launch. Eligible is exactly the frame for which launch_render_body picks
// primary_kernel<true, true, *>, without jitter, without planes and with the
// pinhole's rays (a ray frame, c->rays, has no camera to key a cache by, and a
// lens frame, c->lens, draws other rays every sample); the
// reasons are looked for in the order of the enum. A fill whose slab outgrows
// the allocation waits for the frames that may still read it, then grows it
// (the rule of d_planes): no allocation on a hit or a same-size fill.
int pc_classify(mirt_ctx* c, const FrameConst& f, bool diag, PrimaryUse* use)
{
    PrimaryCache& pc = c->pc;
    *use = PrimaryUse{};
    if (!pc.on) return MIRT_OK;
    const bool packet = c->trav == kTravWavefront && f.use_bvh && f.depth >= 1 && !diag && c->fast_slab &&
                        dev_scene(c).ordered && f.num_rows > 0 && f.width > 0;
    const int why = !packet ? MIRT_PCACHE_SCHEDULE : f.jitter ? MIRT_PCACHE_JITTER
                    : has_planes(c->planes) ? MIRT_PCACHE_PLANES : c->rays ? MIRT_PCACHE_RAYS
                    : c->lens ? MIRT_PCACHE_LENS : 0;
    if (why) {
        pc.bypassed++;
        pc.last = MIRT_PCACHE_BYPASS;
        pc.reason = why;
        return MIRT_OK;
    }
    PrimaryKey k;
    std::memset(&k, 0, sizeof k);
    std::memcpy(k.cam, &f.px, sizeof k.cam);
    k.aspect = f.aspect; k.wf = f.wf; k.hf = f.hf;
    k.width = f.width; k.height = f.height; k.row_block = f.row_block; k.shard = f.shard;
    k.num_shards = f.num_shards; k.lead_skip = f.lead_skip; k.shard_rows = f.shard_rows;
    k.scene_id = scene_of(c)->id;
    if (pc.valid && !std::memcmp(&k, &pc.key, sizeof k)) {
        pc.hits++;
        pc.last = MIRT_PCACHE_HIT;
        pc.reason = 0;
    } else {
        const int reason = !pc.valid ? MIRT_PCACHE_EMPTY : k.scene_id != pc.key.scene_id ? MIRT_PCACHE_SCENE
                           : std::memcmp(&c->frame_cam, &pc.cam, sizeof pc.cam) ? MIRT_PCACHE_CAMERA
                                                                                : MIRT_PCACHE_GEOMETRY;
        pc.valid = false;   // until the launch is enqueued (launch_render)
        const size_t bytes = 8 * (size_t)k.shard_rows * k.width;
        if (bytes > pc.cap) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
            if (int rc = ensure(&pc.d, &pc.cap, bytes)) return rc;
        }
        pc.key = k;
        pc.cam = c->frame_cam;
        pc.fills++;
        pc.last = MIRT_PCACHE_FILL;
        pc.reason = reason;
    }
    use->how = pc.last;
    use->t = (float*)pc.d;
    use->sphere = (int32_t*)pc.d + pc.pixels();
    return MIRT_OK;
}

// MIRT_OPT_PRIMARY_SCAN: the frame being enqueued takes the tile scan
// (*scan = true) or is a bypass with a recorded reason and runs the kernels
// and arguments it ran before, decided here on the host. The
// reasons are looked for in the order of the enum. Eligible is a frame for
// which launch_render_body picks primary_kernel<true, true, *> without
// jitter, planes, rays or a lens, on a bounded tree that nests (o_bound > 0:
// finite coordinates, which pscan.h's margins assume), whose 8-row tiles are
// bands of the image, with a camera pscan_camera accepts. A scanned frame
// whose arrays outgrow the allocation waits for the ctx's frames, then grows
// it: no allocation while the sizes stay.
int ps_classify(mirt_ctx* c, const FrameConst& f, bool diag, bool* scan)
{
    PrimaryScan& ps = c->ps;
    *scan = false;
    const Scene* sn = scene_of(c);
    const DevScene sc = dev_scene(c);
    const bool packet = c->trav == kTravWavefront && f.use_bvh && f.depth >= 1 && !diag && c->fast_slab && sc.ordered &&
                        f.num_rows > 0 && f.width > 0;
    PscanFrame fr;
    std::memcpy(fr.p, &f.px, 12 * sizeof(float));
    fr.aspect = f.aspect; fr.wf = f.wf; fr.hf = f.hf; fr.width = f.width; fr.height = f.height;
    // the caller's camera of this frame (the enqueuing calls record it): its fov, which f no longer shows
    const bool own_cam = !std::memcmp(&c->frame_cam.position, &f.px, 12) && !std::memcmp(&c->frame_cam.forward, &f.fx, 12);
    fr.fov = own_cam ? c->frame_cam.fov : NAN;
    PscanCam cam{};
    int why = !ps.opt ? MIRT_PSCAN_OFF : c->pc.on ? MIRT_PSCAN_CACHE : !packet ? MIRT_PSCAN_SCHEDULE
              : f.jitter ? MIRT_PSCAN_JITTER : has_planes(c->planes) ? MIRT_PSCAN_PLANES : c->rays ? MIRT_PSCAN_RAYS
              : c->lens ? MIRT_PSCAN_LENS : !(sc.wide && sn->prune_ok && sn->o_bound > 0.0f) ? MIRT_PSCAN_TREE
              : !(f.row_block % 8 == 0 || (f.num_shards == 1 && f.lead_skip == 0)) ? MIRT_PSCAN_SHARD : 0;
    if (!why && (f.width > 8 * kPscanMaxTiles || f.height > 8 * kPscanMaxTiles)) why = MIRT_PSCAN_SIZE;
    if (!why && pscan_camera(fr, &cam) != PSCAN_CAM_OK) why = MIRT_PSCAN_CAMERA;
    if (!why && ps.opt == 2 && ps.h_verdict && *(volatile unsigned long long*)ps.h_verdict == sn->id) why = MIRT_PSCAN_SPARSE;
    if (why) {
        if (why != MIRT_PSCAN_OFF) ps.bypassed++;
        ps.last = MIRT_PSCAN_BYPASS;
        ps.reason = why;
        return MIRT_OK;
    }
    PrimaryKey k;
    std::memset(&k, 0, sizeof k);
    std::memcpy(k.cam, &f.px, sizeof k.cam);
    k.aspect = f.aspect; k.wf = f.wf; k.hf = f.hf;
    k.width = f.width; k.height = f.height; k.row_block = f.row_block; k.shard = f.shard;
    k.num_shards = f.num_shards; k.lead_skip = f.lead_skip; k.shard_rows = f.shard_rows;
    k.scene_id = sn->id;
    if (!(ps.valid && !ps.always_rebuild && !std::memcmp(&k, &ps.key, sizeof k))) {
        ps.valid = false;   // until the build is enqueued (launch_render_body)
        const uint32_t nl = sn->num_leaves;
        if (ps.sort_nl != nl) {
            ps.sort_bytes = pscan_sort_bytes(nl);
            ps.sort_nl = nl;
            if (!ps.sort_bytes) return hip_fail(hipErrorUnknown, "rocprim::radix_sort_pairs (size query)");
        }
        const size_t pixels = (size_t)f.shard_rows * f.width;
        const size_t tiles = (size_t)((f.width + 7) / 8) * ((f.shard_rows + 7) / 8);
        const size_t n1 = nl ? nl : 1;
        const size_t sizes[] = {sizeof(PscanRec) * n1, sizeof(PscanRec) * n1, 4 * n1, 4 * n1,
                                sizeof(PscanPlanes) * (size_t)(cam.ntx + cam.nty),
                                sizeof(int) * (size_t)(cam.ntx + 1) * (cam.nty + 1), ps.sort_bytes, 4 * pixels, 4 * pixels,
                                8 * (size_t)kPscanSlots * kPscanSlotWords, 4 * (tiles + 1)};
        size_t off[12] = {0};
        for (int i = 0; i < 11; i++) off[i + 1] = (off[i] + sizes[i] + 255) & ~(size_t)255;
        if (off[11] > ps.cap) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
            if (int rc = ensure(&ps.d, &ps.cap, off[11])) return rc;
        }
        if (!ps.h_verdict) {   // once per ctx, with the first allocation above
            HIP_TRY(hipHostMalloc((void**)&ps.h_verdict, 64, hipHostMallocMapped));
            *ps.h_verdict = 0;
            HIP_TRY(hipHostGetDevicePointer((void**)&ps.d_verdict, ps.h_verdict, 0));
        }
        char* d = (char*)ps.d;
        ps.b = PscanBuild{(PscanRec*)(d + off[0]), (PscanRec*)(d + off[1]), (float*)(d + off[2]), (float*)(d + off[3]),
                          (PscanPlanes*)(d + off[4]), (int*)(d + off[5]), d + off[6], ps.sort_bytes};
        ps.t = (float*)(d + off[7]);
        ps.sphere = (int32_t*)(d + off[8]);
        ps.stats = (unsigned long long*)(d + off[9]);   // the walk list's count follows the counters' last line
        ps.wlist = (uint32_t*)(d + off[10]);
        ps.nl = nl;
        ps.cam = cam;
        ps.key = k;
    }
    ps.scanned++;
    ps.last = MIRT_PSCAN_SCAN;
    ps.reason = MIRT_PSCAN_NONE;
    *scan = true;
    return MIRT_OK;
}

// The scan pass of a frame ps_classify accepted, ahead of its camera-packet
// kernel: the per-camera data if they are not the key's, the tile scan, the
// walk of the tiles it listed. *pcu: the slab, for the cached form.
int launch_scan(mirt_ctx* c, const DevScene& sc, const FrameConst& f, hipStream_t s, PrimaryUse* pcu)
{
    PrimaryScan& ps = c->ps;
    if (!ps.valid) {
        HIP_TRY((hipError_t)pscan_build(ps.cam, sc.leaf_geo, ps.nl, ps.b, s));
        ps.valid = true;
        ps.rebuilds++;
    }
    const int tiles = ((f.width + 7) / 8) * ((f.shard_rows + 7) / 8);
    HIP_TRY(hipMemsetAsync(ps.stats, 0, 8 * (size_t)kPscanSlots * kPscanSlotWords, s));
    HIP_TRY(hipMemsetAsync(ps.wlist, 0, 4, s));
    const PscanDev dev{ps.b.rec, ps.b.grid, ps.nl, ps.cam.ntx + 1, ps.cam.g[0], ps.cam.g[1], ps.cam.g[2],
                       ps.t, ps.sphere, ps.wlist, ps.stats, ps.budget};
    pscan_tile_kernel<<<(tiles + 3) / 4, 256, 0, s>>>(sc, f, dev);
    const int wblocks = std::min((tiles + 3) / 4, 8 * std::max(1, c->num_cus));
    if (camera_bounded(c, f))
        pscan_walk_kernel<true><<<wblocks, 256, 0, s>>>(sc, f, dev);
    else
        pscan_walk_kernel<false><<<wblocks, 256, 0, s>>>(sc, f, dev);
    if (ps.opt == 2) pscan_verdict_kernel<<<1, 1, 0, s>>>(ps.stats, ps.d_verdict, scene_of(c)->id);
    HIP_TRY(hipGetLastError());
    pcu->how = MIRT_PCACHE_HIT;
    pcu->t = ps.t;
    pcu->sphere = ps.sphere;
    return MIRT_OK;
}

int launch_render_body(mirt_ctx* c, const FrameConst& f, uint32_t* d_out, float* d_acc, hipStream_t s, bool timed,
                       mirt_counts* d_counts, uint32_t* d_wave_stats, uint64_t* d_bdiag, AccumShare* chain)
{
    PrimaryUse pcu;
    if (int rc = pc_classify(c, f, d_counts || d_wave_stats || d_bdiag, &pcu)) return rc;
    bool scan = false;
    if (int rc = ps_classify(c, f, d_counts || d_wave_stats || d_bdiag, &scan)) return rc;
    const int tiles = ((f.width + 7) / 8) * ((f.num_rows + 7) / 8);
    const int bw = c->block_waves;
    const int blocks = (tiles + bw - 1) / bw;
    if (blocks == 0) return MIRT_OK;
    if (c->debug_stall_ms > 0) {
        stall_kernel<<<1, 64, 0, s>>>((uint64_t)c->debug_stall_ms * 100000u);
        HIP_TRY(hipGetLastError());
    }
    if (timed) {
        HIP_TRY(hipEventRecord(c->ev0, s));
        c->timed_recorded = true;
    }
    // several frames, or a buffer shared with other ctxs' frames in flight,
    // and an accumulation buffer: raw colours per frame, then
    // fold_samples_kernel accumulates them in order (behind the previous
    // fold into a shared buffer, whichever stream enqueued it)
    float* const d_fold = f.samples > 1 || chain ? d_acc : nullptr;
    if (d_fold) d_acc = nullptr;
    // Lazy fold: a fresh one-sample frame on a share leaves its display
    // pending instead of folding it; any other frame that folds first takes
    // the pending one (an accumulating frame needs it in d_acc) or drops it (a
    // fresh multi-sample fold overwrites d_acc whole)
    const bool lazy = chain && d_fold && !f.accumulate && f.samples == 1;
    if (chain && d_fold && !lazy) {
        if (f.accumulate) {
            if (int rc = accum_materialize(chain, s)) return rc;   // before this frame's render can touch a slab
        } else {
            chain->pend = nullptr;
            chain->pend_ctx = nullptr;
        }
    }
    auto fold = [&]() -> int {
        if (!d_fold) return MIRT_OK;
        if (lazy) return accum_set_pending(chain, c, d_out, s);
        const size_t n = (size_t)f.shard_rows * f.width;
        if (chain && chain->has_fold) HIP_TRY(hipStreamWaitEvent(s, chain->folded, 0));
        fold_samples_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(f, d_out, d_fold);
        HIP_TRY(hipGetLastError());
        if (chain) {
            HIP_TRY(hipEventRecord(chain->folded, s));
            chain->has_fold = true;
        }
        return MIRT_OK;
    };
    const bool wavefront = c->trav == kTravWavefront && f.use_bvh && f.depth >= 2 && !d_counts;
    // depth 1 (camera rays and their shading only): the camera-packet kernel
    // alone, at its 8 waves per SIMD, where the tree admits the ordered walk
    const mirt_ray* const rays = c->rays;   // a ray frame (mirt_render_rays*): never a counting launch
    // a lens frame (mirt_render_lens_frame*) takes the ray frame's branches with its own kernels
    const LensConst* const lens = rays ? nullptr : c->lens;
    const bool given = rays || lens;
    const bool primary_only = c->trav == kTravWavefront && f.use_bvh && f.depth == 1 && !d_counts && c->fast_slab &&
                              dev_scene(c).ordered && !given;
    // a ray frame on the wavefront schedule: ray_primary_kernel at every depth,
    // alone below depth 2; on the others ray_path_kernel
    const bool ray_primary = given && c->trav == kTravWavefront && f.use_bvh;
    const int dbw = wavefront || primary_only ? 4 : bw;  // the wavefront kernels use 256-thread workgroups
    Deferred dfr{nullptr, nullptr, 0};
    c->phases_valid = wavefront;
    const uint32_t ps = c->ph_next;
    if (wavefront) {
        HIP_TRY(hipEventRecord(c->ph0[ps], s));
        c->ph_next = (ps + 1) % kPhaseRing;
        c->ph_count = std::min<uint32_t>(c->ph_count + 1, kPhaseRing);
    }
    const DevScene sc = dev_scene(c);
    // the ordered packet walk takes zero-component camera rays itself
    if (f.use_bvh && c->defer && !sc.ordered && !given) {
        const size_t pixels = (size_t)f.num_rows * f.width;
        int rc = ensure((void**)&c->d_defer, &c->defer_cap, 4 * (pixels + 1));
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(c->d_defer, 0, 4, s));
        mark_deferred_kernel<<<dim3((f.width + 255) / 256, f.num_rows), 256, 0, s>>>(f, c->d_defer + 1, c->d_defer);
        HIP_TRY(hipGetLastError());
        // enough waves for the centre row and column of an axis-aligned
        // camera; a longer list is strided over the same waves
        const size_t want = std::min(pixels, (size_t)(f.width + f.num_rows + 64));
        dfr = Deferred{c->d_defer + 1, c->d_defer, (int)((want + dbw - 1) / dbw)};
    }
    if (primary_only) {
        // no bounce records: the queue is never written (its control words
        // are read only by a bounce pass)
        int rc = ensure(&c->d_queue, &c->queue_cap, sizeof(BounceRec) + kQCtlBytes);
        if (rc) return rc;
        uint32_t* qctl = (uint32_t*)c->d_queue;
        BounceRec* queue = (BounceRec*)((char*)c->d_queue + kQCtlBytes);
        const int ptiles = f.samples >= 4 ? ((f.width + 3) / 4) * ((f.shard_rows + 3) / 4) * ((f.samples + 3) / 4)
                                          : tiles;
        if (scan)
            if (int rc2 = launch_scan(c, sc, f, s, &pcu)) return rc2;
        if (camera_bounded(c, f))
            launch_primary<true, true, true>((ptiles + 3) / 4, s, sc, f, d_out, d_acc, dfr, queue, qctl, 1, c->planes, pcu);
        else
            launch_primary<true, true, false>((ptiles + 3) / 4, s, sc, f, d_out, d_acc, dfr, queue, qctl, 1, c->planes, pcu);
        HIP_TRY(hipGetLastError());
        if (int rc2 = fold()) return rc2;
        if (timed) HIP_TRY(hipEventRecord(c->ev1, s));
        return MIRT_OK;
    }
    if (ray_primary && !wavefront) {
        // depth 0 and 1: no bounce records (the queue is passed, never written)
        int rc = ensure(&c->d_queue, &c->queue_cap, sizeof(BounceRec) + kQCtlBytes);
        if (rc) return rc;
        if (lens)
            launch_lens_primary(c->fast_slab != 0, (tiles + 3) / 4, s, sc, f, *lens, d_out, d_acc,
                                (BounceRec*)((char*)c->d_queue + kQCtlBytes), (uint32_t*)c->d_queue, c->planes);
        else
            launch_ray_primary(c->fast_slab != 0, (tiles + 3) / 4, s, sc, f, rays, d_out, d_acc,
                               (BounceRec*)((char*)c->d_queue + kQCtlBytes), (uint32_t*)c->d_queue, c->planes);
        HIP_TRY(hipGetLastError());
        if (int rc2 = fold()) return rc2;
        if (timed) HIP_TRY(hipEventRecord(c->ev1, s));
        return MIRT_OK;
    }
    if (wavefront) {
        const size_t pixels = (size_t)f.num_rows * f.width;
        int rc = ensure(&c->d_queue, &c->queue_cap, sizeof(BounceRec) * pixels + kQCtlBytes);
        if (rc) return rc;
        uint32_t* qctl = (uint32_t*)c->d_queue;                          // {count}, segment heads
        BounceRec* queue = (BounceRec*)((char*)c->d_queue + kQCtlBytes);
        HIP_TRY(hipMemsetAsync(qctl, 0, kQCtlBytes, s));
        // primary_kernel's packets: 8x8 pixel tiles, or 4x4 pixels x 4 frames
        // for an ordered walk over four frames or more
        const int ptiles = c->fast_slab && sc.ordered && f.samples >= 4 && !given
                               ? ((f.width + 3) / 4) * ((f.shard_rows + 3) / 4) * ((f.samples + 3) / 4)
                               : tiles;
        const int pblocks = (ptiles + 3) / 4 + dfr.blocks;
        const int bblocks = c->bounce_blocks_opt ? c->bounce_blocks_opt : c->bounce_blocks;
        const size_t blds = bounce_lds_bytes(f.depth);
        const int oq = octant_queue(c);
        if (scan)
            if (int rc2 = launch_scan(c, sc, f, s, &pcu)) return rc2;
        if (rays)
            launch_ray_primary(c->fast_slab != 0, pblocks, s, sc, f, rays, d_out, d_acc, queue, qctl, c->planes);
        else if (lens)
            launch_lens_primary(c->fast_slab != 0, pblocks, s, sc, f, *lens, d_out, d_acc, queue, qctl, c->planes);
        else if (c->fast_slab && sc.ordered && camera_bounded(c, f))
            launch_primary<true, true, true>(pblocks, s, sc, f, d_out, d_acc, dfr, queue, qctl, oq, c->planes, pcu);
        else if (c->fast_slab && sc.ordered)
            launch_primary<true, true, false>(pblocks, s, sc, f, d_out, d_acc, dfr, queue, qctl, oq, c->planes, pcu);
        else if (c->fast_slab)
            launch_primary<true, false, false>(pblocks, s, sc, f, d_out, d_acc, dfr, queue, qctl, oq, c->planes);
        else
            launch_primary<false, false, false>(pblocks, s, sc, f, d_out, d_acc, dfr, queue, qctl, oq, c->planes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ph1[ps], s));
        if (d_bdiag && sc.wide)
            bounce_kernel<true, 2, true><<<bblocks, 256, blds, s>>>(sc, f, d_out, d_acc, queue, qctl, c->bounce_threshold, c->quad_drain, confirm_once(c) ? 0 : kExactWalk, c->debug_fail_confirm, d_bdiag);
        else if (d_bdiag)
            bounce_kernel<true, 0, true><<<bblocks, 256, blds, s>>>(sc, f, d_out, d_acc, queue, qctl, c->bounce_threshold, c->quad_drain, confirm_once(c) ? 0 : kExactWalk, c->debug_fail_confirm, d_bdiag);
        else if (sc.wide && leaf_batch(c))
            bounce_kernel<true, 4><<<bblocks, 256, blds, s>>>(sc, f, d_out, d_acc, queue, qctl, c->bounce_threshold, c->quad_drain, confirm_once(c) ? 0 : kExactWalk, c->debug_fail_confirm);
        else if (sc.wide)
            bounce_kernel<true, 2><<<bblocks, 256, blds, s>>>(sc, f, d_out, d_acc, queue, qctl, c->bounce_threshold, c->quad_drain, confirm_once(c) ? 0 : kExactWalk, c->debug_fail_confirm);
        else if (c->fast_slab)
            bounce_kernel<true, 0><<<bblocks, 256, blds, s>>>(sc, f, d_out, d_acc, queue, qctl, c->bounce_threshold, c->quad_drain, confirm_once(c) ? 0 : kExactWalk, c->debug_fail_confirm);
        else
            bounce_kernel<false, 0><<<bblocks, 256, blds, s>>>(sc, f, d_out, d_acc, queue, qctl, c->bounce_threshold, c->quad_drain, confirm_once(c) ? 0 : kExactWalk, c->debug_fail_confirm);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ph2[ps], s));
        if (int rc = fold()) return rc;
        if (timed) HIP_TRY(hipEventRecord(c->ev1, s));
        return MIRT_OK;
    }
    if (rays)
        launch_ray_path(c->fast_slab != 0, (tiles + 3) / 4, s, sc, f, rays, d_out, d_acc, c->planes);
    else if (lens)
        launch_lens_path(c->fast_slab != 0, (tiles + 3) / 4, s, sc, f, *lens, d_out, d_acc, c->planes);
    else if (d_counts)
        dispatch_render<true>(true, sc, f, d_out, d_acc, s, blocks, bw, d_counts, d_wave_stats, dfr, c->planes);
    else
        dispatch_render<false>(c->fast_slab != 0, sc, f, d_out, d_acc, s, blocks, bw, nullptr, nullptr, dfr, c->planes);
    HIP_TRY(hipGetLastError());
    if (int rc = fold()) return rc;
    if (timed) HIP_TRY(hipEventRecord(c->ev1, s));
    return MIRT_OK;
}

// Workgroup size of a per-ray batch kernel: one wave per workgroup while the
// batch is too small to give every CU a few waves (each walk is a chain of
// dependent loads, so spreading the waves over CUs is what shortens it).
int batch_threads(const mirt_ctx* c, int n)
{
    return n < 256 * 4 * std::max(1, c->num_cus) ? 64 : 256;
}

// intersect_quad_kernel for a BVH batch: the four-wide tree, the fast slab
// filter, and fewer rays than give every CU four waves of one ray per lane
// (MIRT_OPT_QUAD_BATCH 0 turns it off)
bool quad_batch(const mirt_ctx* c, int n)
{
    const DevScene sc = dev_scene(c);
    return c->quad_batch && c->fast_slab && sc.wide && n <= 64 * 4 * std::max(1, c->num_cus);
}

// brute_chunk_kernel over the rays in c->d_in: enough sphere chunks that the
// grid has ~8 workgroups per CU whatever the ray count.
int launch_brute(mirt_ctx* c, int n)
{
    int rc = ensure((void**)&c->d_keys, &c->keys_cap, sizeof(unsigned long long) * (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_keys, 0xff, sizeof(unsigned long long) * (size_t)n, c->stream));
    const int ns = scene_of(c)->num_spheres;
    if (ns <= 0) return MIRT_OK;
    const int bx = (n + 255) / 256;
    const int want = std::max(1, 8 * std::max(1, c->num_cus) / bx);
    const int chunks = std::min(std::min(want, (ns + 63) / 64), 65535);
    const int chunk = (ns + chunks - 1) / chunks;
    const dim3 grid(bx, (ns + chunk - 1) / chunk);
    const DevScene sc = dev_scene(c);
    const mirt_ray* d_rays = (const mirt_ray*)c->d_in;
    if (c->fast_slab)
        brute_chunk_kernel<true><<<grid, 256, 0, c->stream>>>(sc, d_rays, n, chunk, c->d_keys);
    else
        brute_chunk_kernel<false><<<grid, 256, 0, c->stream>>>(sc, d_rays, n, chunk, c->d_keys);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

}  // namespace

extern "C" {

int mirt_create(int device, mirt_ctx** out)
{
    if (!out) return MIRT_E_INVALID;
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        set_error("mirt_create: device %d not present (%d visible)", device, n);
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(device));
    mirt_ctx* c = new (std::nothrow) mirt_ctx();
    if (!c) {
        set_error("mirt_create: out of host memory");
        return MIRT_E_NOMEM;
    }
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    for (int k = 0; k < kPhaseRing && e == hipSuccess; k++) {
        e = hipEventCreate(&c->ph0[k]);
        if (e == hipSuccess) e = hipEventCreate(&c->ph1[k]);
        if (e == hipSuccess) e = hipEventCreate(&c->ph2[k]);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->slab_free, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_counts, sizeof(mirt_counts));
    if (e == hipSuccess) {
        c->acc = accum_new(device);
        c->slot = new (std::nothrow) SceneSlot();
        if (!c->acc || !c->slot) e = hipErrorOutOfMemory;
        if (c->slot) c->slot->members.push_back(c);
    }
    if (e == hipSuccess) {
        int cus = 0, per_cu = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bounce_kernel<true, 2>, 256,
                                                             bounce_lds_bytes(kMaxDepth));
        c->bounce_blocks = std::max(1, cus) * std::max(1, per_cu);
        c->num_cus = cus;
    }
    if (e != hipSuccess) {
        mirt_destroy(c);
        return hip_fail(e, "mirt_create");
    }
    *out = c;
    return MIRT_OK;
}

void mirt_destroy(mirt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    // a share that lives on must not keep a pending fold of this ctx's slab
    if (c->acc && c->acc->refs > 1 && c->acc->pend_ctx == c) (void)accum_materialize(c->acc, c->stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->launched && c->last_stream != c->stream) (void)hipEventSynchronize(c->done);  // a frame on a caller's stream
    if (c->slab_guard) (void)hipEventSynchronize(c->slab_free);   // another stream's read of the slab
    accum_release(c->acc);
    mirt::build_state_free(c->build);
    mirt::denoise_state_free(c->denoise);
    mirt::reproject_state_free(c->reproject);
    mirt::vfilter_state_free(c->vfilter);
    slot_leave(c);  // its frames are done: the slot's scene lives on with the other members
    for (void* p : {(void*)c->d_out, c->d_in, c->d_res, (void*)c->d_counts, (void*)c->d_defer, c->d_queue,
                    (void*)c->d_keys, (void*)c->d_overlay, c->d_planes, c->d_rays, c->pc.d, c->ps.d, c->d_guides})
        if (p) (void)hipFree(p);
    if (c->ps.h_verdict) (void)hipHostFree(c->ps.h_verdict);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int k = 0; k < kPhaseRing; k++)
        for (hipEvent_t ev : {c->ph0[k], c->ph1[k], c->ph2[k]})
            if (ev) (void)hipEventDestroy(ev);
    if (c->done) (void)hipEventDestroy(c->done);
    if (c->slab_free) (void)hipEventDestroy(c->slab_free);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int mirt_scene_upload_flat(mirt_ctx* c, const mirt_sphere* spheres, int ns, const mirt_node* nodes, int nn)
try {
    if (!ctx_ok(c, false, "mirt_scene_upload_flat")) return MIRT_E_INVALID;
    if (ns < 0 || nn < 0 || (ns > 0 && !spheres) || (nn > 0 && !nodes)) {
        set_error("mirt_scene_upload_flat: invalid arguments");
        return MIRT_E_INVALID;
    }
    // a malformed tree must not send the host layout builders or the kernels
    // out of bounds
    if (int rc = validate_flat(nodes, nn, ns, 0, "mirt_scene_upload_flat")) return rc;
    SceneLayout lay;
    build_scene_layout(spheres, ns, nodes, nn, lay);
    // the device arrays: `alloc` bytes allocated at *dst (0: the array goes
    // `off` bytes into the allocation the row before made), `bytes` copied
    const size_t n1 = nn > 0 ? nn : 1, nl = lay.leaf_box.size();
    Scene* sn = new Scene();
    const struct {
        void** dst;
        size_t alloc, off;
        const void* src;
        size_t bytes;
    } up[] = {
        {(void**)&sn->d_nodes, sizeof(DNode) * n1, 0, lay.dnodes.data(), sizeof(DNode) * (size_t)nn},
        {(void**)&sn->d_nodes32, sizeof(mirt_node) * n1, 0, nodes, sizeof(mirt_node) * (size_t)nn},
        {(void**)&sn->d_geo, sizeof(float4) * lay.geo.size(), 0, lay.geo.data(), sizeof(float4) * lay.geo.size()},
        {(void**)&sn->d_color, sizeof(uint32_t) * lay.color.size(), 0, lay.color.data(),
         sizeof(uint32_t) * lay.color.size()},
        {(void**)&sn->d_pnodes, sizeof(PNode) * lay.pnodes.size(), 0, lay.pnodes.data(),
         sizeof(PNode) * lay.pnodes.size()},
        {(void**)&sn->d_hnodes, sizeof(HNode) * lay.hnodes.size(), 0, lay.hnodes.data(),
         sizeof(HNode) * lay.hnodes.size()},
        {(void**)&sn->d_haux, sizeof(HAux) * lay.haux.size(), 0, lay.haux.data(), sizeof(HAux) * lay.haux.size()},
        {(void**)&sn->d_leaves, lay.leaf_box_off + sizeof(LeafBox) * std::max<size_t>(nl, 1), 0, lay.leaf_geo.data(),
         sizeof(float4) * nl},
        {(void**)&sn->d_leaves, 0, lay.leaf_box_off, lay.leaf_box.data(), sizeof(LeafBox) * nl},
        {(void**)&sn->d_ndepth, lay.ndepth.size(), 0, lay.ndepth.data(), lay.ndepth.size()},
    };
    if (int rc = link_stage(c)) {
        scene_free(sn);
        return rc;
    }
    // the slot gives up the scene it held first, as this call always has: until
    // every array is in place ctx_ok rejects the slot's contexts
    slot_drop_scene(c->slot);
    slot_reap(c->slot, false);
    auto put = [](void** dst, size_t alloc, size_t off, const void* src, size_t bytes) {
        if (alloc) HIP_TRY(hipMalloc(dst, alloc));
        if (bytes) HIP_TRY(hipMemcpy((char*)*dst + off, src, bytes, hipMemcpyHostToDevice));
        return (int)MIRT_OK;
    };
    for (const auto& u : up)
        if (int rc = put(u.dst, u.alloc, u.off, u.src, u.bytes)) {
            scene_free(sn);
            return rc;
        }
    sn->num_nodes = nn;
    sn->num_spheres = ns;
    sn->num_hnodes = (uint32_t)lay.hnodes.size();
    sn->num_pnodes = (uint32_t)lay.pnodes.size();
    sn->num_leaves = (uint32_t)nl;
    sn->leaf_box_off = lay.leaf_box_off;
    sn->leaf_big = lay.leaf_big;
    sn->wide_root = lay.wide_root;
    sn->ordered_ok = lay.ordered;
    sn->prune_ok = lay.encloses;
    sn->r_max = lay.r_max;
    sn->c_max = lay.c_max;
    sn->o_bound = lay.o_bound;
    slot_install(c, sn);
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    set_error("mirt_scene_upload_flat: out of host memory");
    return MIRT_E_NOMEM;
}

int64_t mirt_scene_resident_layout(mirt_ctx* c, int part, void* out, size_t cap, mirt_scene_layout_info* info)
{
    if (!c) {
        set_error("mirt_scene_resident_layout: null context");
        return MIRT_E_INVALID;
    }
    if (!ctx_ok(c, true, "mirt_scene_resident_layout")) return MIRT_E_NOSCENE;
    const Scene* sn = scene_of(c);
    const size_t nn = (size_t)sn->num_nodes, ns1 = (size_t)sn->num_spheres + 1, nl = sn->num_leaves;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (part) {
    case MIRT_LAYOUT_DNODES: src = sn->d_nodes, bytes = sizeof(DNode) * nn; break;
    case MIRT_LAYOUT_GEO: src = sn->d_geo, bytes = sizeof(float4) * ns1; break;
    case MIRT_LAYOUT_COLOR: src = sn->d_color, bytes = sizeof(uint32_t) * ns1; break;
    case MIRT_LAYOUT_PNODES: src = sn->d_pnodes, bytes = sizeof(PNode) * sn->num_pnodes; break;
    case MIRT_LAYOUT_HNODES: src = sn->d_hnodes, bytes = sizeof(HNode) * sn->num_hnodes; break;
    case MIRT_LAYOUT_HAUX: src = sn->d_haux, bytes = sizeof(HAux) * sn->num_hnodes; break;
    case MIRT_LAYOUT_LEAF_GEO: src = sn->d_leaves, bytes = sizeof(float4) * nl; break;
    case MIRT_LAYOUT_LEAF_BOX: src = sn->d_leaves + sn->leaf_box_off, bytes = sizeof(LeafBox) * nl; break;
    case MIRT_LAYOUT_NDEPTH: src = sn->d_ndepth, bytes = std::max<size_t>(nn, 1); break;
    default: set_error("mirt_scene_resident_layout: unknown part %d", part); return MIRT_E_INVALID;
    }
    if (info) {
        info->encloses = sn->prune_ok;
        info->ordered = sn->ordered_ok;
        info->leaf_big = sn->leaf_big;
        info->r_max = sn->r_max;
        info->c_max = sn->c_max;
        info->o_bound = sn->o_bound;
        info->num_pnodes = sn->num_pnodes;
        info->num_hnodes = sn->num_hnodes;
        info->num_leaves = sn->num_leaves;
        info->wide_root = sn->wide_root;
        info->leaf_box_off = sn->leaf_box_off;
    }
    if (out && cap >= bytes && bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    }
    return (int64_t)bytes;
}

int mirt_last_scene_build_stats(mirt_ctx* c, mirt_scene_build_stats* out)
{
    if (!c || !out) {
        set_error("mirt_last_scene_build_stats: null context or output");
        return MIRT_E_INVALID;
    }
    if (!c->have_scene_stats) {
        set_error("mirt_last_scene_build_stats: no mirt_scene_build_device has finished on this context");
        return MIRT_E_INVALID;
    }
    *out = c->scene_stats;
    return MIRT_OK;
}

int mirt_last_refit_stats(mirt_ctx* c, mirt_refit_stats* out)
{
    if (!c || !out) {
        set_error("mirt_last_refit_stats: null context or output");
        return MIRT_E_INVALID;
    }
    if (!c->have_refit_stats) {
        set_error("mirt_last_refit_stats: no mirt_scene_refit_device has finished on this context");
        return MIRT_E_INVALID;
    }
    *out = c->refit_stats;
    return MIRT_OK;
}

int mirt_scene_upload(mirt_ctx* c, const mirt_sphere* spheres, int ns, const mirt_bvh_node* root)
try {
    if (!root) return mirt_scene_upload_flat(c, spheres, ns, nullptr, 0);
    const int nn = mirt_bvh_count(root);
    std::vector<mirt_node> flat((size_t)nn);
    if (mirt_bvh_flatten(root, spheres, flat.data(), nn) != nn) {
        set_error("mirt_scene_upload: flatten failed");
        return MIRT_E_INVALID;
    }
    return mirt_scene_upload_flat(c, spheres, ns, flat.data(), nn);
} catch (const std::bad_alloc&) {
    set_error("mirt_scene_upload: out of host memory");
    return MIRT_E_NOMEM;
}

// mirt_render_frame_device, under the name `fn` of the entry point it serves.
static int render_frame_device(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* d_out,
                               float* d_acc, void* stream, const char* fn)
{
    if (!ctx_ok(c, true, fn)) return MIRT_E_NOSCENE;
    if (!cam || !frame_desc_valid(fd) || !d_out || (fd->accumulate && !d_acc)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (fd->use_bvh && scene_of(c)->num_nodes == 0) {
        set_error("%s: use_bvh set but no tree uploaded", fn);
        return MIRT_E_NOSCENE;
    }
    const FrameConst f = make_frame_const(cam, fd);
    c->frame_cam = *cam;
    return launch_render(c, f, d_out, d_acc, (hipStream_t)stream, false, nullptr);
}

int mirt_render_frame_device(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* d_out,
                             float* d_acc, void* stream)
{
    return render_frame_device(c, cam, fd, d_out, d_acc, stream, "mirt_render_frame_device");
}

}  // extern "C"

namespace {

// The frame of mirt_render_frame up to its D2H copy, enqueued on the ctx's
// stream: `samples` slabs into d_out (the ctx's own buffer when null),
// accumulation in the ctx's (possibly shared) buffer. *d_display = the slab
// that holds the display after the last frame.
int enqueue_frame(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* d_out,
                  uint32_t** d_display, const char* fn, bool independent = false)
{
    if (!ctx_ok(c, true, fn)) return MIRT_E_NOSCENE;
    if (!cam || !frame_desc_valid(fd)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (fd->use_bvh && scene_of(c)->num_nodes == 0) {
        set_error("%s: use_bvh set but no tree uploaded", fn);
        return MIRT_E_NOSCENE;
    }
    const FrameConst f = make_frame_const(cam, fd);
    const size_t pixels = (size_t)f.shard_rows * f.width;  // one frame (several: slab j = display after frame j)
    if (!d_out && c->out_cap < pixels * f.samples * 4 + 4) {
        // the slab is reallocated: a pending fold of it is taken first, and
        // any other stream's read of it has ended
        if (c->acc->pend_ctx == c) {
            if (int rc = accum_materialize(c->acc, c->stream)) return rc;
        }
        if (c->slab_guard) {
            HIP_TRY(hipEventSynchronize(c->slab_free));
            c->slab_guard = false;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (!d_out) {
        int rc = ensure((void**)&c->d_out, &c->out_cap, pixels * f.samples * 4 + 4);
        if (rc) return rc;
        d_out = c->d_out;
    }
    // a new frame geometry starts a fresh accumulation buffer
    int rc = accum_prepare(c->acc, pixels, c->stream);
    if (rc) return rc;
    // independent fresh frames (mirt_multi's launches of several frames): raw
    // slabs, then the last one folded as a fresh frame, so the (possibly
    // shared) accumulation buffer holds what a sequence of fresh frames leaves
    const bool raw = independent && f.samples > 1 && !f.accumulate;
    c->frame_cam = *cam;
    rc = launch_render(c, f, d_out, raw ? nullptr : c->acc->d_acc, c->stream, true, nullptr);
    if (rc) return rc;
    *d_display = d_out + (size_t)(f.samples - 1) * pixels;
    if (raw && pixels) {   // an empty shard (mirt.h) has nothing to fold: a grid of 0 workgroups is no launch
        FrameConst f1 = f;
        f1.samples = 1;
        f1.accumulate = 0;
        AccumShare* chain = accum_chain(c);
        if (chain) {   // this fold is newer than a pending fresh display: that one is dropped
            chain->pend = nullptr;
            chain->pend_ctx = nullptr;
        }
        if (chain && chain->has_fold) HIP_TRY(hipStreamWaitEvent(c->stream, chain->folded, 0));
        fold_samples_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, c->stream>>>(f1, *d_display, c->acc->d_acc);
        HIP_TRY(hipGetLastError());
        if (chain) {
            HIP_TRY(hipEventRecord(chain->folded, c->stream));
            chain->has_fold = true;
        }
        HIP_TRY(hipEventRecord(c->done, c->stream));
    }
    return MIRT_OK;
}

// The frame of mirt_render_frame up to and including its D2H copy, enqueued
// on the ctx's stream.
int enqueue_host_frame(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out,
                       const char* fn)
{
    if (!out) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    uint32_t* disp = nullptr;
    if (int rc = enqueue_frame(c, cam, fd, nullptr, &disp, fn)) return rc;
    // as a 2D copy (rows x width): the runtime takes a DMA engine for it, where a
    // 1D copy of the same bytes often runs as a blit kernel on this stream's
    // compute queue (as multi.hip does)
    const size_t row = (size_t)fd->width * 4, rows = (size_t)shard_row_count(fd);
    if (rows)   // an empty shard (mirt.h) writes nothing through `out`
        HIP_TRY(hipMemcpy2DAsync(out, row, disp, row, row, rows, hipMemcpyDeviceToHost, c->stream));
    return MIRT_OK;
}

}  // namespace

namespace mirt {
int enqueue_frame_device(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* d_out,
                         uint32_t** d_display, const char* fn, bool independent, const mirt_lens* lens)
{
    if (!c || !cam || !lens || !lens_valid(lens) || lens->aperture == 0.0f)   // a plain frame (enqueue_frame checks c, cam)
        return enqueue_frame(c, cam, fd, d_out, d_display, fn, independent);
    const LensConst lc = lens_const(cam, lens);
    c->lens = &lc;
    const int rc = enqueue_frame(c, cam, fd, d_out, d_display, fn, independent);
    c->lens = nullptr;
    return rc;
}
int ctx_device(const mirt_ctx* c) { return c->device; }
int ctx_build_finish(const mirt_ctx* c) { return c->build_finish; }
BuildState** ctx_build_state(mirt_ctx* c) { return &c->build; }
DenoiseState** ctx_denoise_state(mirt_ctx* c) { return &c->denoise; }
int ctx_denoise_tile(const mirt_ctx* c) { return c->denoise_tile; }
ReprojectState** ctx_reproject_state(mirt_ctx* c) { return &c->reproject; }
VfilterState** ctx_vfilter_state(mirt_ctx* c) { return &c->vfilter; }
void ctx_link_intent(mirt_ctx* c, bool rebuilt, const int32_t* d_perm, const int32_t* h_perm)
{
    c->link_intent = true;
    c->link_rebuilt = rebuilt;
    c->link_d_perm = d_perm;
    c->link_h_perm = h_perm;
}
void ctx_link_intent_clear(mirt_ctx* c)
{
    c->link_intent = c->link_rebuilt = false;
    c->link_d_perm = c->link_h_perm = nullptr;
}
int ctx_launch_begin(mirt_ctx* c, hipStream_t s, bool host_wait)
{
    if (c->launched && host_wait) HIP_TRY(hipEventSynchronize(c->done));
    if (c->launched && c->last_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->done, 0));
    return MIRT_OK;
}
int ctx_launch_end(mirt_ctx* c, hipStream_t s)
{
    HIP_TRY(hipEventRecord(c->done, s));
    c->last_stream = s;
    c->launched = true;
    return MIRT_OK;
}
int ctx_install_scene(mirt_ctx* c, const DeviceScene& sc)
{
    Scene* sn = new (std::nothrow) Scene();
    if (!sn) {
        set_error("out of host memory");
        return MIRT_E_NOMEM;
    }
    sn->d_nodes = (DNode*)sc.dnodes;
    sn->d_nodes32 = (mirt_node*)sc.nodes32;
    sn->d_geo = (float4*)sc.geo;
    sn->d_color = (uint32_t*)sc.color;
    sn->d_pnodes = (PNode*)sc.pnodes;
    sn->d_hnodes = (HNode*)sc.hnodes;
    sn->d_haux = (HAux*)sc.haux;
    sn->d_leaves = (char*)sc.leaves;
    sn->d_ndepth = (uint8_t*)sc.ndepth;
    sn->num_nodes = sc.num_nodes;
    sn->num_hnodes = sc.num_hnodes;
    sn->num_pnodes = sc.num_pnodes;
    sn->num_leaves = sc.num_leaves;
    sn->leaf_box_off = sc.leaf_box_off;
    sn->leaf_big = sc.leaf_big;
    sn->wide_root = sc.wide_root;
    sn->ordered_ok = sc.ordered;
    sn->prune_ok = sc.encloses;
    sn->r_max = sc.r_max;
    sn->c_max = sc.c_max;
    sn->o_bound = sc.o_bound;
    sn->num_spheres = sc.num_spheres;
    if (int rc = link_stage(c)) {
        delete sn;   // (the arrays stay the caller's)
        return rc;
    }
    slot_install(c, sn);
    return MIRT_OK;
}
bool ctx_shares_scene(const mirt_ctx* a, const mirt_ctx* b) { return a && b && a->slot == b->slot; }
void ctx_set_scene_stats(mirt_ctx* c, const mirt_scene_build_stats& st)
{
    c->scene_stats = st;
    c->have_scene_stats = true;
}
bool ctx_resident_scene(const mirt_ctx* c, ResidentScene* out)
{
    const Scene* sn = scene_of(c);
    if (sn->num_spheres < 0) return false;
    *out = ResidentScene{sn->d_nodes32, sn->d_ndepth, sn->num_nodes, sn->num_spheres, sn->ordered_ok};
    return true;
}
void ctx_set_refit_stats(mirt_ctx* c, const mirt_refit_stats& st)
{
    c->refit_stats = st;
    c->have_refit_stats = true;
}
bool ctx_base_cost(const mirt_ctx* c, double* cost)
{
    if (c->slot->have_base_cost) *cost = c->slot->base_cost;
    return c->slot->have_base_cost;
}
void ctx_set_base_cost(mirt_ctx* c, double cost)
{
    c->slot->base_cost = cost;
    c->slot->have_base_cost = true;
}
}  // namespace mirt

extern "C" {

namespace {

// The device-visible address of a page-locked host range (mirt_host_alloc /
// mirt_host_register memory), or null for pageable memory -- and for a range
// that spans separately registered pieces: the device mapping must be ONE
// contiguous range (the last byte's device address = the first's + bytes - 1),
// else the kernels' stores would land elsewhere (the copy path takes it).
uint32_t* host_mapped(const void* p, size_t bytes)
{
    hipPointerAttribute_t a, b;
    if (!bytes) return nullptr;   // an empty shard's output: nothing to store, and no last byte to look up
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost || !a.devicePointer ||
        hipPointerGetAttributes(&b, (const char*)p + bytes - 1) != hipSuccess || b.type != hipMemoryTypeHost ||
        (const char*)b.devicePointer != (const char*)a.devicePointer + bytes - 1) {
        (void)hipGetLastError();   // a pageable pointer is an error to the query, not to the caller
        return nullptr;
    }
    return (uint32_t*)a.devicePointer;
}

}  // namespace

extern "C++" {
namespace mirt {
// The device-visible address of a page-locked host range (null if it is not
// one contiguous mapping): mirt_multi's copy kernels store into it.
uint32_t* host_device_ptr(const void* p, size_t bytes) { return host_mapped(p, bytes); }
// Before a caller frees or reallocates an external slab ctx c rendered into:
// a pending fold of it is taken now and every read of it has ended.
int accum_settle(mirt_ctx* c)
{
    if (c->acc && c->acc->pend_ctx == c) {
        if (int rc = accum_materialize(c->acc, c->stream)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->slab_guard) {
        HIP_TRY(hipEventSynchronize(c->slab_free));
        c->slab_guard = false;
    }
    return MIRT_OK;
}
// Page-locked ranges this library handed out or registered (mirt_host_alloc /
// mirt_host_register): checked without a HIP call, which the frame loops of
// mirt_multi make for every output of every launch.
static std::mutex g_pin_mu;
static std::map<uintptr_t, size_t> g_pinned;   // start -> bytes
void pinned_add(const void* p, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pinned[(uintptr_t)p] = bytes;
}
void pinned_remove(const void* p)
{
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pinned.erase((uintptr_t)p);
}
bool host_page_locked(const void* p, size_t bytes)
{
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pinned.upper_bound((uintptr_t)p);
        if (it != g_pinned.begin()) {
            --it;
            if ((uintptr_t)p + bytes <= it->first + it->second) return true;
        }
    }
    return host_mapped(p, bytes) != nullptr;   // pinned by other means (e.g. the caller's hipHostMalloc)
}
}  // namespace mirt
}

// The frame and the delivery of its display to `out`, enqueued on the ctx's
// stream. in_place and a page-locked destination (the recipe for main.c's
// reused frame buffer: mirt_host_register): the frame kernels store each
// pixel straight into it, so the frame is in host memory when they end -- no
// copy after them (one frame, the ctx's own accumulation: nothing reads the
// output back)
static int enqueue_frame_to_host(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out,
                                 bool in_place, const char* fn)
{
    if (c && in_place && out && frame_desc_valid(fd) && fd->samples <= 1 && !accum_chain(c)) {
        if (uint32_t* d = host_mapped(out, (size_t)shard_row_count(fd) * fd->width * 4)) {
            uint32_t* disp = nullptr;
            return enqueue_frame(c, cam, fd, d, &disp, fn);
        }
    }
    return enqueue_host_frame(c, cam, fd, out, fn);
}

// The blocking call renders one frame with nothing after it on the ctx: its
// first bounces go to the queue in tile order (lone_frame), which the
// bounce pass walks 2-4% faster when no other frame shares the chip.
static int render_frame_blocking(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out,
                                 const char* fn)
{
    if (c) c->lone_frame = true;
    const int rc = enqueue_frame_to_host(c, cam, fd, out, c && c->zero_copy, fn);
    if (c) c->lone_frame = false;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    // (an empty shard records no events: last_ms stays the last timed frame's)
    if (c->timed_recorded) HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_render_frame(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out)
{
    return render_frame_blocking(c, cam, fd, out, "mirt_render_frame");
}

int mirt_render_frame_async(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out)
{
    // MIRT_OPT_ZERO_COPY 2: frames in flight into page-locked memory are
    // written in place too (no DMA behind each frame's kernels)
    return enqueue_frame_to_host(c, cam, fd, out, c && c->zero_copy == 2, "mirt_render_frame_async");
}

// ---- frames with planes (mirt_primary_planes)

// What the planes forms check on top of their plain siblings, before the ctx
// is used and before any HIP call.
static bool planes_args_ok(const mirt_ctx* c, const mirt_frame_desc* fd, const mirt_primary_planes* pl, const char* fn)
{
    if (!c) {
        set_error("%s: null context", fn);
        return false;
    }
    if (!pl || !(pl->t || pl->sphere || pl->normal) || (fd && fd->max_depth < 1)) {
        set_error("%s: invalid arguments", fn);
        return false;
    }
    return true;
}

int mirt_render_frame_planes_device(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* d_out,
                                    float* d_acc, const mirt_primary_planes* d_planes, void* stream)
{
    if (!planes_args_ok(c, fd, d_planes, "mirt_render_frame_planes_device")) return MIRT_E_INVALID;
    c->planes = Planes{d_planes->t, d_planes->sphere, d_planes->normal};
    const int rc = mirt_render_frame_device(c, cam, fd, d_out, d_acc, stream);
    c->planes = Planes{};
    return rc;
}

// The blocking and async forms: the frame stores its planes into device
// memory the ctx keeps (grown by `ensure`, never freed per frame), the
// members the caller asked for one after another, and they are copied to the
// caller's host pointers behind the frame on the ctx's stream.
static int render_frame_planes_host(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out,
                                    const mirt_primary_planes* pl, bool blocking, const char* fn)
{
    if (!planes_args_ok(c, fd, pl, fn)) return MIRT_E_INVALID;
    if (!ctx_ok(c, true, fn)) return MIRT_E_NOSCENE;
    if (!cam || !frame_desc_valid(fd) || !out) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    const size_t n = (size_t)shard_row_count(fd) * fd->width * (fd->samples > 1 ? fd->samples : 1);
    const size_t off_s = pl->t ? 4 * n : 0, off_n = off_s + (pl->sphere ? 4 * n : 0);
    const size_t bytes = off_n + (pl->normal ? 12 * n : 0);
    // the buffer grows: an earlier frame's copies out of it have ended first
    if (bytes > c->planes_cap) HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = ensure(&c->d_planes, &c->planes_cap, bytes)) return rc;
    char* const d = (char*)c->d_planes;
    c->planes = Planes{pl->t ? (float*)d : nullptr, pl->sphere ? (int32_t*)(d + off_s) : nullptr,
                       pl->normal ? (float*)(d + off_n) : nullptr};
    const Planes dev = c->planes;
    c->lone_frame = blocking;
    const int rc = enqueue_frame_to_host(c, cam, fd, out, blocking ? c->zero_copy != 0 : c->zero_copy == 2, fn);
    c->lone_frame = false;
    c->planes = Planes{};
    if (rc) return rc;
    if (n) {
        if (pl->t) HIP_TRY(hipMemcpyAsync(pl->t, dev.t, 4 * n, hipMemcpyDeviceToHost, c->stream));
        if (pl->sphere) HIP_TRY(hipMemcpyAsync(pl->sphere, dev.sphere, 4 * n, hipMemcpyDeviceToHost, c->stream));
        if (pl->normal) HIP_TRY(hipMemcpyAsync(pl->normal, dev.normal, 12 * n, hipMemcpyDeviceToHost, c->stream));
    }
    if (!blocking) return MIRT_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->timed_recorded) HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_render_frame_planes(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out,
                             const mirt_primary_planes* planes)
{
    return render_frame_planes_host(c, cam, fd, out, planes, true, "mirt_render_frame_planes");
}

int mirt_render_frame_planes_async(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_rgba8* out,
                                   const mirt_primary_planes* planes)
{
    return render_frame_planes_host(c, cam, fd, out, planes, false, "mirt_render_frame_planes_async");
}

// ---- ray frames (caller-given camera rays)

// What the ray forms check before the ctx is used and before any HIP call.
static bool rays_args_ok(const mirt_ctx* c, const mirt_ray* rays, const mirt_frame_desc* fd,
                         const mirt_primary_planes* pl, const char* fn)
{
    if (!c) {
        set_error("%s: null context", fn);
        return false;
    }
    if (!rays || !frame_desc_valid(fd) || fd->jitter ||
        (pl && (!(pl->t || pl->sphere || pl->normal) || fd->max_depth < 1))) {
        set_error("%s: invalid arguments", fn);
        return false;
    }
    return true;
}

// A ray frame has no camera: FrameConst's camera fields are never read by its
// kernels, nor by the bounce pass, the folds or the row map.
static const mirt_camera kNoCamera{};

int mirt_render_rays_device(mirt_ctx* c, const mirt_ray* d_rays, const mirt_frame_desc* fd, uint32_t* d_out,
                            float* d_acc, const mirt_primary_planes* d_planes, void* stream)
{
    const char* fn = "mirt_render_rays_device";
    if (!rays_args_ok(c, d_rays, fd, d_planes, fn)) return MIRT_E_INVALID;
    c->rays = d_rays;
    if (d_planes) c->planes = Planes{d_planes->t, d_planes->sphere, d_planes->normal};
    const int rc = render_frame_device(c, &kNoCamera, fd, d_out, d_acc, stream, fn);
    c->planes = Planes{};
    c->rays = nullptr;
    return rc;
}

int mirt_render_rays(mirt_ctx* c, const mirt_ray* rays, const mirt_frame_desc* fd, mirt_rgba8* out,
                     const mirt_primary_planes* planes)
{
    const char* fn = "mirt_render_rays";
    if (!rays_args_ok(c, rays, fd, planes, fn)) return MIRT_E_INVALID;
    if (!ctx_ok(c, true, fn)) return MIRT_E_NOSCENE;
    if (!out) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    const size_t bytes = sizeof(mirt_ray) * (size_t)shard_row_count(fd) * fd->width * (fd->samples > 1 ? fd->samples : 1);
    // the blocking call leaves nothing in flight that reads the buffer: it may grow at once
    if (int rc = ensure(&c->d_rays, &c->rays_cap, bytes)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(c->d_rays, rays, bytes, hipMemcpyHostToDevice, c->stream));
    // (an empty shard launches nothing: its rays are not read, wherever they are)
    c->rays = bytes ? (const mirt_ray*)c->d_rays : rays;
    const int rc = planes ? render_frame_planes_host(c, &kNoCamera, fd, out, planes, true, fn)
                          : render_frame_blocking(c, &kNoCamera, fd, out, fn);
    c->rays = nullptr;
    return rc;
}

// ---- lens frames (a thin lens computed in the frame's own camera pass)

static_assert(MIRT_PCACHE_LENS == 10, "mirt.h: the reasons' values are ABI");

// What the lens forms check before the ctx is used and before any HIP call.
static bool lens_args_ok(const mirt_ctx* c, const mirt_camera* cam, const mirt_lens* lens, const mirt_frame_desc* fd,
                         const mirt_primary_planes* pl, const char* fn)
{
    if (!c) {
        set_error("%s: null context", fn);
        return false;
    }
    if (!cam || !lens_valid(lens) || !frame_desc_valid(fd) ||
        (pl && (!(pl->t || pl->sphere || pl->normal) || fd->max_depth < 1))) {
        set_error("%s: invalid arguments", fn);
        return false;
    }
    return true;
}

int mirt_render_lens_frame_device(mirt_ctx* c, const mirt_camera* cam, const mirt_lens* lens, const mirt_frame_desc* fd,
                                  uint32_t* d_out, float* d_acc, const mirt_primary_planes* d_planes, void* stream)
{
    const char* fn = "mirt_render_lens_frame_device";
    if (!lens_args_ok(c, cam, lens, fd, d_planes, fn)) return MIRT_E_INVALID;
    if (lens->aperture == 0.0f)   // the pinhole, by definition: the plain frame
        return d_planes ? mirt_render_frame_planes_device(c, cam, fd, d_out, d_acc, d_planes, stream)
                        : mirt_render_frame_device(c, cam, fd, d_out, d_acc, stream);
    const LensConst lc = lens_const(cam, lens);
    c->lens = &lc;
    if (d_planes) c->planes = Planes{d_planes->t, d_planes->sphere, d_planes->normal};
    const int rc = render_frame_device(c, cam, fd, d_out, d_acc, stream, fn);
    c->planes = Planes{};
    c->lens = nullptr;
    return rc;
}

int mirt_render_lens_frame(mirt_ctx* c, const mirt_camera* cam, const mirt_lens* lens, const mirt_frame_desc* fd,
                           mirt_rgba8* out, const mirt_primary_planes* planes)
{
    const char* fn = "mirt_render_lens_frame";
    if (!lens_args_ok(c, cam, lens, fd, planes, fn)) return MIRT_E_INVALID;
    if (lens->aperture == 0.0f)
        return planes ? mirt_render_frame_planes(c, cam, fd, out, planes) : mirt_render_frame(c, cam, fd, out);
    const LensConst lc = lens_const(cam, lens);
    c->lens = &lc;
    const int rc = planes ? render_frame_planes_host(c, cam, fd, out, planes, true, fn)
                          : render_frame_blocking(c, cam, fd, out, fn);
    c->lens = nullptr;
    return rc;
}

int mirt_render_lens_frame_async(mirt_ctx* c, const mirt_camera* cam, const mirt_lens* lens, const mirt_frame_desc* fd,
                                 mirt_rgba8* out, const mirt_primary_planes* planes)
{
    const char* fn = "mirt_render_lens_frame_async";
    if (!lens_args_ok(c, cam, lens, fd, planes, fn)) return MIRT_E_INVALID;
    if (lens->aperture == 0.0f)
        return planes ? mirt_render_frame_planes_async(c, cam, fd, out, planes)
                      : mirt_render_frame_async(c, cam, fd, out);
    const LensConst lc = lens_const(cam, lens);
    c->lens = &lc;   // read while the frame is enqueued: the kernels take the struct by value
    const int rc = planes ? render_frame_planes_host(c, cam, fd, out, planes, false, fn)
                          : enqueue_frame_to_host(c, cam, fd, out, c->zero_copy == 2, fn);
    c->lens = nullptr;
    return rc;
}

int mirt_lens_rays(mirt_ctx* c, const mirt_camera* cam, const mirt_lens* lens, const mirt_frame_desc* fd,
                   mirt_ray* out)
{
    const char* fn = "mirt_lens_rays";
    if (!lens_args_ok(c, cam, lens, fd, nullptr, fn)) return MIRT_E_INVALID;
    if (!out) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (lens->aperture == 0.0f) return mirt_camera_rays(c, cam, fd, out);
    if (!ctx_ok(c, false, fn)) return MIRT_E_INVALID;
    const FrameConst f = make_frame_const(cam, fd);
    const LensConst lc = lens_const(cam, lens);
    const size_t bytes = (size_t)f.num_rows * f.width * sizeof(mirt_ray);
    if (int rc = ensure(&c->d_res, &c->res_cap, bytes + 4)) return rc;
    if (f.num_rows > 0) {
        lens_rays_kernel<<<dim3((f.width + 255) / 256, f.num_rows), 256, 0, c->stream>>>(f, lc, (mirt_ray*)c->d_res);
        HIP_TRY(hipGetLastError());
    }
    if (bytes) HIP_TRY(hipMemcpyAsync(out, c->d_res, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

// ---- a frame and its filtered display (csrc/denoise.h)

int mirt_render_frame_denoised(mirt_ctx* c, const mirt_camera* cam, const mirt_lens* lens, const mirt_frame_desc* fd,
                               const mirt_denoise_params* params, mirt_rgba8* out, mirt_rgba8* raw)
{
    const char* fn = "mirt_render_frame_denoised";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!cam || !frame_desc_valid(fd) || (lens && !lens_valid(lens)) || !denoise_params_valid(params) || !out ||
        fd->num_shards != 1 || fd->max_depth < 1) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (accum_chain(c)) {
        set_error("%s: the context shares its accumulation buffer (mirt_ctx_share_accum)", fn);
        return MIRT_E_INVALID;
    }
    if (!ctx_ok(c, true, fn)) return MIRT_E_NOSCENE;
    // the planes of the frame's `samples` slabs, spheres then normals, then
    // the filtered display; the filter is guided by the last slab's planes,
    // those of the frame its source shows
    const size_t n = (size_t)fd->width * fd->height, slabs = fd->samples > 1 ? fd->samples : 1;
    // (the blocking call leaves nothing in flight that uses the buffer: it may grow at once)
    if (int rc = ensure(&c->d_guides, &c->guides_cap, 16 * n * slabs + 4 * n)) return rc;
    int32_t* const d_sphere = (int32_t*)c->d_guides;
    float* const d_normal = (float*)(d_sphere + n * slabs);
    uint32_t* const d_filtered = (uint32_t*)(d_normal + 3 * n * slabs);
    const size_t row = (size_t)fd->width * 4;   // copies out as enqueue_host_frame's: rows x width
    const LensConst lc = lens ? lens_const(cam, lens) : LensConst{};
    if (lens && lens->aperture != 0.0f) c->lens = &lc;   // aperture 0 is the pinhole: the plain frame
    c->planes = Planes{nullptr, d_sphere, d_normal};
    c->lone_frame = true;
    uint32_t* disp = nullptr;
    int rc = enqueue_frame(c, cam, fd, nullptr, &disp, fn);
    c->lone_frame = false;
    c->planes = Planes{};
    c->lens = nullptr;
    if (rc) return rc;
    // the source: the accumulation buffer as the frame's last fold left it
    // (the ctx's own: its frames store into it on this stream), with that
    // frame's divisor, or the last slab's display
    const int frames = fd->accumulate ? fd->frames + (int)slabs - 1 : 1;
    rc = denoise_enqueue(c, fd->width, fd->height, fd->accumulate ? nullptr : disp,
                         fd->accumulate ? c->acc->d_acc : nullptr, frames, d_sphere + n * (slabs - 1),
                         d_normal + 3 * n * (slabs - 1), params, d_filtered, nullptr, c->stream, fn);
    if (rc) return rc;
    // both copies behind the filter (it leaves the display slab alone): a copy
    // into pageable memory holds the host, and the filter's launches with it
    if (raw) HIP_TRY(hipMemcpy2DAsync(raw, row, disp, row, row, (size_t)fd->height, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpy2DAsync(out, row, d_filtered, row, row, (size_t)fd->height, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->timed_recorded) HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

// ---- a frame and the display of its reprojected history (csrc/reproject.h)

// vp: null (mirt_render_frame_reprojected: `out` is the history's display), or the parameters of the
// variance-guided filter (mirt_render_frame_reprojected_denoised: `out` is its display, `reprojected` the history's)
static int frame_reprojected(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd,
                             const mirt_reproject_params* params, const mirt_denoise_var_params* vp, bool filtered,
                             mirt_rgba8* out, mirt_rgba8* reprojected, mirt_rgba8* raw, const char* fn)
{
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!cam || !frame_desc_valid(fd) || !reproject_params_valid(params) || (filtered && !vfilter_params_ok(vp)) ||
        !out || fd->accumulate != 0 || fd->samples > 1 || fd->num_shards != 1 || fd->jitter != 0 || fd->max_depth < 1) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (accum_chain(c)) {
        set_error("%s: the context shares its accumulation buffer (mirt_ctx_share_accum)", fn);
        return MIRT_E_INVALID;
    }
    if (!ctx_ok(c, true, fn)) return MIRT_E_NOSCENE;
    float* d_t = nullptr;
    int32_t* d_sphere = nullptr;
    // the slot's link, if this ctx may use it and it ends at the resident scene (reproject_frame_begin decides by its start)
    const Scene* sn = scene_of(c);
    const HistoryLink& lk = c->slot->link;
    const bool linked = c->history_motion == 1 && lk.valid && lk.to == sn->id && lk.n == sn->num_spheres;
    const mirt_sphere_motion motion{(const float*)sn->d_geo, linked ? lk.geo_prev(lk.half) : nullptr,
                                    linked && lk.rebuilt ? lk.perm(lk.half) : nullptr, sn->num_spheres, lk.n};
    float* d_normal = nullptr;
    if (int rc = reproject_frame_begin(c, fd->width, fd->height, sn->id, linked ? lk.from : 0, &d_t, &d_sphere, fn,
                                       filtered, &d_normal))
        return rc;
    c->planes = Planes{d_t, d_sphere, d_normal};
    c->lone_frame = true;
    uint32_t* disp = nullptr;
    int rc = enqueue_frame(c, cam, fd, nullptr, &disp, fn);
    c->lone_frame = false;
    c->planes = Planes{};
    if (rc) return rc;
    const uint32_t* shown = nullptr;
    rc = reproject_frame_end(c, cam, disp, params, linked ? &motion : nullptr, &shown, c->stream, filtered);
    if (rc) return rc;
    // (the filter reads the new records and leaves them, and both displays, alone)
    const uint32_t* d_filtered = nullptr;
    if (filtered)
        if ((rc = reproject_frame_filter(c, vp, &d_filtered, c->stream, fn))) return rc;
    const size_t row = (size_t)fd->width * 4;   // copies out as enqueue_host_frame's: rows x width
    if (raw) HIP_TRY(hipMemcpy2DAsync(raw, row, disp, row, row, (size_t)fd->height, hipMemcpyDeviceToHost, c->stream));
    if (filtered && reprojected)
        HIP_TRY(hipMemcpy2DAsync(reprojected, row, shown, row, row, (size_t)fd->height, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpy2DAsync(out, row, filtered ? d_filtered : shown, row, row, (size_t)fd->height,
                             hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->timed_recorded) HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_render_frame_reprojected(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd,
                                  const mirt_reproject_params* params, mirt_rgba8* out, mirt_rgba8* raw)
{
    return frame_reprojected(c, cam, fd, params, nullptr, false, out, nullptr, raw, "mirt_render_frame_reprojected");
}

int mirt_render_frame_reprojected_denoised(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd,
                                           const mirt_reproject_params* params, const mirt_denoise_var_params* vp,
                                           mirt_rgba8* out, mirt_rgba8* reprojected, mirt_rgba8* raw)
{
    return frame_reprojected(c, cam, fd, params, vp, true, out, reprojected, raw,
                             "mirt_render_frame_reprojected_denoised");
}

int mirt_ctx_wait(mirt_ctx* c)
{
    if (!ctx_ok(c, false, "mirt_ctx_wait")) return MIRT_E_INVALID;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->timed_recorded) HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_host_alloc(size_t bytes, void** out)
{
    if (!out) return MIRT_E_INVALID;
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable));   // pinned for every device (mirt_multi host-direct)
    mirt::pinned_add(*out, bytes ? bytes : 1);
    return MIRT_OK;
}

void mirt_host_free(void* p)
{
    if (!p) return;
    mirt::pinned_remove(p);
    (void)hipHostFree(p);
}

int mirt_host_register(void* p, size_t bytes)
{
    if (!p || !bytes) {
        set_error("mirt_host_register: invalid arguments");
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable));
    mirt::pinned_add(p, bytes);
    return MIRT_OK;
}

int mirt_host_unregister(void* p)
{
    if (!p) {
        set_error("mirt_host_unregister: null pointer");
        return MIRT_E_INVALID;
    }
    mirt::pinned_remove(p);
    HIP_TRY(hipHostUnregister(p));
    return MIRT_OK;
}

int mirt_accum_download(mirt_ctx* c, float* out, size_t count)
{
    if (!ctx_ok(c, false, "mirt_accum_download") || !out) return MIRT_E_INVALID;
    AccumShare* a = c->acc;
    if (count > a->pixels * 3) {
        set_error("mirt_accum_download: %zu floats requested, %zu held", count, a->pixels * 3);
        return MIRT_E_INVALID;
    }
    // after every fold enqueued so far, whichever ctx's stream carries it
    if (int rc = accum_materialize(a, c->stream)) return rc;
    if (a->has_fold) HIP_TRY(hipStreamWaitEvent(c->stream, a->folded, 0));
    HIP_TRY(hipMemcpyAsync(out, a->d_acc, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_ctx_share_accum(mirt_ctx* c, mirt_ctx* owner)
{
    if (!ctx_ok(c, false, "mirt_ctx_share_accum")) return MIRT_E_INVALID;
    if (owner && owner->device != c->device) {
        set_error("mirt_ctx_share_accum: ctxs on devices %d and %d", c->device, owner->device);
        return MIRT_E_INVALID;
    }
    AccumShare* next = owner && owner != c ? owner->acc : nullptr;
    if (next == c->acc || (!next && c->acc->refs == 1)) return MIRT_OK;  // already so / already private
    if (!next) {
        next = accum_new(c->device);
        if (!next) {
            set_error("mirt_ctx_share_accum: out of host memory");
            return MIRT_E_NOMEM;
        }
    } else {
        if (next->refs == 1) {
            // the owner's frames enqueued while its buffer was private wrote
            // it directly (store_pixel) and recorded no fold event: from now
            // on every fold, on any stream, must follow them
            if (next->has_fold) HIP_TRY(hipStreamWaitEvent(owner->stream, next->folded, 0));
            HIP_TRY(hipEventRecord(next->folded, owner->stream));
            next->has_fold = true;
        }
        next->refs++;
    }
    // c's frames enqueued so far still use its old buffer (and a pending
    // fold of c's slab is taken into it before c leaves)
    if (c->acc->pend_ctx == c) {
        if (int rc = accum_materialize(c->acc, c->stream)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->slab_guard) {
        HIP_TRY(hipEventSynchronize(c->slab_free));
        c->slab_guard = false;
    }
    accum_release(c->acc);
    c->acc = next;
    return MIRT_OK;
}

int mirt_ctx_share_scene(mirt_ctx* c, mirt_ctx* owner)
try {
    if (!c) {
        set_error("mirt_ctx_share_scene: null context");
        return MIRT_E_INVALID;
    }
    if (!ctx_ok(c, false, "mirt_ctx_share_scene")) return MIRT_E_INVALID;
    if (owner && owner->device != c->device) {
        set_error("mirt_ctx_share_scene: ctxs on devices %d and %d", c->device, owner->device);
        return MIRT_E_INVALID;
    }
    SceneSlot* next = owner && owner != c ? owner->slot : nullptr;
    if (next == c->slot || (!next && c->slot->members.size() == 1)) return MIRT_OK;  // already so / already private
    // c's frames enqueued so far read its old slot's scene: once they are
    // done, that slot need not follow c's stream any longer
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
    if (!next) {
        // a private slot again, holding the scene the group has now: the
        // arrays stay shared (and read-only) until either slot's next install
        next = new SceneSlot();
        next->cur = c->slot->cur;
        if (next->cur) next->cur->refs++;
        next->base_cost = c->slot->base_cost;
        next->have_base_cost = c->slot->have_base_cost;
    }
    next->members.reserve(next->members.size() + 1);
    slot_leave(c);
    next->members.push_back(c);
    c->slot = next;
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    set_error("mirt_ctx_share_scene: out of host memory");
    return MIRT_E_NOMEM;
}

int mirt_history_motion_get(mirt_ctx* c, mirt_history_motion* out)
{
    if (!c || !out) {
        set_error("mirt_history_motion_get: invalid arguments");
        return MIRT_E_INVALID;
    }
    *out = mirt_history_motion{};
    const HistoryLink& lk = c->slot->link;
    out->bytes = lk.cap;
    if (lk.valid) {
        out->from_scene_id = lk.from;
        out->to_scene_id = lk.to;
        out->rebuilt = lk.rebuilt ? 1 : 0;
    }
    out->carried = reproject_last_carried(c) ? 1 : 0;
    return MIRT_OK;
}

uint64_t mirt_ctx_scene_id(mirt_ctx* c)
{
    return c ? scene_of(c)->id : 0;
}

int mirt_count_frame(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_counts* out)
{
    if (!ctx_ok(c, true, "mirt_count_frame")) return MIRT_E_NOSCENE;
    if (!cam || !frame_desc_valid(fd) || !out) {
        set_error("mirt_count_frame: invalid arguments");
        return MIRT_E_INVALID;
    }
    const FrameConst f = make_frame_const(cam, fd);
    const size_t pixels = (size_t)f.num_rows * f.width;
    int rc = ensure((void**)&c->d_out, &c->out_cap, pixels * 4 + 4);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_counts, 0, sizeof(mirt_counts), c->stream));
    FrameConst f2 = f;
    f2.accumulate = 0;
    rc = launch_render(c, f2, c->d_out, nullptr, c->stream, false, c->d_counts);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_counts, sizeof(mirt_counts), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_wave_stats(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* out, int cap)
{
    if (!ctx_ok(c, true, "mirt_wave_stats")) return MIRT_E_NOSCENE;
    if (!cam || !frame_desc_valid(fd)) {
        set_error("mirt_wave_stats: invalid arguments");
        return MIRT_E_INVALID;
    }
    FrameConst f = make_frame_const(cam, fd);
    f.accumulate = 0;
    const int waves = ((f.width + 7) / 8) * ((f.num_rows + 7) / 8);
    if (!out || cap < waves) return -waves;
    const size_t pixels = (size_t)f.num_rows * f.width;
    int rc = ensure((void**)&c->d_out, &c->out_cap, pixels * 4 + 4);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, 16 * (size_t)waves + 64);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_counts, 0, sizeof(mirt_counts), c->stream));
    rc = launch_render(c, f, c->d_out, nullptr, c->stream, false, c->d_counts, (uint32_t*)c->d_res);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_res, 16 * (size_t)waves, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return waves;
}

int mirt_bounce_stats(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint64_t* out, int cap)
{
    if (!ctx_ok(c, true, "mirt_bounce_stats")) return MIRT_E_NOSCENE;
    if (!cam || !frame_desc_valid(fd) || !fd->use_bvh || fd->max_depth < 2 || c->trav != kTravWavefront) {
        set_error("mirt_bounce_stats: needs a BVH frame of depth >= 2 under the wavefront schedule");
        return MIRT_E_INVALID;
    }
    const int waves = (c->bounce_blocks_opt ? c->bounce_blocks_opt : c->bounce_blocks) * 4;
    if (!out || cap < waves) return -waves;
    FrameConst f = make_frame_const(cam, fd);
    f.accumulate = 0;
    const size_t pixels = (size_t)f.num_rows * f.width;
    int rc = ensure((void**)&c->d_out, &c->out_cap, pixels * 4 + 4);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, 8 * kBounceDiag * (size_t)waves + 64);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_res, 0, 8 * kBounceDiag * (size_t)waves, c->stream));
    rc = launch_render(c, f, c->d_out, nullptr, c->stream, false, nullptr, nullptr, (uint64_t*)c->d_res);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_res, 8 * kBounceDiag * (size_t)waves, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return waves;
}

int mirt_camera_rays(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, mirt_ray* out)
{
    if (!ctx_ok(c, false, "mirt_camera_rays")) return MIRT_E_INVALID;
    if (!cam || !frame_desc_valid(fd) || !out) {
        set_error("mirt_camera_rays: invalid arguments");
        return MIRT_E_INVALID;
    }
    const FrameConst f = make_frame_const(cam, fd);
    const size_t bytes = (size_t)f.num_rows * f.width * sizeof(mirt_ray);
    int rc = ensure(&c->d_res, &c->res_cap, bytes + 4);
    if (rc) return rc;
    if (f.num_rows > 0) {
        camera_rays_kernel<<<dim3((f.width + 255) / 256, f.num_rows), 256, 0, c->stream>>>(f, (mirt_ray*)c->d_res);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(out, c->d_res, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_trace_rays(mirt_ctx* c, const mirt_ray* rays, int n, int depth, int use_bvh, uint64_t seed,
                    uint32_t sample, mirt_rgba8* out)
{
    return mirt_trace_rays_at(c, rays, n, depth, use_bvh, seed, sample, 0, out);
}

int mirt_trace_rays_at(mirt_ctx* c, const mirt_ray* rays, int n, int depth, int use_bvh, uint64_t seed,
                       uint32_t sample, uint32_t pixel0, mirt_rgba8* out)
{
    if (!ctx_ok(c, true, "mirt_trace_rays")) return MIRT_E_NOSCENE;
    if (n < 0 || (n > 0 && (!rays || !out)) || depth < 0 || depth > kMaxDepth) {
        set_error("mirt_trace_rays: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (use_bvh && scene_of(c)->num_nodes == 0) {
        set_error("mirt_trace_rays: use_bvh set but no tree uploaded");
        return MIRT_E_NOSCENE;
    }
    if (n == 0) return MIRT_OK;
    int rc = ensure(&c->d_in, &c->in_cap, sizeof(mirt_ray) * (size_t)n);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, 4 * (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_in, rays, sizeof(mirt_ray) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    {
        const dim3 g((n + 255) / 256), b(256);
        const DevScene sc = dev_scene(c);
        const mirt_ray* in = (const mirt_ray*)c->d_in;
        uint32_t* res = (uint32_t*)c->d_res;
        if (c->fast_slab)
            trace_rays_kernel<true><<<g, b, 0, c->stream>>>(sc, in, n, depth, use_bvh, seed, sample, pixel0, res);
        else
            trace_rays_kernel<false><<<g, b, 0, c->stream>>>(sc, in, n, depth, use_bvh, seed, sample, pixel0, res);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_res, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_intersect_rays(mirt_ctx* c, const mirt_ray* rays, int n, int use_bvh, mirt_hit* out)
{
    if (!ctx_ok(c, true, "mirt_intersect_rays")) return MIRT_E_NOSCENE;
    if (n < 0 || (n > 0 && (!rays || !out))) {
        set_error("mirt_intersect_rays: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (use_bvh && scene_of(c)->num_nodes == 0) {
        set_error("mirt_intersect_rays: use_bvh set but no tree uploaded");
        return MIRT_E_NOSCENE;
    }
    if (n == 0) return MIRT_OK;
    int rc = ensure(&c->d_in, &c->in_cap, sizeof(mirt_ray) * (size_t)n);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, sizeof(mirt_hit) * (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_in, rays, sizeof(mirt_ray) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    const int bt = batch_threads(c, n);
    if (!use_bvh) {
        rc = launch_brute(c, n);
        if (rc) return rc;
        brute_finish_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n,
                                                                    c->d_keys, (mirt_hit*)c->d_res);
    } else if (quad_batch(c, n)) {
        intersect_quad_kernel<false><<<(n + kQuadBatchThreads / 4 - 1) / (kQuadBatchThreads / 4), kQuadBatchThreads, 0,
                                        c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n, (mirt_hit*)c->d_res,
                                                     nullptr);
    } else if (c->fast_slab) {
        intersect_kernel<true><<<(n + bt - 1) / bt, bt, 0, c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n,
                                                                      use_bvh, (mirt_hit*)c->d_res);
    } else {
        intersect_kernel<false><<<(n + bt - 1) / bt, bt, 0, c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n,
                                                                       use_bvh, (mirt_hit*)c->d_res);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_res, sizeof(mirt_hit) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_any_hit_rays(mirt_ctx* c, const mirt_ray* rays, int n, int use_bvh, int32_t* out)
{
    if (!ctx_ok(c, true, "mirt_any_hit_rays")) return MIRT_E_NOSCENE;
    if (n < 0 || (n > 0 && (!rays || !out))) {
        set_error("mirt_any_hit_rays: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (use_bvh && scene_of(c)->num_nodes == 0) {
        set_error("mirt_any_hit_rays: use_bvh set but no tree uploaded");
        return MIRT_E_NOSCENE;
    }
    if (n == 0) return MIRT_OK;
    int rc = ensure(&c->d_in, &c->in_cap, sizeof(mirt_ray) * (size_t)n);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, sizeof(int32_t) * (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_in, rays, sizeof(mirt_ray) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    const int bt = batch_threads(c, n);
    if (!use_bvh) {
        rc = launch_brute(c, n);
        if (rc) return rc;
        keys_to_flags_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(c->d_keys, n, (int32_t*)c->d_res);
    } else if (quad_batch(c, n)) {
        intersect_quad_kernel<true><<<(n + kQuadBatchThreads / 4 - 1) / (kQuadBatchThreads / 4), kQuadBatchThreads, 0,
                                       c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n, nullptr,
                                                    (int32_t*)c->d_res);
    } else if (c->fast_slab) {
        bvh_any_kernel<true><<<(n + bt - 1) / bt, bt, 0, c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n,
                                                                    (int32_t*)c->d_res);
    } else {
        bvh_any_kernel<false><<<(n + bt - 1) / bt, bt, 0, c->stream>>>(dev_scene(c), (const mirt_ray*)c->d_in, n,
                                                                     (int32_t*)c->d_res);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_res, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    return MIRT_OK;
}

int mirt_bvh_overlay(mirt_ctx* c, const mirt_camera* cam, int width, int height, int max_levels, mirt_rgba8* out)
{
    if (!ctx_ok(c, true, "mirt_bvh_overlay")) return MIRT_E_NOSCENE;
    // width, height <= 2^30: world_to_screen's range test forms width * 2 and height * 2 in int
    if (!cam || width <= 0 || height <= 0 || !out || width > (1 << 30) || height > (1 << 30) ||
        (size_t)width * height > ((size_t)1 << 31)) {
        set_error("mirt_bvh_overlay: invalid arguments");
        return MIRT_E_INVALID;
    }
    OverlayConst o{};
    o.px = cam->position.x; o.py = cam->position.y; o.pz = cam->position.z;
    o.fx = cam->forward.x; o.fy = cam->forward.y; o.fz = cam->forward.z;
    o.rx = cam->right.x; o.ry = cam->right.y; o.rz = cam->right.z;
    o.ux = cam->up.x; o.uy = cam->up.y; o.uz = cam->up.z;
    const float fov_rad = (float)((double)cam->fov * (M_PI / 180.0));  // bvh_visualiser.c:26
    o.half_h = tanf(fov_rad / 2.0f);                                    // :27 (float tanf)
    o.half_w = (float)width / (float)height * o.half_h;                 // :28-29
    o.width = width;
    o.height = height;
    o.max_levels = max_levels;
    const size_t pixels = (size_t)width * height;
    // The image goes through the ctx's frame slab, on the ctx's stream: behind
    // every frame enqueued on it and its copy out. A fresh frame's display
    // left pending on a shared accumulation buffer (the lazy fold) lives in
    // that slab: it is folded first, as before the slab is reallocated
    // (enqueue_frame); and the slab grows only once the stream has left it.
    if (c->acc && c->acc->pend_ctx == c) {
        if (int rc = accum_materialize(c->acc, c->stream)) return rc;
    }
    if (c->slab_guard) {
        HIP_TRY(hipStreamWaitEvent(c->stream, c->slab_free, 0));
        c->slab_guard = false;
    }
    if (c->out_cap < 4 * pixels + 4) HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = ensure((void**)&c->d_overlay, &c->overlay_cap, 4 * pixels);
    if (!rc) rc = ensure((void**)&c->d_out, &c->out_cap, 4 * pixels + 4);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_overlay, 0, 4 * pixels, c->stream));
    const Scene* sn = scene_of(c);
    const uint64_t lines = (uint64_t)sn->num_nodes * 60;
    if (lines > 0xffffffffull) {
        set_error("mirt_bvh_overlay: too many nodes");
        return MIRT_E_INVALID;
    }
    if (lines) {
        overlay_lines_kernel<<<(unsigned)((lines + 255) / 256), 256, 0, c->stream>>>(o, sn->d_nodes32, sn->d_ndepth,
                                                                                     (uint32_t)lines, c->d_overlay);
        HIP_TRY(hipGetLastError());
    }
    overlay_colour_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, c->stream>>>(c->d_overlay, sn->d_nodes32,
                                                                                 sn->d_ndepth, pixels, c->d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->d_out, 4 * pixels, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_camera_rays_uv(mirt_ctx* c, const mirt_camera* cam, int width, int height, const float* uv, int n,
                        mirt_ray* out)
{
    if (!ctx_ok(c, false, "mirt_camera_rays_uv")) return MIRT_E_INVALID;
    if (!cam || width <= 0 || height <= 0 || n < 0 || (n > 0 && (!uv || !out))) {
        set_error("mirt_camera_rays_uv: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (n == 0) return MIRT_OK;
    mirt_frame_desc fd{};
    fd.width = width;
    fd.height = height;
    fd.row_block = 8;
    fd.num_shards = 1;
    const FrameConst f = make_frame_const(cam, &fd);
    int rc = ensure(&c->d_in, &c->in_cap, 8 * (size_t)n);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, sizeof(mirt_ray) * (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_in, uv, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    camera_uv_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(f, (const float2*)c->d_in, n, (mirt_ray*)c->d_res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->d_res, sizeof(mirt_ray) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_sphere_pairs(mirt_ctx* c, const mirt_ray* rays, const mirt_sphere* spheres, int n, mirt_hit* out)
{
    if (!ctx_ok(c, false, "mirt_sphere_pairs")) return MIRT_E_INVALID;
    if (n < 0 || (n > 0 && (!rays || !spheres || !out))) {
        set_error("mirt_sphere_pairs: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (n == 0) return MIRT_OK;
    const size_t rb = sizeof(mirt_ray) * (size_t)n, sb = sizeof(mirt_sphere) * (size_t)n;
    int rc = ensure(&c->d_in, &c->in_cap, rb + sb + 16);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, sizeof(mirt_hit) * (size_t)n);
    if (rc) return rc;
    char* din = (char*)c->d_in;
    HIP_TRY(hipMemcpyAsync(din, rays, rb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + rb, spheres, sb, hipMemcpyHostToDevice, c->stream));
    sphere_pairs_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const mirt_ray*)din, (const mirt_sphere*)(din + rb),
                                                               n, (mirt_hit*)c->d_res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->d_res, sizeof(mirt_hit) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_aabb_pairs(mirt_ctx* c, const mirt_ray* rays, const mirt_aabb* boxes, int n, int32_t* out)
{
    if (!ctx_ok(c, false, "mirt_aabb_pairs")) return MIRT_E_INVALID;
    if (n < 0 || (n > 0 && (!rays || !boxes || !out))) {
        set_error("mirt_aabb_pairs: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (n == 0) return MIRT_OK;
    const size_t rb = sizeof(mirt_ray) * (size_t)n, bb = sizeof(mirt_aabb) * (size_t)n;
    int rc = ensure(&c->d_in, &c->in_cap, rb + bb + 16);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, 4 * (size_t)n);
    if (rc) return rc;
    char* din = (char*)c->d_in;
    HIP_TRY(hipMemcpyAsync(din, rays, rb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + rb, boxes, bb, hipMemcpyHostToDevice, c->stream));
    aabb_pairs_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const mirt_ray*)din, (const mirt_aabb*)(din + rb), n,
                                                             (int32_t*)c->d_res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->d_res, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_hemisphere_probe(mirt_ctx* c, const uint64_t* keys, const uint32_t* k0, const float* normals,
                          const int32_t* need, int n, float* out_dir, uint32_t* out_k)
{
    if (!ctx_ok(c, false, "mirt_hemisphere_probe")) return MIRT_E_INVALID;
    if (!keys || !k0 || !normals || !need || !out_dir || !out_k || (n != 64 && (n <= 0 || n % 256 != 0))) {
        set_error("mirt_hemisphere_probe: invalid arguments (n is 64 or a multiple of 256)");
        return MIRT_E_INVALID;
    }
    const size_t sn = (size_t)n, kb = 8 * sn, wb = 4 * sn, vb = 12 * sn;
    int rc = ensure(&c->d_in, &c->in_cap, kb + wb + vb + wb);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, vb + wb);
    if (rc) return rc;
    char* din = (char*)c->d_in;
    char* dres = (char*)c->d_res;
    HIP_TRY(hipMemcpyAsync(din, keys, kb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + kb, k0, wb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + kb + wb, normals, vb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + kb + wb + vb, need, wb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dres, out_dir, vb, hipMemcpyHostToDevice, c->stream));
    const int threads = n == 64 ? 64 : 256;
    hemisphere_probe_kernel<<<n / threads, threads, 0, c->stream>>>(
        (const uint64_t*)din, (const uint32_t*)(din + kb), (const float*)(din + kb + wb),
        (const int32_t*)(din + kb + wb + vb), (float*)dres, (uint32_t*)(dres + vb));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_dir, dres, vb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_k, dres + vb, wb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_box_form_pairs(mirt_ctx* c, const mirt_ray* rays, const mirt_aabb* boxes, const float* best, int n, int form,
                        int32_t* out)
{
    if (!ctx_ok(c, true, "mirt_box_form_pairs")) return MIRT_E_NOSCENE;
    if (n < 0 || form < MIRT_BOX_FORM_SLAB || form > MIRT_BOX_FORM_CONS_CAMERA ||
        (n > 0 && (!rays || !boxes || !best || !out))) {
        set_error("mirt_box_form_pairs: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (n == 0) return MIRT_OK;
    const size_t rb = sizeof(mirt_ray) * (size_t)n, bb = sizeof(mirt_aabb) * (size_t)n, fb = 4 * (size_t)n;
    int rc = ensure(&c->d_in, &c->in_cap, rb + bb + fb + 16);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, 4 * (size_t)n);
    if (rc) return rc;
    char* din = (char*)c->d_in;
    HIP_TRY(hipMemcpyAsync(din, rays, rb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + rb, boxes, bb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + rb + bb, best, fb, hipMemcpyHostToDevice, c->stream));
    box_form_pairs_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(dev_scene(c), (const mirt_ray*)din,
                                                                 (const mirt_aabb*)(din + rb),
                                                                 (const float*)(din + rb + bb), n, form,
                                                                 (int32_t*)c->d_res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->d_res, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_sphere_form_pairs(mirt_ctx* c, const mirt_ray* rays, const mirt_sphere* spheres, const float* best, int n,
                           int fast, uint32_t* out)
{
    if (!ctx_ok(c, false, "mirt_sphere_form_pairs")) return MIRT_E_INVALID;
    if (n < 0 || fast < 0 || fast > 3 || (n > 0 && (!rays || !spheres || !best || !out))) {
        set_error("mirt_sphere_form_pairs: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (n == 0) return MIRT_OK;
    const size_t rb = sizeof(mirt_ray) * (size_t)n, sb = sizeof(mirt_sphere) * (size_t)n, fb = 4 * (size_t)n;
    int rc = ensure(&c->d_in, &c->in_cap, rb + sb + fb + 16);
    if (!rc) rc = ensure(&c->d_res, &c->res_cap, 4 * (size_t)n);
    if (rc) return rc;
    char* din = (char*)c->d_in;
    HIP_TRY(hipMemcpyAsync(din, rays, rb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + rb, spheres, sb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(din + rb + sb, best, fb, hipMemcpyHostToDevice, c->stream));
    const dim3 grid((n + 255) / 256);
    const mirt_ray* dr = (const mirt_ray*)din;
    const mirt_sphere* ds = (const mirt_sphere*)(din + rb);
    const float* db = (const float*)(din + rb + sb);
    uint32_t* dout = (uint32_t*)c->d_res;
    switch (fast) {
    case 0: sphere_form_pairs_kernel<0><<<grid, 256, 0, c->stream>>>(dr, ds, db, n, dout); break;
    case 1: sphere_form_pairs_kernel<1><<<grid, 256, 0, c->stream>>>(dr, ds, db, n, dout); break;
    case 2: sphere_form_pairs_kernel<2><<<grid, 256, 0, c->stream>>>(dr, ds, db, n, dout); break;
    default: sphere_form_pairs_kernel<3><<<grid, 256, 0, c->stream>>>(dr, ds, db, n, dout); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->d_res, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_sqrt_form_sweep(mirt_ctx* c, uint64_t* mismatches, uint32_t* first)
{
    if (!ctx_ok(c, false, "mirt_sqrt_form_sweep")) return MIRT_E_INVALID;
    if (!mismatches || !first) {
        set_error("mirt_sqrt_form_sweep: invalid arguments");
        return MIRT_E_INVALID;
    }
    const int rc = ensure(&c->d_res, &c->res_cap, 16);
    if (rc) return rc;
    unsigned long long res[2] = {0ull, ~0ull};
    HIP_TRY(hipMemcpyAsync(c->d_res, res, sizeof(res), hipMemcpyHostToDevice, c->stream));
    sqrt_form_sweep_kernel<<<8192, 256, 0, c->stream>>>((unsigned long long*)c->d_res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(res, c->d_res, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *mismatches = res[0];
    *first = (uint32_t)res[1];
    return MIRT_OK;
}

float mirt_last_kernel_ms(mirt_ctx* c) { return c ? c->last_ms : 0.0f; }

void* mirt_ctx_stream(mirt_ctx* c)
{
    return c ? (void*)c->stream : nullptr;
}

int mirt_last_phase_ms(mirt_ctx* c, float* phase)
{
    if (!c || !phase) return MIRT_E_INVALID;
    if (!c->phases_valid) {
        set_error("mirt_last_phase_ms: the last frame did not use the wavefront schedule");
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t k = (c->ph_next + kPhaseRing - 1) % kPhaseRing;
    HIP_TRY(hipEventSynchronize(c->ph2[k]));
    HIP_TRY(hipEventElapsedTime(&phase[0], c->ph0[k], c->ph1[k]));
    HIP_TRY(hipEventElapsedTime(&phase[1], c->ph1[k], c->ph2[k]));
    return MIRT_OK;
}

int mirt_phase_log(mirt_ctx* c, float* out, int max)
{
    if (!c || max < 0 || (max > 0 && !out)) return MIRT_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    const int n = std::min<int>(max, (int)c->ph_count);
    for (int j = 0; j < n; j++) {  // oldest first
        const uint32_t k = (c->ph_next + kPhaseRing - (uint32_t)(n - j)) % kPhaseRing;
        HIP_TRY(hipEventSynchronize(c->ph2[k]));
        HIP_TRY(hipEventElapsedTime(&out[2 * j], c->ph0[k], c->ph1[k]));
        HIP_TRY(hipEventElapsedTime(&out[2 * j + 1], c->ph1[k], c->ph2[k]));
    }
    return n;
}

int mirt_set_option(mirt_ctx* c, int option, int value)
{
    if (!c) return MIRT_E_INVALID;
    switch (option) {
    case MIRT_OPT_TRAVERSAL:
        // mirt 0.2 numbered WAVEFRONT 1 (0.1 and 0.3+: 5); 1 stays a
        // deprecated alias so binaries built against the 0.2 header keep working
        if (value == MIRT_TRAV_WAVEFRONT_V02) value = MIRT_TRAV_WAVEFRONT;
        if (value != MIRT_TRAV_TILE && value != MIRT_TRAV_WAVEFRONT) break;
        c->trav = value;
        return MIRT_OK;
    case MIRT_OPT_FAST_SLAB:
        c->fast_slab = value != 0;
        return MIRT_OK;
    case MIRT_OPT_BOUNCE_THRESHOLD:
        if (value < 0 || value > 64) break;
        c->bounce_threshold = value;
        return MIRT_OK;
    case MIRT_OPT_DEFER:
        c->defer = value != 0;
        return MIRT_OK;
    case MIRT_OPT_PRUNE:
        c->prune = value != 0;
        return MIRT_OK;
    case MIRT_OPT_ORDERED:
        c->ordered = value != 0;
        return MIRT_OK;
    case MIRT_OPT_BOUNCE_BLOCKS:
        if (value < 0) break;
        c->bounce_blocks_opt = value;
        return MIRT_OK;
    case MIRT_OPT_QUAD_DRAIN:
        c->quad_drain = value != 0;
        return MIRT_OK;
    case MIRT_OPT_QUAD_BATCH:
        c->quad_batch = value != 0;
        return MIRT_OK;
    case MIRT_OPT_ZERO_COPY:
        if (value < 0 || value > 2) break;
        c->zero_copy = value;
        return MIRT_OK;
    case MIRT_OPT_DEBUG_STALL_MS:
        if (value < 0 || value > 10000) break;
        c->debug_stall_ms = value;
        return MIRT_OK;
    case MIRT_OPT_CONFIRM_ONCE:
        if (value < 0 || value > 2) break;
        c->confirm_once = value;
        return MIRT_OK;
    case MIRT_OPT_DEBUG_FAIL_CONFIRM:
        if (value < 0) break;
        c->debug_fail_confirm = value;
        return MIRT_OK;
    case MIRT_OPT_BUILD_FINISH:
        if (value < 0 || value > 64) break;
        c->build_finish = value;
        return MIRT_OK;
    case MIRT_OPT_QUEUE_ORDER:
        if (value < 0 || value > 2) break;
        c->queue_order = value;
        return MIRT_OK;
    case MIRT_OPT_LEAF_BATCH:
        if (value < 0 || value > 2) break;
        c->leaf_batch_opt = value;
        return MIRT_OK;
    case MIRT_OPT_BLOCK_WAVES:
        if (value != 1 && value != 2 && value != 4 && value != 8) break;
        c->block_waves = value;
        return MIRT_OK;
    case MIRT_OPT_DENOISE_TILE:
        if (value != 0 && value != 1) break;
        c->denoise_tile = value;
        return MIRT_OK;
    case MIRT_OPT_HISTORY_MOTION:
        if (value != 0 && value != 1) break;
        c->history_motion = value;
        return MIRT_OK;
    case MIRT_OPT_PRIMARY_CACHE:
        if (value != 0 && value != 1) break;
        if (value == 0 && c->pc.d) {
            // the frames that may still read or fill the slab, on whichever stream
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
            (void)hipFree(c->pc.d);
        }
        if (value == 0) c->pc = PrimaryCache{};
        c->pc.on = value;
        c->pc.hits = c->pc.fills = c->pc.bypassed = 0;   // counted since the option was last set to 1
        return MIRT_OK;
    case MIRT_OPT_PRIMARY_SCAN: {
        if (value < 0 || value > 2) break;
        if (value == 0 && c->ps.d) {
            // the frames that may still read or write the arrays, on whichever stream
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
            (void)hipFree(c->ps.d);
            if (c->ps.h_verdict) (void)hipHostFree(c->ps.h_verdict);
        }
        const int budget = c->ps.budget, rebuild = c->ps.always_rebuild;
        if (value == 0) c->ps = PrimaryScan{};
        c->ps.opt = value;
        c->ps.budget = budget;
        c->ps.always_rebuild = rebuild;
        c->ps.scanned = c->ps.bypassed = c->ps.rebuilds = 0;   // counted since the option was last set
        return MIRT_OK;
    }
    case MIRT_OPT_PRIMARY_SCAN_BUDGET:
        if (value < 1 || value > (1 << 24)) break;
        c->ps.budget = value;
        return MIRT_OK;
    case MIRT_OPT_PRIMARY_SCAN_REBUILD:
        if (value != 0 && value != 1) break;
        c->ps.always_rebuild = value;
        return MIRT_OK;
    default:
        break;
    }
    set_error("mirt_set_option: bad option %d / value %d", option, value);
    return MIRT_E_INVALID;
}

int mirt_get_option(mirt_ctx* c, int option)
{
    if (!c) return MIRT_E_INVALID;
    if (option == MIRT_OPT_TRAVERSAL) return c->trav;
    if (option == MIRT_OPT_FAST_SLAB) return c->fast_slab;
    if (option == MIRT_OPT_BLOCK_WAVES) return c->block_waves;
    if (option == MIRT_OPT_DEFER) return c->defer;
    if (option == MIRT_OPT_BOUNCE_THRESHOLD) return c->bounce_threshold;
    if (option == MIRT_OPT_PRUNE) return c->prune;
    if (option == MIRT_OPT_ORDERED) return c->ordered;
    if (option == MIRT_OPT_BOUNCE_BLOCKS) return c->bounce_blocks_opt;
    if (option == MIRT_OPT_QUAD_DRAIN) return c->quad_drain;
    if (option == MIRT_OPT_QUAD_BATCH) return c->quad_batch;
    if (option == MIRT_OPT_ZERO_COPY) return c->zero_copy;
    if (option == MIRT_OPT_QUEUE_ORDER) return c->queue_order;
    if (option == MIRT_OPT_DEBUG_STALL_MS) return c->debug_stall_ms;
    if (option == MIRT_OPT_CONFIRM_ONCE) return confirm_once(c) ? 1 : 0;  // in effect for the uploaded scene
    if (option == MIRT_OPT_DEBUG_FAIL_CONFIRM) return c->debug_fail_confirm;
    if (option == MIRT_OPT_BUILD_FINISH) return c->build_finish;
    if (option == MIRT_OPT_PRIMARY_CACHE) return c->pc.on;
    if (option == MIRT_OPT_PRIMARY_SCAN) return c->ps.opt;
    if (option == MIRT_OPT_PRIMARY_SCAN_BUDGET) return c->ps.budget;
    if (option == MIRT_OPT_PRIMARY_SCAN_REBUILD) return c->ps.always_rebuild;
    if (option == MIRT_OPT_DENOISE_TILE) return c->denoise_tile;
    if (option == MIRT_OPT_HISTORY_MOTION) return c->history_motion;
    if (option == MIRT_OPT_LEAF_BATCH) return leaf_batch(c) ? 1 : 0;  // in effect for the uploaded scene
    set_error("mirt_get_option: bad option %d", option);
    return MIRT_E_INVALID;
}

int mirt_primary_cache_stats_get(mirt_ctx* c, mirt_primary_cache_stats* out)
{
    if (!c || !out) {
        set_error("mirt_primary_cache_stats_get: invalid arguments");
        return MIRT_E_INVALID;
    }
    const PrimaryCache& pc = c->pc;
    *out = mirt_primary_cache_stats{};
    out->hits = pc.hits;
    out->fills = pc.fills;
    out->bypassed = pc.bypassed;
    out->scene_id = pc.valid ? pc.key.scene_id : 0;
    out->bytes = pc.cap;
    out->valid = pc.valid ? 1 : 0;
    out->last = pc.last;
    out->reason = pc.reason;
    out->width = pc.valid ? pc.key.width : 0;
    out->rows = pc.valid ? pc.key.shard_rows : 0;
    return MIRT_OK;
}

int mirt_primary_scan_stats_get(mirt_ctx* c, mirt_primary_scan_stats* out)
{
    if (!c || !out) {
        set_error("mirt_primary_scan_stats_get: invalid arguments");
        return MIRT_E_INVALID;
    }
    const PrimaryScan& ps = c->ps;
    *out = mirt_primary_scan_stats{};
    out->scanned = ps.scanned;
    out->bypassed = ps.bypassed;
    out->rebuilds = ps.rebuilds;
    out->bytes = ps.cap;
    out->last = ps.last;
    out->reason = ps.opt ? ps.reason : MIRT_PSCAN_OFF;
    out->budget = ps.budget;
    out->leaves = ps.valid ? ps.nl : 0;
    if (ps.last != MIRT_PSCAN_SCAN || !ps.stats) return MIRT_OK;
    // the last scanned frame's counters: the only device call, after its frames
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
    unsigned long long h[kPscanSlots * kPscanSlotWords];
    HIP_TRY(hipMemcpy(h, ps.stats, sizeof h, hipMemcpyDeviceToHost));
    for (int k = 0; k < kPscanSlots; k++) {
        out->tiles_scan += h[k * kPscanSlotWords];
        out->tiles_walk += h[k * kPscanSlotWords + 1];
        out->tiles_empty += h[k * kPscanSlotWords + 2];
        out->chunks += h[k * kPscanSlotWords + 3];
        out->leaves_tested += h[k * kPscanSlotWords + 4];
        out->candidates += h[k * kPscanSlotWords + 5];
    }
    return MIRT_OK;
}

// What the two slab calls check before any HIP call.
static bool pc_slab_args_ok(const mirt_ctx* c, const void* t, const void* sphere, size_t n, const char* fn)
{
    if (!c || !t || !sphere || !c->pc.valid || n != c->pc.pixels()) {
        set_error("%s: invalid arguments, or no valid cache of that size", fn);
        return false;
    }
    return true;
}

// The frames that may still fill or read the slab have ended.
static int pc_settle(mirt_ctx* c)
{
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->launched && c->last_stream != c->stream) HIP_TRY(hipEventSynchronize(c->done));
    return MIRT_OK;
}

int mirt_primary_cache_read(mirt_ctx* c, float* t, int32_t* sphere, size_t n)
{
    if (!pc_slab_args_ok(c, t, sphere, n, "mirt_primary_cache_read")) return MIRT_E_INVALID;
    if (int rc = pc_settle(c)) return rc;
    HIP_TRY(hipMemcpy(t, c->pc.d, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sphere, (const char*)c->pc.d + 4 * n, 4 * n, hipMemcpyDeviceToHost));
    return MIRT_OK;
}

int mirt_primary_cache_write(mirt_ctx* c, const float* t, const int32_t* sphere, size_t n)
{
    if (!pc_slab_args_ok(c, t, sphere, n, "mirt_primary_cache_write")) return MIRT_E_INVALID;
    // a hit frame indexes the scene's arrays with what the slab holds. The
    // bound is the resident scene's: a hit implies that it is the key's (scene
    // ids never recur), and a slab of any other scene is never read again
    const int ns = scene_of(c)->num_spheres;
    for (size_t i = 0; i < n; i++)
        if (sphere[i] < -1 || sphere[i] >= ns || (sphere[i] >= 0 && !(std::isfinite(t[i]) && t[i] > 0.0f))) {
            set_error("mirt_primary_cache_write: element %zu (t %g, sphere %d) is no hit of the resident scene", i,
                      (double)t[i], sphere[i]);
            return MIRT_E_INVALID;
        }
    if (int rc = pc_settle(c)) return rc;
    HIP_TRY(hipMemcpy(c->pc.d, t, 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((char*)c->pc.d + 4 * n, sphere, 4 * n, hipMemcpyHostToDevice));
    return MIRT_OK;
}

}  // extern "C"

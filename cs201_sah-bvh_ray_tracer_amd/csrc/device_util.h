// What the .hip files of the tree (bvh_device, scene_device, refit_device,
// quality_device) share of HIP plumbing: error handling, owned device memory,
// one-way atomics, and the two-level prefix sum. For .hip files only; every
// definition has internal linkage, so each file carries its own copy of the
// kernels it launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "internal.h"

namespace mirt {
namespace {

// ---- host side

int hip_fail(hipError_t e, const char* what)
{
    set_error("%s: %s", what, hipGetErrorString(e));
    return MIRT_E_DEVICE;
}

#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

inline unsigned blocks(size_t items, int per) { return (unsigned)((items + (size_t)per - 1) / (size_t)per); }

// a device allocation freed on the way out
struct DevMem {
    void* p = nullptr;
    ~DevMem()
    {
        if (p) (void)hipFree(p);
    }
};

// ---- one-way updates of global words. The plain read may be stale, which only
// means an atomic that changes nothing: the values move one way.

__device__ __forceinline__ void flag(int* ctl, int w)
{
    if (!*(volatile int*)&ctl[w]) atomicOr(&ctl[w], 1);
}
__device__ __forceinline__ void global_min(int* p, int v)
{
    if (v < *(volatile int*)p) atomicMin(p, v);
}
__device__ __forceinline__ void global_max(int* p, int v)
{
    if (v > *(volatile int*)p) atomicMax(p, v);
}

// ---- prefix sums over n ints: exclusive within tiles of kScanTile (scan_tile,
// one workgroup of kScanBlock threads per tile), then the tile sums made
// exclusive (scan_sums_kernel); element i's prefix is scan_prefix(data, tsum, i)

constexpr int kScanBlock = 256;
constexpr int kScanTile = 4 * kScanBlock;
constexpr int kSumBlock = 1024;  // the one workgroup that scans an array's tile sums

// exclusive prefix sum of one value per thread over a workgroup of B threads
template <int B>
__device__ int block_excl_scan(int v, int* sh, int* total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < B; off <<= 1) {
        const int x = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[B - 1];
    __syncthreads();
    return incl - v;
}

// The tile of workgroup blockIdx.x: out[i] = the sum of load(j) over the tile's
// j < i, written for i < n_out; load(i) is asked for i < n_in only. The tile's
// total goes to *tile_sum. `out` may be the array `load` reads: a thread reads
// its four elements before it writes them.
template <class Load>
__device__ __forceinline__ void scan_tile(Load load, int n_in, int n_out, int* out, int* tile_sum)
{
    __shared__ int sh[kScanBlock];
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * 4;
    int f[4], s = 0;
    for (int j = 0; j < 4; j++) {
        f[j] = i0 + j < n_in ? load(i0 + j) : 0;
        s += f[j];
    }
    int total;
    int run = block_excl_scan<kScanBlock>(s, sh, &total);
    for (int j = 0; j < 4; j++) {
        if (i0 + j < n_out) out[i0 + j] = run;
        run += f[j];
    }
    if (threadIdx.x == 0) *tile_sum = total;
}

// one workgroup of B threads per array: its `tiles` tile sums made exclusive in place, the grand total to
// totals[array] if asked (a template, so only the files that launch it carry it)
template <int B>
__global__ void scan_sums_kernel(int* tsum, int tiles, int* totals)
{
    __shared__ int sh[B];
    int* ts = tsum + (size_t)tiles * blockIdx.x;
    int carry = 0;
    for (int base = 0; base < tiles; base += B) {
        const int i = base + (int)threadIdx.x;
        const int v = i < tiles ? ts[i] : 0;
        int total;
        const int ex = block_excl_scan<B>(v, sh, &total);
        if (i < tiles) ts[i] = carry + ex;
        carry += total;
    }
    if (totals && threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__device__ __forceinline__ int scan_prefix(const int* data, const int* tsum, int i)
{
    return data[i] + tsum[i / kScanTile];
}

}  // namespace
}  // namespace mirt

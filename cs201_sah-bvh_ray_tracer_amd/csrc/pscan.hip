// The per-camera data of the primary scan (MIRT_OPT_PRIMARY_SCAN, DESIGN
// 9.15; the arithmetic and its margins: pscan.h): one record per leaf sorted
// by depth key, and the number of records whose rectangle holds each tile.
// Built once per (camera, frame geometry, scene) on the frame's stream, ahead
// of the frame that needs it; the per-frame kernels are render.hip's
// (pscan_tile_kernel, pscan_walk_kernel).
//
//   pscan_planes_kernel   the bounding planes of every tile column and row
//   pscan_records_kernel  a leaf's record and its four corners in the
//                         difference grid (one thread per leaf)
//   rocprim radix sort    the records by key, ascending
//   pscan_prefix_kernel   the difference grid summed along rows, then columns:
//                         element (i, j) = the records holding tile (i, j)
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "internal.h"
#include "pscan.h"

namespace mirt {

namespace {

__global__ void pscan_planes_kernel(PscanCam cam, PscanPlanes* __restrict__ planes)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < cam.ntx) planes[k] = pscan_column(cam, k);
    else if (k < cam.ntx + cam.nty) planes[k] = pscan_row(cam, k - cam.ntx);
}

__global__ void pscan_records_kernel(PscanCam cam, const PscanPlanes* __restrict__ planes,
                                     const float4* __restrict__ leaf_geo, uint32_t nl, PscanRec* __restrict__ rec,
                                     float* __restrict__ key, int* __restrict__ grid)
{
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= nl) return;
    const float4 g = leaf_geo[li];
    const PscanRec r = pscan_record(cam, planes, planes + cam.ntx, li, g.x, g.y, g.z, g.w);
    rec[li] = r;
    key[li] = r.z;
    const int i0 = (int)(r.cols & 0xffffu), i1 = (int)(r.cols >> 16), j0 = (int)(r.rows & 0xffffu), j1 = (int)(r.rows >> 16);
    if (i1 < i0) return;
    // i1 + 1 <= ntx and j1 + 1 <= nty: the grid is (ntx + 1) x (nty + 1)
    const int w = cam.ntx + 1;
    atomicAdd(&grid[j0 * w + i0], 1);
    atomicAdd(&grid[j0 * w + i1 + 1], -1);
    atomicAdd(&grid[(j1 + 1) * w + i0], -1);
    atomicAdd(&grid[(j1 + 1) * w + i1 + 1], 1);
}

// One workgroup: every row summed left to right, then every column top to bottom.
__global__ __launch_bounds__(1024) void pscan_prefix_kernel(int* __restrict__ grid, int w, int h)
{
    for (int j = threadIdx.x; j < h; j += blockDim.x) {
        int acc = 0;
        for (int i = 0; i < w; i++) {
            acc += grid[j * w + i];
            grid[j * w + i] = acc;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < w; i += blockDim.x) {
        int acc = 0;
        for (int j = 0; j < h; j++) {
            acc += grid[j * w + i];
            grid[j * w + i] = acc;
        }
    }
}

}  // namespace

size_t pscan_sort_bytes(uint32_t nl)
{
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (float*)nullptr, (float*)nullptr, (PscanRec*)nullptr,
                                  (PscanRec*)nullptr, (size_t)nl) != hipSuccess)
        return 0;
    return bytes ? bytes : 1;
}

int pscan_build(const PscanCam& cam, const void* leaf_geo, uint32_t nl, const PscanBuild& b, ihipStream_t* s)
{
    const int gw = cam.ntx + 1, gh = cam.nty + 1;
    hipError_t e = hipMemsetAsync(b.grid, 0, sizeof(int) * (size_t)gw * gh, s);
    if (e != hipSuccess) return e;
    pscan_planes_kernel<<<(cam.ntx + cam.nty + 255) / 256, 256, 0, s>>>(cam, b.planes);
    if (nl) {
        pscan_records_kernel<<<(nl + 63) / 64, 64, 0, s>>>(cam, b.planes, (const float4*)leaf_geo, nl, b.rec_in,
                                                          b.key_in, b.grid);
        size_t bytes = b.sort_bytes;
        e = rocprim::radix_sort_pairs(b.sort_tmp, bytes, b.key_in, b.key_out, b.rec_in, b.rec, (size_t)nl, 0u, 32u, s);
        if (e != hipSuccess) return e;
    }
    pscan_prefix_kernel<<<1, 1024, 0, s>>>(b.grid, gw, gh);
    return hipGetLastError();
}

}  // namespace mirt

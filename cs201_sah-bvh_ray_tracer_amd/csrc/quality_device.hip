// The SAH quality of a tree on the device (mirt_scene_quality, and the
// measurement mirt_scene_update_device decides by): what bvh_quality.cpp states
// on the host, byte for byte.
//
//   quality  one thread per node. e comes from node 0, a uniform load every
//            thread repeats. A thread forms its node's term (quality.h) and
//            adds its halves to the inner or the leaf pair; the four uint64
//            partial sums and the four counters are reduced across the wave by
//            shuffles, across the workgroup's four waves through LDS, and one
//            thread per workgroup adds them to the ctl words: one set of
//            atomics per workgroup. There are kSlots sets of ctl words, a
//            cache line apart, and workgroup b uses set b % kSlots: with one
//            set, the 8 x 24k atomics of a 6.1M-node tree queue on eight
//            addresses (MEASUREMENTS.md E: 2.15 ms the call, 0.35 ms with 64).
// The sums are integers, so the order in which the atomics land does not show.
// The host reads the ctl words back once, adds the sets and ends in
// quality_finish, as the host path does. Every loop is bounded at launch; no workgroup waits on
// another.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "device_util.h"
#include "internal.h"
#include "quality.h"

#pragma clang fp contract(off)

namespace {

using namespace mirt;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kWords = 8;  // per thread: four uint64 sums, four counters

constexpr int kSlots = 64;  // sets of ctl words the workgroups spread their atomics over

struct alignas(128) Slot {
    QualitySums q;
};
static_assert(sizeof(QualitySums) == 56 && sizeof(Slot) == 128, "a set of ctl words per cache line");

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(v & 0xffffffffull), off);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ void quality_kernel(const mirt_node* nd, int nn, int ns, Slot* ctl)
{
    __shared__ unsigned long long sh[kWaves][kWords];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const float a0 = box_area(nd[0]);
    const bool ok = quality_root_ok(a0);
    const double scale = ok ? quality_scale(quality_exponent(a0)) : 0.0;
    // inner hi / lo, leaf hi / lo, inner nodes, leaves, dead leaves, clamped
    unsigned long long v[kWords] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < nn) {
        const mirt_node n = nd[i];
        const bool inner = n.sphere < 0, dead = dead_leaf(n, ns);
        int32_t clamped = 0;
        const uint64_t t = ok && !dead ? quality_term(box_area(n), a0, scale, &clamped) : 0;
        const unsigned long long hi = t >> 24, lo = t & 0xffffffu;
        v[0] = inner ? hi : 0;
        v[1] = inner ? lo : 0;
        v[2] = inner ? 0 : hi;
        v[3] = inner ? 0 : lo;
        v[4] = inner ? 1 : 0;
        v[5] = !inner && !dead ? 1 : 0;
        v[6] = dead ? 1 : 0;
        v[7] = (unsigned long long)clamped;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < kWords; k++) v[k] += shfl_xor_u64(v[k], off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int k = 0; k < kWords; k++) sh[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long t[kWords];
    for (int k = 0; k < kWords; k++) {
        t[k] = 0;
        for (int w = 0; w < kWaves; w++) t[k] += sh[w][k];
    }
    ctl += blockIdx.x % kSlots;  // workgroups share kSlots sets of ctl words, a cache line apart; the host adds them
    unsigned long long* sums = (unsigned long long*)ctl;  // inner_hi, inner_lo, leaf_hi, leaf_lo
    for (int k = 0; k < 4; k++)
        if (t[k]) atomicAdd(&sums[k], t[k]);
    int* counts = &ctl->q.inner_nodes;  // inner_nodes, leaves, dead_leaves, clamped
    for (int k = 0; k < 4; k++)
        if (t[4 + k]) atomicAdd(&counts[k], (int)t[4 + k]);
    if (blockIdx.x == 0) ctl->q.root_area_bits = float_bits(a0);
}

}  // namespace

// The quality of the validated flat tree d_nodes[nn] on the device, measured on stream s. Blocking (one read-back).
int mirt::quality_device(hipStream_t s, const mirt_node* d_nodes, int nn, int ns, mirt_tree_quality* out, const char* fn)
{
    std::memset(out, 0, sizeof *out);
    if (nn <= 0) return MIRT_OK;
    DevMem ctl;
    HIP_TRY(hipMalloc(&ctl.p, sizeof(Slot) * kSlots));
    HIP_TRY(hipMemsetAsync(ctl.p, 0, sizeof(Slot) * kSlots, s));
    quality_kernel<<<blocks((size_t)nn, kBlock), kBlock, 0, s>>>(d_nodes, nn, ns, (Slot*)ctl.p);
    HIP_TRY(hipGetLastError());
    Slot slots[kSlots];
    HIP_TRY(hipMemcpyAsync(slots, ctl.p, sizeof(Slot) * kSlots, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    QualitySums q = slots[0].q;
    for (int k = 1; k < kSlots; k++) {
        q.inner_hi += slots[k].q.inner_hi;
        q.inner_lo += slots[k].q.inner_lo;
        q.leaf_hi += slots[k].q.leaf_hi;
        q.leaf_lo += slots[k].q.leaf_lo;
        q.inner_nodes += slots[k].q.inner_nodes;
        q.leaves += slots[k].q.leaves;
        q.dead_leaves += slots[k].q.dead_leaves;
        q.clamped += slots[k].q.clamped;
    }
    if (q.inner_nodes < 0 || q.leaves < 0 || q.dead_leaves < 0 ||
        (int64_t)q.inner_nodes + q.leaves + q.dead_leaves != (int64_t)nn) {
        set_error("%s: the quality kernel counted %d + %d + %d of %d nodes", fn, q.inner_nodes, q.leaves, q.dead_leaves,
                  nn);
        return MIRT_E_DEVICE;
    }
    quality_finish(q, out);
    return MIRT_OK;
}

extern "C" {

int mirt_scene_quality(mirt_ctx* c, mirt_tree_quality* out)
{
    const char* fn = "mirt_scene_quality";
    if (!c || !out) {
        set_error("%s: null context or output", fn);
        return MIRT_E_INVALID;
    }
    ResidentScene rs{};
    if (!ctx_resident_scene(c, &rs)) {
        set_error("%s: no scene uploaded", fn);
        return MIRT_E_NOSCENE;
    }
    HIP_TRY(hipSetDevice(ctx_device(c)));
    return quality_device((hipStream_t)mirt_ctx_stream(c), rs.nodes32, rs.num_nodes, rs.num_spheres, out, fn);
}

}  // extern "C"

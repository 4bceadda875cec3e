// The SAH build of bvh_build.cpp (the reference's build_bvh_node, bvh.c:117-209)
// on the device: mirt_bvh_build_flat_device returns the same flat tree and the
// same reordered sphere array as mirt_bvh_build_flat, bit for bit.
//
// The tree is built level by level. The nodes of one level own disjoint
// contiguous ranges of the sphere array; every sphere carries the index of its
// node. One level is
//   bounds     min/max of the sphere boxes fl(c -+ r) per node, atomics on an
//              order-preserving integer key of the float: exact, so the order
//              of the combine does not matter;
//   classify   leaf (n <= 1 or depth >= 40) or inner; inner nodes take a pair
//              of child slots in the next level. Their count is read back
//              once: the node and bin arrays are sized from it, never guessed;
//   bin, sah   bvh_build.cpp's 8 bins per axis; the planes, the areas and the
//              cost are tree.h's split_plane, box_area and sah_cost, which the
//              host builder calls too (no contraction: -ffp-contract=off);
//              nodes of at most kSmall spheres are binned by their own SAH
//              thread instead of by atomics, by the same rule;
//   partition  the reference's swap loop (bvh.c:172-201) in closed form. With
//              positions relative to the range and L_0 < L_1 < ... the
//              positions of the nl elements left of the plane, position
//              k < nl receives the element of L_k, and a right element at p
//              ends at the first q >= nl of the chain p -> L_p -> L_{L_p} ...
//              (each swap of the loop moves the right element at `mid` to the
//              place of the left element it meets). Left ranks come from one
//              prefix sum over the array, chains are resolved by pointer
//              doubling, ceil(log2(longest range)) rounds.
// The finish (MIRT_OPT_BUILD_FINISH): once a level's read-back
// shows that no open node holds more than F <= 64 spheres, the level loop
// stops and one wave per open node builds that node's whole subtree, one
// sphere per lane, by the same rules (subtree_kernel). It runs twice: pass A
// orders the spheres and counts each subtree's nodes, pass B, after the sizes
// and pre-order indices of the levels above, writes the nodes where they belong.
// Then subtree sizes bottom-up, pre-order indices top-down, and the nodes are
// written in mirt_node layout. The download of the result is a separate step:
// mirt_scene_build_device (scene_device.hip) takes the tree where it lies.
//
// Order independence needs min/max to be exact and symmetric: a NaN or an
// infinity among the inputs, or a sphere box coordinate that is -0.0 (fmin(-0,
// +0) depends on operand order), is found by the first pass and the host
// builder runs on the untouched input instead (mirt_build_stats.on_device 0).
//
// Every kernel loop is bounded at launch; no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "device_util.h"
#include "internal.h"
#include "tree.h"

#pragma clang fp contract(off)

namespace {

using namespace mirt;

constexpr int kBlock = kScanBlock;
constexpr int kItems = 8;
constexpr int kChunk = kBlock * kItems;  // spheres per workgroup of the bounds / bin passes
constexpr int kTile = kScanTile;         // spheres per workgroup of the prefix sum
constexpr int kBinWords = 168;           // per inner node: 3 x 8 counts, 3 x 8 x 3 lo keys, 3 x 8 x 3 hi keys
constexpr int kBinLo = 24, kBinHi = 96;
constexpr int kKeyPosInf = 0x7f800000;       // fkey(+inf)
constexpr int kKeyNegInf = (int)0x807fffffu; // fkey(-inf)
constexpr int kMaxDepth = 40;                // bvh.c:131
constexpr int kSmall = 32;                   // inner nodes of at most this many spheres are binned by their SAH thread

// One node of the level arrays (64 B). Storage order within a level is
// arbitrary (child slots are handed out by an atomic counter); the tree is in
// `left`, and the output order comes from sizes and pre-order indices.
struct BNode {
    int lo, hi;      // range of the device sphere array
    int left;        // global index of the left child (right = left + 1); -1: leaf; kFinishRoot: subtree_kernel's
    int axis;
    int klo[3], khi[3];  // bounds as ordered keys
    float split;
    int nl;          // elements left of the plane
    int gbase;       // prefix sum of the left flags at lo
    uint32_t size;   // nodes of the subtree
    uint32_t pre;    // pre-order index
    int pad;
};
static_assert(sizeof(BNode) == 64, "BNode");

// ctl words read back by the host (kCtlFinNodes: 64 bits, words 4 and 5)
enum { kCtlInner = 0, kCtlMaxRange = 1, kCtlDeclined = 2, kCtlFinNodes = 4, kCtlMoved = 6, kCtlError = 7, kCtlWords = 8 };

// The finish: an open node of the hand-off level whose subtree one wave builds
// (BNode::left), the spheres a wave takes, and the cap of its walk -- m spheres
// at depth d make at most m * (40 - d) + 1 nodes, so a walk never reaches it.
constexpr int kFinishRoot = -2;
constexpr int kWave = 64;
constexpr int kFinishCap = kWave * (kMaxDepth + 1) + 1;
constexpr int kFinishFrames = kMaxDepth + 1;  // the nodes of one root-to-leaf path
// MIRT_OPT_BUILD_FINISH 1 (automatic): builds of at most this many spheres take the finish. Measured
// ahead at 10k spheres (4.3 against 6.9 ms), level at 100k, behind at 1M (64 against 41 ms), where the
// 65k waves' redundant per-lane SAH scans cost more than the 24 level rounds they replace.
constexpr int kFinishAutoMax = 131072;
enum { kErrCap = 1, kErrSize = 2 };           // kCtlError bits: the walk hit kFinishCap / pass B outgrew pass A's count

// float <-> int key with the same order (-0.0 < +0.0; the build declines -0.0 boxes)
__device__ __forceinline__ int fkey(float f)
{
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float funkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__device__ __forceinline__ float comp(const float4& g, int axis) { return axis == 0 ? g.x : (axis == 1 ? g.y : g.z); }

__device__ __forceinline__ bool goes_left(int axis, float split, const float4& g) { return comp(g, axis) < split; }
__device__ __forceinline__ bool goes_left(const BNode& nd, const float4& g) { return goes_left(nd.axis, nd.split, g); }

// the sphere's box fl(c -+ r) as keys (bvh.c:26-46)
__device__ __forceinline__ void sphere_keys(const float4& g, int* kl, int* kh)
{
    for (int x = 0; x < 3; x++) {
        const float c = comp(g, x);
        kl[x] = fkey(c - g.w);
        kh[x] = fkey(c + g.w);
    }
}

// ---- first and last pass: the caller's 20-byte spheres <-> (centre, radius) + colour

__global__ void prep_kernel(const uint32_t* aos, int n, float4* geo, uint32_t* col, int* nof, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t* s = aos + 5 * (size_t)i;
    const uint32_t w[4] = {s[0], s[1], s[2], s[3]};
    if (sphere_declined(w[0], w[1], w[2], w[3])) atomicOr(&ctl[kCtlDeclined], 1);
    geo[i] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
    col[i] = s[4];
    nof[i] = 0;
}

// The device-source entry of a build (mirt_scene_update_device_ptr's rebuild):
// the `total` 20-byte spheres at src copied to the build's scratch with each
// colour word replaced by the sphere's index, the colours saved aside. One
// thread per 32-bit word, so loads and stores stay coalesced.
__global__ void tag_kernel(const uint32_t* __restrict__ src, size_t words, uint32_t* __restrict__ aos,
                           uint32_t* __restrict__ colour)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= words) return;
    const size_t sphere = i / 5;
    uint32_t v = src[i];
    if (i - 5 * sphere == 4) {
        colour[sphere] = v;
        v = (uint32_t)sphere;
    }
    aos[i] = v;
}

__global__ void finish_kernel(const float4* geo, const uint32_t* col, int n, uint32_t* aos)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 g = geo[i];
    uint32_t* s = aos + 5 * (size_t)i;
    s[0] = __float_as_uint(g.x);
    s[1] = __float_as_uint(g.y);
    s[2] = __float_as_uint(g.z);
    s[3] = __float_as_uint(g.w);
    s[4] = col[i];
}

__global__ void root_kernel(BNode* nodes, int n)
{
    BNode nd{};
    nd.lo = 0;
    nd.hi = n;
    nd.left = -1;
    for (int a = 0; a < 3; a++) {
        nd.klo[a] = kKeyPosInf;
        nd.khi[a] = kKeyNegInf;
    }
    nodes[0] = nd;
}

// ---- bounds of every node of the level (bvh.c:26-46)

__global__ void bounds_kernel(const float4* geo, const int* nof, int n, BNode* nodes)
{
    __shared__ int sh[6];
    const int t = threadIdx.x;
    const int base = blockIdx.x * kChunk;
    const int end = min(base + kChunk, n);
    // ranges are contiguous: first and last sphere in one node = all of them
    const int first = nof[base], last = nof[end - 1];
    const bool uni = first == last && first >= 0;
    if (uni) {
        if (t < 6) sh[t] = t < 3 ? kKeyPosInf : kKeyNegInf;
        __syncthreads();
    }
    int alo[3] = {kKeyPosInf, kKeyPosInf, kKeyPosInf}, ahi[3] = {kKeyNegInf, kKeyNegInf, kKeyNegInf};
    for (int i = base + t; i < end; i += kBlock) {
        const int k = uni ? first : nof[i];
        if (k < 0) continue;
        const float4 g = geo[i];
        // a node's only sphere writes its box without atomics (most nodes of the deep levels)
        const bool alone = !uni && nodes[k].hi - nodes[k].lo == 1;
        for (int a = 0; a < 3; a++) {
            const float c = comp(g, a);
            const int l = fkey(c - g.w), h = fkey(c + g.w);
            if (uni) {
                alo[a] = min(alo[a], l);
                ahi[a] = max(ahi[a], h);
            } else if (alone) {
                nodes[k].klo[a] = l;
                nodes[k].khi[a] = h;
            } else {
                global_min(&nodes[k].klo[a], l);
                global_max(&nodes[k].khi[a], h);
            }
        }
    }
    if (uni) {
        for (int a = 0; a < 3; a++) {
            atomicMin(&sh[a], alo[a]);
            atomicMax(&sh[3 + a], ahi[a]);
        }
        __syncthreads();
        if (t < 3) global_min(&nodes[first].klo[t], sh[t]);
        else if (t < 6) global_max(&nodes[first].khi[t - 3], sh[t]);
    }
}

// ---- leaf or inner (bvh.c:131); inner nodes take two slots of the next level

__global__ void classify_kernel(BNode* nodes, int off, int cnt, int next_off, int at_max_depth, int* ctl)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = j < cnt;
    BNode* nd = valid ? &nodes[off + j] : nullptr;
    const int m = valid ? nd->hi - nd->lo : 0;
    const bool inner = valid && m > 1 && !at_max_depth;
    // one atomic per wave: the first inner lane takes slots for all of them
    const unsigned long long mask = __ballot(inner);
    if (mask) {
        const int lane = __lane_id(), leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctl[kCtlInner], __popcll(mask));
        base = __shfl(base, leader);
        if (inner) {
            nd->left = next_off + 2 * (base + __popcll(mask & ((1ull << lane) - 1ull)));
            global_max(&ctl[kCtlMaxRange], m);
        }
    }
    if (valid && !inner) nd->left = -1;
}

// ---- binned SAH (bvh_build.cpp FlatBuilder::build). The rules -- a bin word's
// start value, the planes, a sphere's bins, the scan over the candidates -- are
// stated once here, for the level kernels and for subtree_kernel.

__device__ __forceinline__ int bin_word_init(int w) { return w < kBinLo ? 0 : (w < kBinHi ? kKeyPosInf : kKeyNegInf); }

// the seven candidate planes of every axis of the box (bvh.c:150/154/158)
__device__ __forceinline__ void split_planes(const int* klo, const int* khi, float sp[3][7])
{
    for (int a = 0; a < 3; a++) {
        const float lo = funkey(klo[a]), hi = funkey(khi[a]);
        for (int p = 0; p < 7; p++) sp[a][p] = split_plane(lo, hi, p + 1);
    }
}

// The sphere's bin on every axis: add(bin word index, its box keys). Bin b + 1 of
// an axis is the first plane the centre is left of (7: none), never a floor.
template <class Add>
__device__ __forceinline__ void bin_sphere(const float4& g, const float sp[3][7], Add add)
{
    int kl[3], kh[3];
    sphere_keys(g, kl, kh);
    for (int a = 0; a < 3; a++) {
        const float c = comp(g, a);
        int b = 7;
        for (int p = 6; p >= 0; p--)
            if (c < sp[a][p]) b = p;
        add(a * 8 + b, kl, kh);
    }
}

__global__ void init_bins_kernel(int* bins, size_t words)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= words) return;
    bins[i] = bin_word_init((int)(i % kBinWords));
}

__global__ void bin_kernel(const float4* geo, const int* nof, int n, const BNode* nodes, int next_off, int* bins)
{
    __shared__ int sh[kBinWords];
    const int t = threadIdx.x;
    const int base = blockIdx.x * kChunk;
    const int end = min(base + kChunk, n);
    const int first = nof[base], last = nof[end - 1];
    const bool uni = first == last && first >= 0;
    // the whole workgroup sits in one leaf, or in a node the SAH kernel bins itself
    if (uni && (nodes[first].left < 0 || nodes[first].hi - nodes[first].lo <= kSmall)) return;
    if (uni) {
        for (int w = t; w < kBinWords; w += kBlock) sh[w] = bin_word_init(w);
        __syncthreads();
    }
    int ck = -1;       // node the planes below belong to
    float sp[3][7];
    int* dst = nullptr;
    for (int i = base + t; i < end; i += kBlock) {
        const int k = uni ? first : nof[i];
        if (k < 0) continue;
        if (k != ck) {
            const BNode& nd = nodes[k];
            const int left = nd.left;
            if (left < 0 || nd.hi - nd.lo <= kSmall) continue;
            ck = k;
            dst = bins + (size_t)((left - next_off) >> 1) * kBinWords;
            split_planes(nd.klo, nd.khi, sp);
        }
        bin_sphere(geo[i], sp, [&](int idx, const int* kl, const int* kh) {
            if (uni) {
                atomicAdd(&sh[idx], 1);
                for (int x = 0; x < 3; x++) {
                    atomicMin(&sh[kBinLo + idx * 3 + x], kl[x]);
                    atomicMax(&sh[kBinHi + idx * 3 + x], kh[x]);
                }
            } else {
                atomicAdd(&dst[idx], 1);
                for (int x = 0; x < 3; x++) {
                    global_min(&dst[kBinLo + idx * 3 + x], kl[x]);
                    global_max(&dst[kBinHi + idx * 3 + x], kh[x]);
                }
            }
        });
    }
    if (uni) {
        __syncthreads();
        int* out = bins + (size_t)((nodes[first].left - next_off) >> 1) * kBinWords;
        for (int w = t; w < kBinWords; w += kBlock) {
            const int v = sh[w];
            if (w < kBinLo) {
                if (v) atomicAdd(&out[w], v);
            } else if (w < kBinHi) {
                global_min(&out[w], v);
            } else {
                global_max(&out[w], v);
            }
        }
    }
}

struct KBox {
    int lo[3], hi[3];
};
__device__ __forceinline__ KBox kbox_empty()
{
    KBox b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = kKeyPosInf;
        b.hi[a] = kKeyNegInf;
    }
    return b;
}
__device__ __forceinline__ void kbox_merge(KBox& b, const int* bin, int idx)
{
    for (int a = 0; a < 3; a++) {
        b.lo[a] = min(b.lo[a], bin[kBinLo + idx * 3 + a]);
        b.hi[a] = max(b.hi[a], bin[kBinHi + idx * 3 + a]);
    }
}
__device__ __forceinline__ float kbox_area(const KBox& b)
{
    return box_area(funkey(b.hi[0]) - funkey(b.lo[0]), funkey(b.hi[1]) - funkey(b.lo[1]),
                    funkey(b.hi[2]) - funkey(b.lo[2]));
}

// The split of a node from its filled bins (bvh.c:139-170): suffix boxes, prefix
// boxes, the first candidate of the least cost, axis-major then plane-minor;
// no candidate below +inf leaves axis 0 at 0.0f.
__device__ __forceinline__ void sah_split(const int* bin, const int* klo, const int* khi, int* axis, float* split)
{
    float best_cost = INFINITY, best_split = 0.0f;  // bvh.c:139-141
    int best_axis = 0;
    for (int a = 0; a < 3; a++) {
        const float lo = funkey(klo[a]), hi = funkey(khi[a]);
        KBox right[8];
        int nr[8];
        KBox acc = kbox_empty();
        int c = 0;
        for (int i = 8; i >= 2; i--) {  // right of plane i - 1 = bins i..8
            kbox_merge(acc, bin, a * 8 + i - 1);
            c += bin[a * 8 + i - 1];
            right[i - 1] = acc;
            nr[i - 1] = c;
        }
        acc = kbox_empty();
        c = 0;
        for (int i = 1; i < 8; i++) {  // left of plane i = bins 1..i
            kbox_merge(acc, bin, a * 8 + i - 1);
            c += bin[a * 8 + i - 1];
            const float cost = sah_cost(c, kbox_area(acc), nr[i], kbox_area(right[i]));
            if (cost < best_cost) {
                best_cost = cost;
                best_axis = a;
                best_split = split_plane(lo, hi, i);
            }
        }
    }
    *axis = best_axis;
    *split = best_split;
}

__global__ void sah_kernel(const float4* geo, BNode* nodes, int off, int cnt, int next_off, const int* bins)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    BNode& nd = nodes[off + j];
    if (nd.left < 0) return;
    const int* bin = bins + (size_t)((nd.left - next_off) >> 1) * kBinWords;
    // A small node's bins are filled here, by the same rule as bin_kernel's
    // (which skips it): for the many small nodes of the deep levels nearly
    // every atomic would be the first touch of its word.
    int own[kBinWords];
    if (nd.hi - nd.lo <= kSmall) {
        for (int w = 0; w < kBinWords; w++) own[w] = bin_word_init(w);
        float sp[3][7];
        split_planes(nd.klo, nd.khi, sp);
        for (int e = nd.lo; e < nd.hi; e++)
            bin_sphere(geo[e], sp, [&](int idx, const int* kl, const int* kh) {
                own[idx]++;
                for (int x = 0; x < 3; x++) {
                    own[kBinLo + idx * 3 + x] = min(own[kBinLo + idx * 3 + x], kl[x]);
                    own[kBinHi + idx * 3 + x] = max(own[kBinHi + idx * 3 + x], kh[x]);
                }
            });
        bin = own;
    }
    sah_split(bin, nd.klo, nd.khi, &nd.axis, &nd.split);
}

// ---- partition (bvh.c:172-201 in closed form); also run by mirt_build_partition_probe

__device__ __forceinline__ bool left_flag(const float4* geo, const int* nof, const BNode* nodes, int i)
{
    const int k = nof[i];
    if (k < 0) return false;
    const BNode& nd = nodes[k];
    return nd.left >= 0 && goes_left(nd, geo[i]);
}

// rank[i] = left flags before i within its tile, tsum[tile] = flags of the tile; i runs to n inclusive
__global__ void scan_tiles_kernel(const float4* geo, const int* nof, int n, const BNode* nodes, int* rank, int* tsum)
{
    scan_tile([=](int i) { return left_flag(geo, nof, nodes, i) ? 1 : 0; }, n, n + 1, rank, &tsum[blockIdx.x]);
}

// counts of every inner node of the level, and its two children's records
__global__ void children_kernel(BNode* nodes, int off, int cnt, const int* rank, const int* tsum)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    BNode& nd = nodes[off + j];
    if (nd.left < 0) return;
    const int gb = scan_prefix(rank, tsum, nd.lo);
    const int nl = scan_prefix(rank, tsum, nd.hi) - gb;
    nd.gbase = gb;
    nd.nl = nl;
    BNode ch{};
    ch.left = -1;
    for (int a = 0; a < 3; a++) {
        ch.klo[a] = kKeyPosInf;
        ch.khi[a] = kKeyNegInf;
    }
    ch.lo = nd.lo;
    ch.hi = nd.lo + nl;
    nodes[nd.left] = ch;
    ch.lo = nd.lo + nl;
    ch.hi = nd.hi;
    nodes[nd.left + 1] = ch;
}

// jump[lo + k] = L_k for k < nl; positions >= nl are where chains end
__global__ void jump_init_kernel(const float4* geo, const int* nof, int n, const BNode* nodes, const int* rank,
                                 const int* tsum, int* jump)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int k = nof[i];
    if (k < 0) return;
    const BNode& nd = nodes[k];
    if (nd.left < 0) return;
    if (goes_left(nd, geo[i])) jump[nd.lo + (scan_prefix(rank, tsum, i) - nd.gbase)] = i;
    if (i - nd.lo >= nd.nl) jump[i] = i;
}

// One round of pointer doubling, in place. jump[j] may be read before or after
// its own update in this round; either value lies further along the same
// non-decreasing chain, so after r rounds every pointer is at least 2^r steps on.
__global__ void jump_round_kernel(const int* nof, int n, const BNode* nodes, int* jump)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int k = nof[i];
    if (k < 0) return;
    const BNode& nd = nodes[k];
    if (nd.left < 0 || i - nd.lo >= nd.nl) return;
    const int j = jump[i];
    if (j - nd.lo < nd.nl) jump[i] = jump[j];
}

// Moves every sphere of an inner node to its place and hands it to its child.
// Spheres of leaves are copied once (-1 or a leaf's index -> -2: now the same in
// both buffers) and then left alone.
__global__ void scatter_kernel(const float4* geo, const uint32_t* col, const int* nof, int n, const BNode* nodes,
                               const int* rank, const int* tsum, const int* jump, float4* geo_out,
                               uint32_t* col_out, int* nof_out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int k = nof[i];
    if (k == -2) {
        nof_out[i] = -2;
        return;
    }
    const float4 g = geo[i];
    const uint32_t cl = col[i];
    int dst = i, child = -2;
    if (k >= 0) {
        const BNode& nd = nodes[k];
        if (nd.left >= 0) {
            const int mid = nd.lo + nd.nl;
            if (goes_left(nd, g)) dst = nd.lo + (scan_prefix(rank, tsum, i) - nd.gbase);
            else if (i < mid) dst = jump[i];
            child = dst < mid ? nd.left : nd.left + 1;
        }
    }
    geo_out[dst] = g;
    col_out[dst] = cl;
    nof_out[dst] = child;
}

// ---- emission: sizes bottom-up, pre-order indices top-down

__global__ void size_kernel(BNode* nodes, int off, int cnt)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    BNode& nd = nodes[off + j];
    if (nd.left == kFinishRoot) return;  // counted by subtree_kernel's pass A
    nd.size = nd.left < 0 ? 1u : 1u + nodes[nd.left].size + nodes[nd.left + 1].size;
}

__global__ void emit_kernel(BNode* nodes, int off, int cnt, int sphere0, mirt_node* out)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const BNode& nd = nodes[off + j];
    if (nd.left == kFinishRoot) return;  // subtree_kernel's pass B writes it at nd.pre, with its subtree
    const uint32_t at = nd.pre;
    mirt_node o;
    for (int a = 0; a < 3; a++) {
        o.bmin[a] = funkey(nd.klo[a]);
        o.bmax[a] = funkey(nd.khi[a]);
    }
    if (nd.left < 0) {
        o.sphere = sphere0 + nd.lo;
        o.skip = (at + 1) | (nd.hi == nd.lo ? MIRT_NODE_EMPTY : 0u);
    } else {
        o.sphere = -1;
        o.skip = at + nd.size;
        nodes[nd.left].pre = at + 1;
        nodes[nd.left + 1].pre = at + 1 + nodes[nd.left].size;
    }
    out[at] = o;
}

// ---- the finish: one wave builds the whole subtree of one open node of at most
// kWave spheres, lane i holding the sphere at position i of the node's range.
// A pre-order walk, left child first (bvh.c:203-204), over an explicit stack of
// the open path's frames; every node by the rules above: keys for the bounds,
// bin_sphere and sah_split for the plane, the partition in closed form. All
// control flow is uniform over the wave, and waves share nothing: no workgroup
// barrier anywhere.
//   EMIT false (pass A): the spheres go back in final order, the subtree's node
//        count to the open node's `size`, which becomes a kFinishRoot;
//   EMIT true (pass B): the same walk over the spheres now in final order --
//        bounds and bins do not depend on the order, and the partition of a
//        partitioned range moves nothing (counted: kCtlMoved stays 0) -- writes
//        node k of the subtree at out[pre + k].

// LDS written by some lanes of the wave is read by others behind this
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int wave_min(int v)
{
    for (int o = kWave / 2; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = kWave / 2; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

enum { kFrLo = 0, kFrMid = 1, kFrHi = 2, kFrAt = 3, kFrStage = 4, kFrWords = 5 };

template <bool EMIT>
__global__ void __launch_bounds__(kBlock) subtree_kernel(float4* geo, uint32_t* col, BNode* nodes, int off, int cnt,
                                                         int depth0, int sphere0, mirt_node* out, int* ctl)
{
    constexpr int kWaves = kBlock / kWave;
    __shared__ float4 xg[kWaves][kWave];  // a partition's exchange
    __shared__ uint32_t xc[kWaves][kWave];
    __shared__ int lpos[kWaves][kWave];   // L_k, relative to the node's range
    __shared__ int sbin[kWaves][kBinWords];
    __shared__ int frames[kWaves][kFinishFrames][kFrWords];
    const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
    const int j = blockIdx.x * kWaves + w;
    if (j >= cnt) return;
    BNode& root = nodes[off + j];
    const int root_left = root.left;
    if (EMIT ? root_left != kFinishRoot : root_left < 0) return;
    const int base = root.lo, m = root.hi - root.lo;
    const uint32_t pre = EMIT ? root.pre : 0u, size = EMIT ? root.size : 0u;
    if (m > kWave) {  // the hand-off rule keeps every open range within one wave
        if (lane == 0) atomicOr(&ctl[kCtlError], kErrCap);
        return;
    }
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t cl = 0;
    if (lane < m) {
        g = geo[base + lane];
        cl = col[base + lane];
    }
    float4* wg = xg[w];
    uint32_t* wc = xc[w];
    int* wl = lpos[w];
    int* bin = sbin[w];
    int(*fr)[kFrWords] = frames[w];
    int sp = 0, cur = 0, moved = 0, err = 0;
    fr[0][kFrLo] = 0;
    fr[0][kFrHi] = m;
    fr[0][kFrStage] = 0;
    // a node is entered, returned to after its left subtree, and left after its right one
    for (int step = 0; sp >= 0 && step < 3 * kFinishCap; step++) {
        const int lo = uniform(fr[sp][kFrLo]), hi = uniform(fr[sp][kFrHi]), stage = uniform(fr[sp][kFrStage]);
        if (stage == 1) {
            fr[sp][kFrStage] = 2;
            fr[sp + 1][kFrLo] = uniform(fr[sp][kFrMid]);
            fr[sp + 1][kFrHi] = hi;
            fr[sp + 1][kFrStage] = 0;
            sp++;
            continue;
        }
        if (stage == 2) {
            if (EMIT && lane == 0) out[pre + (uint32_t)uniform(fr[sp][kFrAt])].skip = pre + (uint32_t)cur;
            sp--;
            continue;
        }
        if (cur >= kFinishCap) {
            err = kErrCap;
            break;
        }
        if (EMIT && (uint32_t)cur >= size) {  // pass A counted fewer: nothing is written past its count
            err = kErrSize;
            break;
        }
        const int at = cur++;
        const int n = hi - lo;
        const bool in = lane >= lo && lane < hi;
        int kl[3] = {kKeyPosInf, kKeyPosInf, kKeyPosInf}, kh[3] = {kKeyNegInf, kKeyNegInf, kKeyNegInf};
        if (in) sphere_keys(g, kl, kh);
        int klo[3], khi[3];
        for (int a = 0; a < 3; a++) {  // one sphere: its own box, from its lane; none: the inverted box
            klo[a] = n > 1 ? wave_min(kl[a]) : (n == 1 ? __builtin_amdgcn_readlane(kl[a], lo) : kKeyPosInf);
            khi[a] = n > 1 ? wave_max(kh[a]) : (n == 1 ? __builtin_amdgcn_readlane(kh[a], lo) : kKeyNegInf);
        }
        const bool leaf = n <= 1 || depth0 + sp >= kMaxDepth;  // bvh.c:131
        if (EMIT && lane == 0) {
            mirt_node o;
            for (int a = 0; a < 3; a++) {
                o.bmin[a] = funkey(klo[a]);
                o.bmax[a] = funkey(khi[a]);
            }
            o.sphere = leaf ? sphere0 + base + lo : -1;
            o.skip = leaf ? (pre + (uint32_t)at + 1u) | (n == 0 ? MIRT_NODE_EMPTY : 0u) : 0u;  // inner: set at stage 2
            out[pre + (uint32_t)at] = o;
        }
        if (leaf) {
            sp--;
            continue;
        }
        if (sp + 1 >= kFinishFrames) {  // an inner node lies above depth 40: its child has a frame
            err = kErrCap;
            break;
        }
        for (int x = lane; x < kBinWords; x += kWave) bin[x] = bin_word_init(x);
        float pl[3][7];
        split_planes(klo, khi, pl);
        wave_sync();
        if (in)
            bin_sphere(g, pl, [&](int idx, const int* bl, const int* bh) {
                atomicAdd(&bin[idx], 1);
                for (int x = 0; x < 3; x++) {
                    atomicMin(&bin[kBinLo + idx * 3 + x], bl[x]);
                    atomicMax(&bin[kBinHi + idx * 3 + x], bh[x]);
                }
            });
        wave_sync();
        int axis;
        float split;
        sah_split(bin, klo, khi, &axis, &split);
        // the partition (bvh.c:172-201 in closed form, as scatter_kernel's)
        const bool left = in && goes_left(axis, split, g);
        const unsigned long long mask = __ballot(left) >> lo;
        const int p = lane - lo, nl = __popcll(mask);
        int dst = p;
        if (left) {
            dst = __popcll(mask & ((1ull << p) - 1ull));
            wl[dst] = p;
        }
        wave_sync();
        if (in && !left)
            for (int k = 0; k < kWave && dst < nl; k++) dst = wl[dst];
        moved += __popcll(__ballot(in && dst != p));
        if (in) {
            wg[lo + dst] = g;
            wc[lo + dst] = cl;
        }
        wave_sync();
        if (in) {
            g = wg[lane];
            cl = wc[lane];
        }
        wave_sync();
        fr[sp][kFrMid] = lo + nl;
        fr[sp][kFrAt] = at;
        fr[sp][kFrStage] = 1;
        fr[sp + 1][kFrLo] = lo;
        fr[sp + 1][kFrHi] = lo + nl;
        fr[sp + 1][kFrStage] = 0;
        sp++;
    }
    if (sp >= 0 && !err) err = kErrCap;  // the step bound ended the walk
    if (!EMIT) {
        if (lane < m) {
            geo[base + lane] = g;
            col[base + lane] = cl;
        }
        if (lane == 0) {
            root.size = (uint32_t)cur;
            root.left = kFinishRoot;
            atomicAdd((unsigned long long*)&ctl[kCtlFinNodes], (unsigned long long)cur);
        }
    } else if (lane == 0 && moved) {
        atomicAdd(&ctl[kCtlMoved], moved);
    }
    if (lane == 0 && err) atomicOr(&ctl[kCtlError], err);
}

// ---- host side

struct Buf {
    void* p = nullptr;
    size_t cap = 0;
};

// at least `bytes`; keep: the first `keep` bytes survive a move
int ensure(Buf& b, size_t bytes, hipStream_t s = nullptr, size_t keep = 0)
{
    if (bytes <= b.cap) return MIRT_OK;
    if (keep) bytes = std::max(bytes, b.cap + b.cap / 2);
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    if (keep && b.p) {
        hipError_t e = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return hip_fail(e, "mirt device build: moving the node array");
        }
    }
    if (b.p) (void)hipFree(b.p);
    b.p = p;
    b.cap = bytes;
    return MIRT_OK;
}

}  // namespace

namespace mirt {

// Device scratch of the builds of one ctx: grown on demand, released by mirt_destroy.
struct BuildState {
    Buf aos, geo[2], col[2], nof[2], rank, tsum, jump, nodes, bins, ctl, out;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evf[4] = {nullptr, nullptr, nullptr, nullptr};  // around the finish's pass A and pass B
    mirt_build_stats stats{};
    bool have_stats = false;
    mirt_build_finish_stats fin{};  // of the last device build, whichever entry point ran it
    bool have_fin = false;
};

void build_state_free(BuildState* st)
{
    if (!st) return;
    for (Buf* b : {&st->aos, &st->geo[0], &st->geo[1], &st->col[0], &st->col[1], &st->nof[0], &st->nof[1], &st->rank,
                   &st->tsum, &st->jump, &st->nodes, &st->bins, &st->ctl, &st->out})
        if (b->p) (void)hipFree(b->p);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    for (hipEvent_t e : st->evf)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

}  // namespace mirt

namespace {

using mirt::BuildState;

int get_state(mirt_ctx* c, BuildState** out)
{
    BuildState** slot = mirt::ctx_build_state(c);
    if (!*slot) {
        BuildState* st = new (std::nothrow) BuildState();
        if (!st) {
            mirt::set_error("mirt device build: out of host memory");
            return MIRT_E_NOMEM;
        }
        *slot = st;  // owned by the ctx from here on
        HIP_TRY(hipEventCreate(&st->ev0));
        HIP_TRY(hipEventCreate(&st->ev1));
        for (hipEvent_t& e : st->evf) HIP_TRY(hipEventCreate(&e));
    }
    if (!(*slot)->ev0 || !(*slot)->ev1 || !(*slot)->evf[3]) {
        mirt::set_error("mirt device build: the context's build state could not be set up");
        return MIRT_E_DEVICE;
    }
    *out = *slot;
    return MIRT_OK;
}

int ensure_spheres(BuildState& st, int n)
{
    const size_t m = (size_t)std::max(n, 1);
    const size_t tiles = ((size_t)n + 1 + kTile - 1) / kTile;
    int rc = MIRT_OK;
    for (int k = 0; k < 2 && !rc; k++) {
        rc = ensure(st.geo[k], m * sizeof(float4));
        if (!rc) rc = ensure(st.col[k], m * 4);
        if (!rc) rc = ensure(st.nof[k], m * 4);
    }
    if (!rc) rc = ensure(st.rank, tiles * kTile * 4);
    if (!rc) rc = ensure(st.tsum, tiles * 4);
    if (!rc) rc = ensure(st.jump, m * 4);
    if (!rc) rc = ensure(st.ctl, kCtlWords * 4);
    return rc;
}

// Partitions every inner node among nodes[off, off + cnt) of buffer `cur` into
// buffer 1 - cur. max_range: the longest inner range (bounds the chains).
int run_partition(BuildState& st, hipStream_t s, int cur, int n, int off, int cnt, int max_range)
{
    if (n <= 0) return MIRT_OK;
    const float4* geo = (const float4*)st.geo[cur].p;
    const uint32_t* col = (const uint32_t*)st.col[cur].p;
    const int* nof = (const int*)st.nof[cur].p;
    BNode* nodes = (BNode*)st.nodes.p;
    int *rank = (int*)st.rank.p, *tsum = (int*)st.tsum.p, *jump = (int*)st.jump.p;
    const int tiles = (int)(((size_t)n + 1 + kTile - 1) / kTile);
    scan_tiles_kernel<<<tiles, kBlock, 0, s>>>(geo, nof, n, nodes, rank, tsum);
    scan_sums_kernel<kSumBlock><<<1, kSumBlock, 0, s>>>(tsum, tiles, nullptr);
    children_kernel<<<blocks(cnt, kBlock), kBlock, 0, s>>>(nodes, off, cnt, rank, tsum);
    const unsigned g = blocks(n, kBlock);
    jump_init_kernel<<<g, kBlock, 0, s>>>(geo, nof, n, nodes, rank, tsum, jump);
    int rounds = 0;
    while (((long long)1 << rounds) < (long long)max_range) rounds++;
    for (int r = 0; r < rounds; r++) jump_round_kernel<<<g, kBlock, 0, s>>>(nof, n, nodes, jump);
    scatter_kernel<<<g, kBlock, 0, s>>>(geo, col, nof, n, nodes, rank, tsum, jump, (float4*)st.geo[1 - cur].p,
                                        (uint32_t*)st.col[1 - cur].p, (int*)st.nof[1 - cur].p);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// The build proper, left on the device: `total` spheres go to st.aos, the tree
// of the n of them from `first` on is built (leaf indices count from sphere0)
// and stays in st.out, *out_count nodes; st.aos then holds all `total` spheres
// with that range reordered. Enqueued, not waited for: download() or the
// caller synchronises. *declined = 1: nothing was built, the host builder must run.
// d_src set: the spheres come from device memory instead, tagged by tag_kernel
// (d_colour[total] receives their colours).
int device_build(mirt_ctx* c, BuildState& st, const mirt_sphere* spheres, int total, int first, int n, int sphere0,
                 int depth, int* out_count, int* declined, int* levels_out, const uint32_t* d_src = nullptr,
                 uint32_t* d_colour = nullptr)
{
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    *declined = 0;
    st.have_fin = false;
    // MIRT_OPT_BUILD_FINISH: the longest open range the finish takes (0: off); automatic: a whole
    // wave up to kFinishAutoMax spheres, off beyond (MEASUREMENTS.md E)
    const int opt = mirt::ctx_build_finish(c);
    const int F = opt == 1 ? (n <= kFinishAutoMax ? kWave : 0) : opt;
    mirt_build_finish_stats fin{};
    fin.range = F;
    fin.round = -1;
    int rc = ensure_spheres(st, n);
    if (!rc) rc = ensure(st.aos, (size_t)std::max(total, 1) * sizeof(mirt_sphere));
    if (!rc) rc = ensure(st.nodes, ((size_t)2 * (size_t)n + 64) * sizeof(BNode));
    if (rc) return rc;
    int* ctl = (int*)st.ctl.p;
    int h_ctl[kCtlWords] = {};
    int cur = 0;
    HIP_TRY(hipMemsetAsync(ctl, 0, kCtlWords * 4, s));
    if (total > 0 && d_src) {
        const size_t words = 5 * (size_t)total;
        tag_kernel<<<blocks(words, kBlock), kBlock, 0, s>>>(d_src, words, (uint32_t*)st.aos.p, d_colour);
        HIP_TRY(hipGetLastError());
    } else if (total > 0) {
        HIP_TRY(hipMemcpyAsync(st.aos.p, spheres, (size_t)total * sizeof(mirt_sphere), hipMemcpyHostToDevice, s));
    }
    uint32_t* aos = (uint32_t*)st.aos.p + 5 * (size_t)first;  // the range being built
    HIP_TRY(hipEventRecord(st.ev0, s));
    if (n > 0) {
        prep_kernel<<<blocks(n, kBlock), kBlock, 0, s>>>(aos, n, (float4*)st.geo[0].p,
                                                        (uint32_t*)st.col[0].p, (int*)st.nof[0].p, ctl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctl, ctl, kCtlWords * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_ctl[kCtlDeclined]) {
            *declined = 1;
            st.fin = fin;
            st.have_fin = true;
            return MIRT_OK;
        }
    }
    root_kernel<<<1, 1, 0, s>>>((BNode*)st.nodes.p, n);
    std::vector<int> level_off, level_cnt;
    int off = 0, cnt = 1;
    for (int d = depth;; d++) {
        level_off.push_back(off);
        level_cnt.push_back(cnt);
        BNode* nodes = (BNode*)st.nodes.p;
        const unsigned gn = blocks(cnt, kBlock);
        if (n > 0)
            bounds_kernel<<<blocks(n, kChunk), kBlock, 0, s>>>((const float4*)st.geo[cur].p, (const int*)st.nof[cur].p,
                                                              n, nodes);
        HIP_TRY(hipMemsetAsync(ctl, 0, 2 * 4, s));
        classify_kernel<<<gn, kBlock, 0, s>>>(nodes, off, cnt, off + cnt, d >= kMaxDepth ? 1 : 0, ctl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_ctl, ctl, 2 * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const int inner = h_ctl[kCtlInner];
        if (inner <= 0) break;
        if (inner > cnt || (size_t)off + (size_t)cnt + 2 * (size_t)inner > (size_t)INT32_MAX) {
            mirt::set_error("mirt_bvh_build_flat_device: the tree exceeds 2^31 nodes");
            return MIRT_E_INVALID;
        }
        // the hand-off: every open node of this level fits one wave of the finish
        if (F > 0 && d >= 0 && h_ctl[kCtlMaxRange] <= F) {
            fin.round = (int)level_off.size() - 1;
            fin.subtrees = inner;
            break;
        }
        // the next level, sized from the count just read
        const size_t have = (size_t)off + (size_t)cnt;
        rc = ensure(st.nodes, (have + 2 * (size_t)inner) * sizeof(BNode), s, have * sizeof(BNode));
        if (!rc) rc = ensure(st.bins, (size_t)inner * kBinWords * 4);
        if (rc) return rc;
        nodes = (BNode*)st.nodes.p;
        int* bins = (int*)st.bins.p;
        const size_t words = (size_t)inner * kBinWords;
        init_bins_kernel<<<blocks(words, kBlock), kBlock, 0, s>>>(bins, words);
        bin_kernel<<<blocks(n, kChunk), kBlock, 0, s>>>((const float4*)st.geo[cur].p, (const int*)st.nof[cur].p, n,
                                                       nodes, off + cnt, bins);
        sah_kernel<<<gn, kBlock, 0, s>>>((const float4*)st.geo[cur].p, nodes, off, cnt, off + cnt, bins);
        HIP_TRY(hipGetLastError());
        rc = run_partition(st, s, cur, n, off, cnt, h_ctl[kCtlMaxRange]);
        if (rc) return rc;
        cur = 1 - cur;
        off += cnt;
        cnt = 2 * inner;
    }
    size_t total_nodes = (size_t)off + (size_t)cnt;
    const unsigned fin_grid = blocks((size_t)cnt * kWave, kBlock);  // one wave per node of the hand-off level
    if (fin.round >= 0) {
        // pass A: the spheres in final order, every subtree's node count; the total sizes the output
        HIP_TRY(hipEventRecord(st.evf[0], s));
        subtree_kernel<false><<<fin_grid, kBlock, 0, s>>>((float4*)st.geo[cur].p, (uint32_t*)st.col[cur].p,
                                                          (BNode*)st.nodes.p, off, cnt, depth + fin.round, sphere0,
                                                          nullptr, ctl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(st.evf[1], s));
        HIP_TRY(hipMemcpyAsync(h_ctl, ctl, kCtlWords * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_ctl[kCtlError]) {
            mirt::set_error("mirt device build: a subtree walk of the finish reached its cap (code %d)",
                            h_ctl[kCtlError]);
            return MIRT_E_DEVICE;
        }
        unsigned long long fin_nodes = 0;
        std::memcpy(&fin_nodes, &h_ctl[kCtlFinNodes], 8);
        total_nodes = total_nodes - (size_t)fin.subtrees + (size_t)fin_nodes;
        if (fin_nodes > (unsigned long long)INT32_MAX || total_nodes > (size_t)INT32_MAX) {
            mirt::set_error("mirt_bvh_build_flat_device: the tree exceeds 2^31 nodes");
            return MIRT_E_INVALID;
        }
        fin.nodes = (int)fin_nodes;
    }
    rc = ensure(st.out, total_nodes * sizeof(mirt_node));
    if (rc) return rc;
    BNode* nodes = (BNode*)st.nodes.p;
    const int nl = (int)level_off.size();
    for (int l = nl - 1; l >= 0; l--)
        size_kernel<<<blocks(level_cnt[l], kBlock), kBlock, 0, s>>>(nodes, level_off[l], level_cnt[l]);
    for (int l = 0; l < nl; l++)
        emit_kernel<<<blocks(level_cnt[l], kBlock), kBlock, 0, s>>>(nodes, level_off[l], level_cnt[l], sphere0,
                                                                   (mirt_node*)st.out.p);
    if (fin.round >= 0) {
        // pass B: every finish root knows its place now; the subtrees are written there
        HIP_TRY(hipEventRecord(st.evf[2], s));
        subtree_kernel<true><<<fin_grid, kBlock, 0, s>>>((float4*)st.geo[cur].p, (uint32_t*)st.col[cur].p, nodes, off,
                                                         cnt, depth + fin.round, sphere0, (mirt_node*)st.out.p, ctl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(st.evf[3], s));
    }
    if (n > 0)
        finish_kernel<<<blocks(n, kBlock), kBlock, 0, s>>>((const float4*)st.geo[cur].p, (const uint32_t*)st.col[cur].p,
                                                          n, aos);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev1, s));
    if (fin.round >= 0) {
        // the control words of pass B, read once with the result
        HIP_TRY(hipMemcpyAsync(h_ctl, ctl, kCtlWords * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        fin.moved = h_ctl[kCtlMoved];
        if (h_ctl[kCtlError] || fin.moved) {
            mirt::set_error("mirt device build: pass B of the finish disagrees with pass A (code %d, %d spheres moved)",
                            h_ctl[kCtlError], fin.moved);
            return MIRT_E_DEVICE;
        }
        float a = 0.0f, b = 0.0f;
        HIP_TRY(hipEventElapsedTime(&a, st.evf[0], st.evf[1]));
        HIP_TRY(hipEventElapsedTime(&b, st.evf[2], st.evf[3]));
        fin.finish_ms = a + b;
    }
    st.fin = fin;
    st.have_fin = true;
    *out_count = (int)total_nodes;
    *levels_out = nl;
    return MIRT_OK;
}

// the built tree and the n reordered spheres (the first n of st.aos) to the host
int download(mirt_ctx* c, BuildState& st, mirt_sphere* spheres, int n, int count, mirt_node** out_nodes)
{
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    const size_t total = (size_t)count;
    mirt_node* out = (mirt_node*)std::malloc(total * sizeof(mirt_node));
    if (!out) {
        (void)hipStreamSynchronize(s);
        mirt::set_error("mirt_bvh_build_flat_device: out of host memory");
        return MIRT_E_NOMEM;
    }
    hipError_t e = hipMemcpyAsync(out, st.out.p, total * sizeof(mirt_node), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the tree is complete before the caller's spheres change
    if (e == hipSuccess && n > 0)
        e = hipMemcpyAsync(spheres, st.aos.p, (size_t)n * sizeof(mirt_sphere), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        std::free(out);
        (void)hipStreamSynchronize(s);
        return hip_fail(e, "mirt_bvh_build_flat_device");
    }
    *out_nodes = out;
    return MIRT_OK;
}

}  // namespace

namespace mirt {

namespace {
int build_resident_from(mirt_ctx* c, const mirt_sphere* spheres, const uint32_t* d_src, uint32_t* d_colour, int total,
                        int start, int end, int depth, ResidentTree* out, int* declined)
{
    BuildState* st = nullptr;
    if (int rc = get_state(c, &st)) return rc;
    int count = 0, levels = 0;
    if (int rc = device_build(c, *st, spheres, total, start, end - start, start, depth, &count, declined, &levels,
                              d_src, d_colour)) {
        (void)hipStreamSynchronize((hipStream_t)mirt_ctx_stream(c));
        return rc;
    }
    out->aos = (const uint32_t*)st->aos.p;
    out->nodes = (const mirt_node*)st->out.p;
    out->num_nodes = count;
    out->levels = levels;
    return MIRT_OK;
}
}  // namespace

int build_resident(mirt_ctx* c, const mirt_sphere* spheres, int total, int start, int end, int depth,
                   ResidentTree* out, int* declined)
{
    return build_resident_from(c, spheres, nullptr, nullptr, total, start, end, depth, out, declined);
}

int build_resident_tagged(mirt_ctx* c, const void* d_spheres, int total, int start, int end, int depth,
                          uint32_t* d_colour, ResidentTree* out, int* declined)
{
    return build_resident_from(c, nullptr, (const uint32_t*)d_spheres, d_colour, total, start, end, depth, out,
                               declined);
}

int build_resident_ms(mirt_ctx* c, float* ms)
{
    BuildState* st = *ctx_build_state(c);
    if (!st || !st->ev0 || !st->ev1) {
        set_error("mirt device build: no build has run on this context");
        return MIRT_E_INVALID;
    }
    HIP_TRY(hipEventElapsedTime(ms, st->ev0, st->ev1));
    return MIRT_OK;
}

}  // namespace mirt

extern "C" {

int mirt_bvh_build_flat_device(mirt_ctx* c, mirt_sphere* spheres, int start, int end, int depth,
                               mirt_node** out_nodes, int* out_count)
try {
    if (!c) {
        mirt::set_error("mirt_bvh_build_flat_device: null context");
        return MIRT_E_INVALID;
    }
    if (!spheres || !out_nodes || !out_count || start < 0 || end < start) {
        mirt::set_error("mirt_bvh_build_flat_device: invalid arguments");
        return MIRT_E_INVALID;
    }
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(mirt::ctx_device(c)));
    BuildState* st = nullptr;
    if (int rc = get_state(c, &st)) return rc;
    st->have_stats = false;
    int declined = 0, levels = 0, count = 0;
    const int n = end - start;
    int rc = device_build(c, *st, spheres + start, n, 0, n, start, depth, &count, &declined, &levels);
    if (!rc && !declined) rc = download(c, *st, spheres + start, n, count, out_nodes);
    if (rc) {
        (void)hipStreamSynchronize((hipStream_t)mirt_ctx_stream(c));
        return rc;
    }
    if (!declined) *out_count = count;
    mirt_build_stats bs{};
    if (declined) {
        rc = mirt_bvh_build_flat(spheres, start, end, depth, out_nodes, out_count);
        if (rc) return rc;
    } else {
        bs.on_device = 1;
        bs.levels = levels;
        HIP_TRY(hipEventElapsedTime(&bs.device_ms, st->ev0, st->ev1));
    }
    bs.nodes = *out_count;
    bs.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->stats = bs;
    st->have_stats = true;
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    mirt::set_error("mirt_bvh_build_flat_device: out of host memory");
    return MIRT_E_NOMEM;
}

int mirt_last_build_stats(mirt_ctx* c, mirt_build_stats* out)
{
    if (!c || !out) {
        mirt::set_error("mirt_last_build_stats: null context or output");
        return MIRT_E_INVALID;
    }
    const BuildState* st = *mirt::ctx_build_state(c);
    if (!st || !st->have_stats) {
        mirt::set_error("mirt_last_build_stats: no device build has finished on this context");
        return MIRT_E_INVALID;
    }
    *out = st->stats;
    return MIRT_OK;
}

int mirt_last_build_finish(mirt_ctx* c, mirt_build_finish_stats* out)
{
    if (!c || !out) {
        mirt::set_error("mirt_last_build_finish: null context or output");
        return MIRT_E_INVALID;
    }
    const BuildState* st = *mirt::ctx_build_state(c);
    if (!st || !st->have_fin) {
        mirt::set_error("mirt_last_build_finish: no device build has finished on this context");
        return MIRT_E_INVALID;
    }
    *out = st->fin;
    return MIRT_OK;
}

int mirt_build_partition_probe(mirt_ctx* c, const float* centre, int n, const int32_t* seg, int nseg,
                               const float* split, int32_t* perm)
try {
    if (!c) {
        mirt::set_error("mirt_build_partition_probe: null context");
        return MIRT_E_INVALID;
    }
    bool ok = n >= 0 && nseg >= 0 && seg && (nseg == 0 || split) && (n == 0 || (centre && perm));
    for (int k = 0; ok && k <= nseg; k++) ok = seg[k] >= (k ? seg[k - 1] : 0) && seg[k] <= n;
    if (!ok) {
        mirt::set_error("mirt_build_partition_probe: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (n == 0) return MIRT_OK;
    // the build's inputs: keys on axis 0, the source index as the payload,
    // segment k as inner node k with children 3k.. behind the segments
    std::vector<float4> geo((size_t)n);
    std::vector<int32_t> col((size_t)n), nof((size_t)n, -1);
    std::vector<BNode> nodes((size_t)3 * (size_t)nseg + 1);
    int max_range = 0;
    for (int i = 0; i < n; i++) {
        geo[i] = make_float4(centre[i], 0.0f, 0.0f, 0.0f);
        col[i] = i;
    }
    for (int k = 0; k < nseg; k++) {
        BNode nd{};
        nd.lo = seg[k];
        nd.hi = seg[k + 1];
        nd.left = nseg + 2 * k;
        nd.axis = 0;
        nd.split = split[k];
        nodes[k] = nd;
        for (int i = nd.lo; i < nd.hi; i++) nof[i] = k;
        max_range = std::max(max_range, nd.hi - nd.lo);
    }
    HIP_TRY(hipSetDevice(mirt::ctx_device(c)));
    BuildState* st = nullptr;
    if (int rc = get_state(c, &st)) return rc;
    int rc = ensure_spheres(*st, n);
    if (!rc) rc = ensure(st->nodes, nodes.size() * sizeof(BNode));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    HIP_TRY(hipMemcpyAsync(st->geo[0].p, geo.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st->col[0].p, col.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st->nof[0].p, nof.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st->nodes.p, nodes.data(), nodes.size() * sizeof(BNode), hipMemcpyHostToDevice, s));
    if (nseg > 0) {
        rc = run_partition(*st, s, 0, n, 0, nseg, max_range);
        if (rc) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
    } else {
        HIP_TRY(hipMemcpyAsync(st->col[1].p, st->col[0].p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    }
    hipError_t e = hipMemcpyAsync(perm, st->col[1].p, (size_t)n * 4, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // the host vectors above outlive the copies
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return hip_fail(e, "mirt_build_partition_probe");
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    mirt::set_error("mirt_build_partition_probe: out of host memory");
    return MIRT_E_NOMEM;
}

}  // extern "C"

// The device layouts of a scene (layout.h) derived ON the device from the raw
// spheres and a flat pre-order tree already there: what scene_layout.cpp's
// build_scene_layout derives on the host, byte for byte, so a tree built by
// bvh_device.hip never has to leave HBM (mirt_scene_build_device), and a tree
// that comes from the host crosses the link once, raw
// (mirt_scene_upload_flat_device). One code path for any validated tree.
//
// scene_layout.cpp walks the tree serially; here every numbering it hands out
// is recovered from pre-order alone:
//   scalars   r_max, c_max, the coordinate bound and the "any" flags (a
//             non-finite sphere, a box that does not nest, an orphaned
//             phantom) are max / or reductions: exact in any order. The bound
//             itself, cb (1 + 2^-10) + 2^-10 in double, is formed on the host
//             from the reduced maxima by layout_rules.h's layout_bound, which
//             scene_layout.cpp calls too;
//   PNodes    pidx = 1 + the rank of an inner node among the inner nodes in
//             pre-order: an exclusive prefix sum of the inner flags;
//   depth     of node i = inner nodes before i - inner subtrees that end at or
//             before i: a second prefix sum, over a histogram of subtree ends.
//             ndepth is that clamped to 255, the packet walk's stack bound the
//             maximum over inner nodes;
//   mono      every hit-able leaf is compacted (a third prefix sum, which also
//             gives the leaf count) and compared with the one before it;
//   HNodes    build_hnodes fills HNodes breadth-first from a queue and numbers
//             leaves as slots are filled. Level by level: each HNode of a level
//             computes its slots, an ORDERED exclusive scan over (HNode, slot)
//             hands out the next level's HNode indices and the leaf indices,
//             and the level's two totals are read back once: the next launch
//             is sized from them, never guessed.
// Every kernel loop is bounded at launch; no workgroup waits on another. The
// arithmetic and the per-node decisions (outward rounding, the HNode cut, a
// PNode child, a slot's packed box) are layout_rules.h's, the functions
// scene_layout.cpp calls: only the numbering is stated twice.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "device_util.h"
#include "internal.h"
#include "layout.h"
#include "layout_rules.h"

#pragma clang fp contract(off)

namespace {

using namespace mirt;

constexpr int kBlock = kScanBlock;
constexpr int kTile = kScanTile;  // elements per workgroup of the prefix sums

// ctl words (device, read back by the host)
enum {
    kBadSphere = 0,  // a non-finite sphere
    kBadNest,        // a box that does not hold its sphere / its children
    kOrphan,         // orphan_phantoms
    kRMax,           // float bits (non-negative floats order as ints)
    kCMax,
    kBoxMax,         // largest finite |coordinate| of a non-empty node's box
    kNotMono,
    kDepth,          // open inner nodes at the deepest inner node
    kTotInner,       // totals of the three prefix sums over the nodes
    kTotClose,
    kTotLive,
    kLvlInner,       // totals of the two prefix sums over an HNode level
    kLvlLeaf,
    kOverflow,       // an index beyond an array's capacity was refused
    kCtlWords = 16
};

__device__ __forceinline__ bool finite_bits(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }

// ---- prefix sums: `arrays` arrays of n ints, `stride` apart, each made exclusive within its tiles

__global__ void scan_tiles_kernel(int* data, size_t stride, int n, int* tsum, int tiles)
{
    int* d = data + stride * blockIdx.y;
    scan_tile([=](int i) { return d[i]; }, n, n, d, &tsum[(size_t)tiles * blockIdx.y + blockIdx.x]);
}

// ---- spheres: geo / color with their sentinels, r_max, c_max, the finite check

__global__ void spheres_kernel(const uint32_t* aos, int ns, float4* geo, uint32_t* color, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > ns) return;
    if (i == ns) {  // &spheres[N]: never hits
        const float q = __uint_as_float(0x7fc00000u);
        geo[i] = make_float4(q, q, q, q);
        color[i] = 0xff000000u;
        return;
    }
    const uint32_t* s = aos + 5 * (size_t)i;
    const uint32_t w[4] = {s[0], s[1], s[2], s[3]};
    geo[i] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
    color[i] = s[4];
    if (!finite_bits(w[0]) || !finite_bits(w[1]) || !finite_bits(w[2]) || !finite_bits(w[3])) {
        flag(ctl, kBadSphere);
        return;
    }
    const float r = fabsf(__uint_as_float(w[3]));
    const float a0 = fabsf(__uint_as_float(w[0])), a1 = fabsf(__uint_as_float(w[1])), a2 = fabsf(__uint_as_float(w[2]));
    const float m = fmaxf(a0, fmaxf(a1, a2)) + r;
    global_max(&ctl[kRMax], (int)__float_as_uint(r));
    global_max(&ctl[kCMax], (int)__float_as_uint(m));
}

// ---- nodes: DNodes, the nesting check, the three flag arrays, the coordinate bound

// is_inner / closes / is_live: three arrays of nn + 1 ints, zeroed; tested: ns + 1 bytes, zeroed
__global__ void nodes_kernel(const mirt_node* nd, int nn, const uint32_t* aos, int ns, uint32_t* dnodes, int* is_inner,
                             int* closes, int* is_live, uint8_t* tested, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    const mirt_node n = nd[i];
    const bool inner = n.sphere < 0, empty = (n.skip & MIRT_NODE_EMPTY) != 0;
    const bool live = hitable(n, ns);
    uint32_t g[4] = {0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u};
    if (!inner && n.sphere < ns)
        for (int k = 0; k < 4; k++) g[k] = aos[5 * (size_t)n.sphere + k];
    uint32_t* d = dnodes + 16 * (size_t)i;
    for (int k = 0; k < 3; k++) {
        d[k] = __float_as_uint(n.bmin[k]);
        d[3 + k] = __float_as_uint(n.bmax[k]);
    }
    d[6] = (uint32_t)n.sphere;
    d[7] = n.skip;
    for (int k = 0; k < 4; k++) {
        d[8 + k] = g[k];
        d[12 + k] = 0u;
    }
    is_inner[i] = inner ? 1 : 0;
    is_live[i] = live ? 1 : 0;
    if (inner) atomicAdd(&closes[min(skip_of(n), (uint32_t)nn)], 1);
    if (live) tested[n.sphere] = 1;
    if (empty) return;
    for (int k = 0; k < 3; k++) {
        const uint32_t lo = __float_as_uint(n.bmin[k]), hi = __float_as_uint(n.bmax[k]);
        if (finite_bits(lo)) global_max(&ctl[kBoxMax], (int)(lo & 0x7fffffffu));
        if (finite_bits(hi)) global_max(&ctl[kBoxMax], (int)(hi & 0x7fffffffu));
    }
    bool ok = true;
    if (!inner) {
        if (n.sphere >= ns) return;  // the never-hit sentinel
        const float c[3] = {__uint_as_float(g[0]), __uint_as_float(g[1]), __uint_as_float(g[2])};
        const float r = fabsf(__uint_as_float(g[3]));
        for (int k = 0; k < 3; k++)
            if (!(n.bmin[k] <= c[k] - r && n.bmax[k] >= c[k] + r)) ok = false;
    } else if (i + 1 < nn) {
        const mirt_node left = nd[i + 1];
        const uint32_t right = skip_of(left);
        if (!holds(n, left)) ok = false;
        if (right < (uint32_t)nn && right < skip_of(n) && !holds(n, nd[right])) ok = false;
    }
    if (!ok) flag(ctl, kBadNest);
}

__global__ void orphan_kernel(const mirt_node* nd, int nn, int ns, const uint8_t* tested, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    const mirt_node n = nd[i];
    if (n.sphere >= 0 && n.sphere < ns && (n.skip & MIRT_NODE_EMPTY) && !tested[n.sphere]) flag(ctl, kOrphan);
}

// after the prefix sums: depths, and the hit-able leaves' spheres in DFS order
__global__ void depth_kernel(const mirt_node* nd, int nn, int ns, const int* is_inner, const int* closes,
                             const int* is_live, const int* tsum, int tiles, uint8_t* ndepth, int* compact, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    const mirt_node n = nd[i];
    const int depth = scan_prefix(is_inner, tsum, i) - scan_prefix(closes, tsum + tiles, i + 1);
    ndepth[i] = (uint8_t)min(max(depth, 0), 255);
    if (n.sphere < 0) global_max(&ctl[kDepth], depth + 1);
    if (hitable(n, ns)) {
        const int k = scan_prefix(is_live, tsum + 2 * (size_t)tiles, i);
        if (k < nn) compact[k] = n.sphere;
    }
}

__global__ void mono_kernel(const int* compact, int nn, int* ctl)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k < 1 || k >= nn || k >= ctl[kTotLive]) return;
    if (compact[k] <= compact[k - 1]) flag(ctl, kNotMono);
}

// ---- PNodes (scene_layout.cpp build_pnodes / set_child)

__device__ void set_child(const mirt_node* nd, int nn, int ns, const int* is_inner, const int* tsum, double grow,
                          uint32_t c, uint32_t* slot, uint32_t* ref_out)
{
    const uint32_t ci = live_node(nd, nn, ns, c);
    const bool inner = ci != kPNone && nd[ci].sphere < 0;
    const uint32_t pidx = inner ? 1u + (uint32_t)scan_prefix(is_inner, tsum, (int)ci) : kPNone;
    float box[6];
    *ref_out = pnode_child(nd, ns, grow, c, ci, pidx, box);
    for (int k = 0; k < 6; k++) slot[k] = __float_as_uint(box[k]);
}

// thread i < nn: the PNode of inner node i; thread nn: PNode 0, the virtual parent of the root
__global__ void pnodes_kernel(const mirt_node* nd, int nn, int ns, const int* is_inner, const int* tsum, double grow,
                              uint32_t* pnodes, uint32_t cap)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > nn) return;
    uint32_t w[16];
    for (int k = 0; k < 16; k++) w[k] = 0u;
    uint32_t at = 0;
    if (i == nn) {
        w[12] = w[13] = kPNone;
        w[14] = 0xffffffffu;  // flat + 1 == 0: the whole tree
        w[15] = (uint32_t)nn;
        if (nn > 0) set_child(nd, nn, ns, is_inner, tsum, grow, 0u, &w[0], &w[12]);
    } else {
        const mirt_node n = nd[i];
        if (n.sphere >= 0 || i + 1 >= nn) return;
        at = 1u + (uint32_t)scan_prefix(is_inner, tsum, i);
        set_child(nd, nn, ns, is_inner, tsum, grow, (uint32_t)i + 1u, &w[0], &w[12]);
        const uint32_t r = skip_of(nd[i + 1]);
        if (r < (uint32_t)nn) set_child(nd, nn, ns, is_inner, tsum, grow, r, &w[6], &w[13]);
        w[14] = (uint32_t)i;
        w[15] = skip_of(n);
    }
    if (at >= cap) return;
    uint32_t* p = pnodes + 16 * (size_t)at;
    for (int k = 0; k < 16; k++) p[k] = w[k];
}

// ---- HNodes (scene_layout.cpp build_hnodes), one level per launch

struct HOut {
    uint32_t* hnodes;   // 16 words each
    uint32_t* haux;     // 2 words each
    float4* leaf_geo;
    uint32_t* leaf_box; // 8 words each
    uint32_t cap_h, cap_l;
};

// One slot (scene_layout.cpp fill) for live flat node ci: its box in fp16 rounded outward; an inner node takes
// HNode index *next_h, a leaf leaf index *next_l.
__device__ void fill_slot(const mirt_node* nd, int ns, const uint32_t* aos, double grow, const HOut& o, uint32_t ci,
                          uint32_t* slot, uint32_t* next_h, uint32_t* next_l, int* ctl)
{
    const mirt_node n = nd[ci];
    hnode_slot_box(n, grow, slot);
    uint32_t ref = kPNone;
    if (n.skip & MIRT_NODE_EMPTY) {
        ref = kPNone;
    } else if (n.sphere >= 0) {
        if (n.sphere < ns) {
            const uint32_t li = (*next_l)++;
            if (li < o.cap_l) {
                uint32_t* b = o.leaf_box + 8 * (size_t)li;
                for (int k = 0; k < 3; k++) {
                    b[k] = __float_as_uint(n.bmin[k]);
                    b[3 + k] = __float_as_uint(n.bmax[k]);
                }
                b[6] = (uint32_t)n.sphere;
                b[7] = 0u;
                const uint32_t* s = aos + 5 * (size_t)n.sphere;
                o.leaf_geo[li] = make_float4(__uint_as_float(s[0]), __uint_as_float(s[1]), __uint_as_float(s[2]),
                                             __uint_as_float(s[3]));
                ref = kPLeaf | li;
            } else {
                flag(ctl, kOverflow);
            }
        }
    } else {
        const uint32_t hi = (*next_h)++;
        if (hi < o.cap_h) {
            o.haux[2 * (size_t)hi] = ci;
            o.haux[2 * (size_t)hi + 1] = skip_of(n);
            ref = hi;
        } else {
            flag(ctl, kOverflow);
        }
    }
    slot[3] = ref;
}

// HNode 0: the virtual node whose only slot is the root. Leaves the size of level 1 in ctl.
__global__ void hroot_kernel(const mirt_node* nd, int nn, int ns, const uint32_t* aos, double grow, HOut o, int* ctl)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t w[16];
    for (int k = 0; k < 16; k++) w[k] = (k & 3) == 3 ? kPNone : 0u;
    uint32_t next_h = 1, next_l = 0;
    if (nn > 0) {
        const uint32_t ci = live_node(nd, nn, ns, 0u);
        if (ci != kPNone) fill_slot(nd, ns, aos, grow, o, ci, &w[0], &next_h, &next_l, ctl);
    }
    for (int k = 0; k < 16; k++) o.hnodes[k] = w[k];
    o.haux[0] = 0xffffffffu;  // flat + 1 == 0: the whole tree
    o.haux[1] = (uint32_t)nn;
    ctl[kLvlInner] = (int)next_h - 1;
    ctl[kLvlLeaf] = (int)next_l;
}

// inner and leaf slots of each HNode of the level [hoff, hoff + cnt)
__global__ void hcount_kernel(const mirt_node* nd, int nn, int ns, const uint32_t* haux, uint32_t hoff, int cnt,
                              int* n_inner, int* n_leaf)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    uint32_t cut[4];
    const int m = hnode_cut(nd, nn, ns, haux[2 * ((size_t)hoff + j)], cut);
    int ni = 0, nl = 0;
    for (int k = 0; k < 4; k++)
        if (k < m) {
            const mirt_node n = nd[cut[k]];
            if (n.sphere < 0) ni++;
            else if (hitable(n, ns)) nl++;
        }
    n_inner[j] = ni;
    n_leaf[j] = nl;
}

// n_inner / n_leaf now hold the exclusive sums over the level: HNode hoff + j hands its inner slots the
// HNode indices from hoff + cnt + n_inner[j] on and its leaves the indices from leaf_base + n_leaf[j] on
__global__ void hfill_kernel(const mirt_node* nd, int nn, int ns, const uint32_t* aos, double grow, HOut o,
                             uint32_t hoff, int cnt, uint32_t leaf_base, const int* n_inner, const int* n_leaf,
                             const int* tsum, int tiles, int* ctl)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t h = hoff + (uint32_t)j;
    if (h >= o.cap_h) return;
    uint32_t cut[4];
    const int m = hnode_cut(nd, nn, ns, o.haux[2 * (size_t)h], cut);
    uint32_t next_h = hoff + (uint32_t)cnt + (uint32_t)scan_prefix(n_inner, tsum, j);
    uint32_t next_l = leaf_base + (uint32_t)scan_prefix(n_leaf, tsum + tiles, j);
    uint32_t w[16];
    for (int k = 0; k < 16; k++) w[k] = (k & 3) == 3 ? kPNone : 0u;
    for (int k = 0; k < 4; k++)
        if (k < m) fill_slot(nd, ns, aos, grow, o, cut[k], &w[4 * k], &next_h, &next_l, ctl);
    uint32_t* p = o.hnodes + 16 * (size_t)h;
    for (int k = 0; k < 16; k++) p[k] = w[k];
}

// ---- host side

// the arrays of a scene being made: freed unless the ctx took them
struct Pending {
    DeviceScene sc;
    bool taken = false;
    ~Pending()
    {
        if (taken) return;
        for (void* p : {sc.dnodes, sc.nodes32, sc.geo, sc.color, sc.pnodes, sc.hnodes, sc.haux, sc.leaves, sc.ndepth})
            if (p) (void)hipFree(p);
    }
};

}  // namespace

// The layouts of the `ns` 20-byte spheres at d_aos and the validated flat tree d_nodes[nn], both on the device,
// made by the kernels above on stream s and installed in the ctx (internal.h: refit_device.hip calls it too).
int mirt::layout_device(mirt_ctx* c, hipStream_t s, const uint32_t* d_aos, int ns, const mirt_node* d_nodes, int nn,
                        const char* fn)
{
    Pending out;
    DeviceScene& sc = out.sc;
    const size_t n1 = nn > 0 ? (size_t)nn : 1, ns1 = (size_t)ns + 1;
    HIP_TRY(hipMalloc(&sc.dnodes, sizeof(DNode) * n1));
    HIP_TRY(hipMalloc(&sc.nodes32, sizeof(mirt_node) * n1));
    HIP_TRY(hipMalloc(&sc.geo, sizeof(float4) * ns1));
    HIP_TRY(hipMalloc(&sc.color, sizeof(uint32_t) * ns1));
    HIP_TRY(hipMalloc(&sc.ndepth, n1));
    // scratch, one allocation: three flag arrays over the nodes (+ 1) and their tile sums, two count arrays
    // over an HNode level and theirs, the compacted leaves, the tested marks, the ctl words
    const int tiles = (int)(((size_t)nn + 1 + kTile - 1) / kTile);
    const size_t pad = (size_t)tiles * kTile;
    const size_t ints = 5 * pad + 5 * (size_t)tiles + n1 + kCtlWords;
    const size_t bytes = ints * 4 + ns1;
    DevMem scratch;
    HIP_TRY(hipMalloc(&scratch.p, bytes));
    int* flags = (int*)scratch.p;                 // is_inner, closes, is_live
    int* fsum = flags + 3 * pad;
    int* lvl = fsum + 3 * (size_t)tiles;          // n_inner, n_leaf of a level
    int* lsum = lvl + 2 * pad;
    int* compact = lsum + 2 * (size_t)tiles;
    int* ctl = compact + n1;
    uint8_t* tested = (uint8_t*)(ctl + kCtlWords);
    HIP_TRY(hipMemsetAsync(scratch.p, 0, bytes, s));
    HIP_TRY(hipMemsetAsync(sc.ndepth, 0, n1, s));
    if (nn > 0) HIP_TRY(hipMemcpyAsync(sc.nodes32, d_nodes, sizeof(mirt_node) * (size_t)nn, hipMemcpyDeviceToDevice, s));
    const unsigned gn = blocks((size_t)nn, kBlock);
    spheres_kernel<<<blocks(ns1, kBlock), kBlock, 0, s>>>(d_aos, ns, (float4*)sc.geo, (uint32_t*)sc.color, ctl);
    if (nn > 0) {
        nodes_kernel<<<gn, kBlock, 0, s>>>(d_nodes, nn, d_aos, ns, (uint32_t*)sc.dnodes, flags, flags + pad,
                                           flags + 2 * pad, tested, ctl);
        orphan_kernel<<<gn, kBlock, 0, s>>>(d_nodes, nn, ns, tested, ctl);
    }
    scan_tiles_kernel<<<dim3((unsigned)tiles, 3), kBlock, 0, s>>>(flags, pad, nn + 1, fsum, tiles);
    scan_sums_kernel<kSumBlock><<<3, kSumBlock, 0, s>>>(fsum, tiles, ctl + kTotInner);
    if (nn > 0) {
        depth_kernel<<<gn, kBlock, 0, s>>>(d_nodes, nn, ns, flags, flags + pad, flags + 2 * pad, fsum, tiles,
                                           (uint8_t*)sc.ndepth, compact, ctl);
        mono_kernel<<<gn, kBlock, 0, s>>>(compact, nn, ctl);
    }
    HIP_TRY(hipGetLastError());
    int h[kCtlWords];
    HIP_TRY(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int inner = h[kTotInner], nl = h[kTotLive];
    if (inner < 0 || inner > nn || nl < 0 || nl > nn) {
        set_error("%s: the layout kernels counted %d inner nodes and %d leaves among %d nodes", fn, inner, nl, nn);
        return MIRT_E_DEVICE;
    }
    // the scalars, as build_scene_layout forms them
    const bool nests = !h[kBadSphere] && !h[kBadNest];
    sc.r_max = nests ? bits_float(h[kRMax]) : 0.0f;
    sc.c_max = nests ? bits_float(h[kCMax]) : 0.0f;
    sc.encloses = nests && !h[kOrphan];
    const LayoutBound bound = layout_bound(sc.c_max, bits_float(h[kBoxMax]), sc.encloses);
    sc.o_bound = bound.o_bound;
    const double grow = bound.grow;
    sc.ordered = nn > 0 && !h[kNotMono] && h[kDepth] + 2 <= 64;
    sc.num_nodes = nn;
    sc.num_spheres = ns;
    sc.num_pnodes = 1u + (uint32_t)inner;
    sc.num_leaves = (uint32_t)nl;
    sc.leaf_box_off = (sizeof(Geo4) * (size_t)nl + 255) & ~(size_t)255;
    // an inner node is the slot of at most one HNode: 1 + inner bounds their number
    const uint32_t cap_h = sc.num_pnodes;
    HIP_TRY(hipMalloc(&sc.pnodes, sizeof(PNode) * (size_t)sc.num_pnodes));
    HIP_TRY(hipMalloc(&sc.hnodes, sizeof(HNode) * (size_t)cap_h));
    HIP_TRY(hipMalloc(&sc.haux, sizeof(HAux) * (size_t)cap_h));
    HIP_TRY(hipMalloc(&sc.leaves, sc.leaf_box_off + sizeof(LeafBox) * std::max<size_t>((size_t)nl, 1)));
    pnodes_kernel<<<blocks((size_t)nn + 1, kBlock), kBlock, 0, s>>>(d_nodes, nn, ns, flags, fsum, grow,
                                                                    (uint32_t*)sc.pnodes, sc.num_pnodes);
    HOut ho{(uint32_t*)sc.hnodes, (uint32_t*)sc.haux, (float4*)sc.leaves,
            (uint32_t*)((char*)sc.leaves + sc.leaf_box_off), cap_h, (uint32_t)nl};
    hroot_kernel<<<1, 64, 0, s>>>(d_nodes, nn, ns, d_aos, grow, ho, ctl);
    HIP_TRY(hipGetLastError());
    int lv[3];  // kLvlInner, kLvlLeaf, kOverflow
    HIP_TRY(hipMemcpyAsync(lv, ctl + kLvlInner, sizeof lv, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    sc.wide_root = lv[0] == 1 ? 1u : 0u;
    uint32_t hoff = 1, leaf_base = 0;
    while (true) {
        const int cnt = lv[0], leaves = lv[1];
        if (lv[2] || cnt < 0 || leaves < 0 || (size_t)hoff + (size_t)cnt > cap_h ||
            (size_t)leaf_base + (size_t)leaves > (size_t)nl) {
            set_error("%s: the four-wide layout outgrew its bounds (%u + %d of %u nodes, %u + %d of %d leaves)", fn,
                      hoff, cnt, cap_h, leaf_base, leaves, nl);
            return MIRT_E_DEVICE;
        }
        leaf_base += (uint32_t)leaves;
        if (cnt == 0) break;
        const unsigned gl = blocks((size_t)cnt, kBlock);
        const int ltiles = (int)(((size_t)cnt + kTile - 1) / kTile);
        hcount_kernel<<<gl, kBlock, 0, s>>>(d_nodes, nn, ns, (const uint32_t*)sc.haux, hoff, cnt, lvl, lvl + pad);
        scan_tiles_kernel<<<dim3((unsigned)ltiles, 2), kBlock, 0, s>>>(lvl, pad, cnt, lsum, ltiles);
        scan_sums_kernel<kSumBlock><<<2, kSumBlock, 0, s>>>(lsum, ltiles, ctl + kLvlInner);
        hfill_kernel<<<gl, kBlock, 0, s>>>(d_nodes, nn, ns, d_aos, grow, ho, hoff, cnt, leaf_base, lvl, lvl + pad, lsum,
                                           ltiles, ctl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(lv, ctl + kLvlInner, sizeof lv, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        hoff += (uint32_t)cnt;
    }
    if (leaf_base != (uint32_t)nl) {
        set_error("%s: the four-wide layout holds %u of %d leaves", fn, leaf_base, nl);
        return MIRT_E_DEVICE;
    }
    sc.num_hnodes = hoff;
    if (hoff < cap_h) {  // the ctx keeps arrays of the size an upload gives them, not of the bound
        void *hn = nullptr, *ha = nullptr;
        hipError_t e = hipMalloc(&hn, sizeof(HNode) * (size_t)hoff);
        if (e == hipSuccess) e = hipMalloc(&ha, sizeof(HAux) * (size_t)hoff);
        if (e == hipSuccess) e = hipMemcpyAsync(hn, sc.hnodes, sizeof(HNode) * (size_t)hoff, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(ha, sc.haux, sizeof(HAux) * (size_t)hoff, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            if (hn) (void)hipFree(hn);
            if (ha) (void)hipFree(ha);
            return hip_fail(e, fn);
        }
        (void)hipFree(sc.hnodes);
        (void)hipFree(sc.haux);
        sc.hnodes = hn;
        sc.haux = ha;
    }
    sc.leaf_big = sizeof(HNode) * (size_t)hoff + (sizeof(Geo4) + sizeof(LeafBox)) * (size_t)nl > ((size_t)32 << 20);
    if (int rc = ctx_install_scene(c, sc)) return rc;
    out.taken = true;
    return MIRT_OK;
}

extern "C" {

int mirt_scene_upload_flat_device(mirt_ctx* c, const mirt_sphere* spheres, int ns, const mirt_node* nodes, int nn)
{
    const char* fn = "mirt_scene_upload_flat_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (ns < 0 || nn < 0 || (ns > 0 && !spheres) || (nn > 0 && !nodes)) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    // a malformed tree must not send the kernels out of bounds
    if (int rc = validate_flat(nodes, nn, ns, 0, fn)) return rc;
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    DevMem aos, tree;
    HIP_TRY(hipMalloc(&aos.p, sizeof(mirt_sphere) * (size_t)std::max(ns, 1)));
    HIP_TRY(hipMalloc(&tree.p, sizeof(mirt_node) * (size_t)std::max(nn, 1)));
    if (ns > 0) HIP_TRY(hipMemcpyAsync(aos.p, spheres, sizeof(mirt_sphere) * (size_t)ns, hipMemcpyHostToDevice, s));
    if (nn > 0) HIP_TRY(hipMemcpyAsync(tree.p, nodes, sizeof(mirt_node) * (size_t)nn, hipMemcpyHostToDevice, s));
    const int rc = layout_device(c, s, (const uint32_t*)aos.p, ns, (const mirt_node*)tree.p, nn, fn);
    (void)hipStreamSynchronize(s);  // the caller's arrays and the scratch are free again
    return rc;
}

int mirt_scene_build_device(mirt_ctx* c, const mirt_sphere* spheres, int num_spheres, int start, int end, int depth,
                            mirt_sphere* reordered)
try {
    const char* fn = "mirt_scene_build_device";
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!spheres || num_spheres < 0 || start < 0 || end < start || end > num_spheres) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    mirt_scene_build_stats st{};
    ResidentTree tree{};
    int declined = 0;
    if (int rc = build_resident(c, spheres, num_spheres, start, end, depth, &tree, &declined)) return rc;
    if (declined) {
        // the host builder and the host upload, on a copy: the caller's array is not written
        std::vector<mirt_sphere> copy(spheres, spheres + num_spheres);
        mirt_node* nodes = nullptr;
        int nn = 0;
        if (int rc = mirt_bvh_build_flat(copy.data(), start, end, depth, &nodes, &nn)) return rc;
        const int rc = mirt_scene_upload_flat(c, copy.data(), num_spheres, nodes, nn);
        mirt_bvh_free_flat(nodes);
        if (rc) return rc;
        if (reordered && num_spheres > 0) std::memcpy(reordered, copy.data(), sizeof(mirt_sphere) * (size_t)num_spheres);
        st.nodes = nn;
    } else {
        HIP_TRY(hipStreamSynchronize(s));  // the build's last kernels: layout_ms starts behind them
        const auto t1 = std::chrono::steady_clock::now();
        int rc = layout_device(c, s, tree.aos, num_spheres, tree.nodes, tree.num_nodes, fn);
        if (!rc && reordered && num_spheres > 0)
            HIP_TRY(hipMemcpyAsync(reordered, tree.aos, sizeof(mirt_sphere) * (size_t)num_spheres,
                                   hipMemcpyDeviceToHost, s));
        const hipError_t e = hipStreamSynchronize(s);
        if (rc) return rc;
        if (e != hipSuccess) return hip_fail(e, fn);
        st.layout_ms = since(t1);
        st.on_device = 1;
        st.levels = tree.levels;
        st.nodes = tree.num_nodes;
        if ((rc = build_resident_ms(c, &st.build_ms))) return rc;
    }
    st.total_ms = since(t0);
    ctx_set_scene_stats(c, st);
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    set_error("mirt_scene_build_device: out of host memory");
    return MIRT_E_NOMEM;
}

}  // extern "C"

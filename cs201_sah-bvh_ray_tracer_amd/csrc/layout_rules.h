// The arithmetic and the per-node decisions of the device layouts (layout.h),
// each stated once for scene_layout.cpp (which numbers the nodes serially) and
// scene_device.hip (which numbers them by prefix sums): outward rounding, the
// nesting test, the four-slot cut of an HNode, a PNode child's box and
// reference, an HNode slot's packed box, and the scalar bound. Host and device,
// no HIP includes: a plain host compiler builds it, as it does layout.h. No
// contraction (-ffp-contract=off).
#pragma once
#include <algorithm>
#include <cstdint>

#include "layout.h"
#include "tree.h"

namespace mirt {

static_assert(kPNone == kNoNode, "live_node's `nothing below can hit` is the empty reference");

// nextafter(x, -inf) / nextafter(x, +inf) as integer steps
MIRT_HD inline float next_down(float x)
{
    const uint32_t b = float_bits(x);
    if (x != x || b == 0xff800000u) return x;
    if ((b & 0x7fffffffu) == 0u) return bits_float(0x80000001u);
    return bits_float((b & 0x80000000u) ? b + 1u : b - 1u);
}
MIRT_HD inline float next_up(float x)
{
    const uint32_t b = float_bits(x);
    if (x != x || b == 0x7f800000u) return x;
    if ((b & 0x7fffffffu) == 0u) return bits_float(0x00000001u);
    return bits_float((b & 0x80000000u) ? b - 1u : b + 1u);
}

// fp16 bits of the largest half <= v / the smallest half >= v (a value beyond
// the fp16 range rounds out to -inf / +inf: still a superset): the nearest
// half, then stepped to the right side. One step is ever needed; 4 bound it.
MIRT_HD inline uint32_t half_bits(float v) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v); }
MIRT_HD inline float half_value(uint32_t b) { return (float)__builtin_bit_cast(_Float16, (unsigned short)b); }
MIRT_HD inline uint32_t half_down(float v)
{
    uint32_t b = half_bits(v);
    for (int k = 0; k < 4 && half_value(b) > v; k++) b = b == 0x0000u ? 0x8001u : ((b & 0x8000u) ? b + 1u : b - 1u);
    return b & 0xffffu;
}
MIRT_HD inline uint32_t half_up(float v)
{
    uint32_t b = half_bits(v);
    for (int k = 0; k < 4 && half_value(b) < v; k++) b = b == 0x8000u ? 0x0001u : ((b & 0x8000u) ? b - 1u : b + 1u);
    return b & 0xffffu;
}

// a box face moved out by `grow`, rounded outward again: the float of lo - grow may lie above it
MIRT_HD inline float grown_lo(float lo, double grow) { return next_down((float)((double)lo - grow)); }
MIRT_HD inline float grown_hi(float hi, double grow) { return next_up((float)((double)hi + grow)); }

// the nesting test of tree_encloses: an empty leaf (+inf / -inf box, no sphere) nests anywhere
MIRT_HD inline bool holds(const mirt_node& outer, const mirt_node& inner)
{
    if (inner.skip & MIRT_NODE_EMPTY) return true;
    for (int k = 0; k < 3; k++)
        if (!(outer.bmin[k] <= inner.bmin[k] && outer.bmax[k] >= inner.bmax[k])) return false;
    return true;
}

// Slot k of a PNode for flat child c, whose live node is ci = live_node(c) and
// whose PNode index is pidx when ci is an inner node: the child's box into
// box[6] (lo.xyz, hi.xyz), the reference returned. grow > 0: an inner child's
// box grown by `grow` on each face (rounded outward): the camera packets'
// margin-free test (trace.h); leaf children keep their exact boxes, which gate
// every sphere.
MIRT_HD inline uint32_t pnode_child(const mirt_node* nd, int ns, double grow, uint32_t c, uint32_t ci, uint32_t pidx,
                                    float* box)
{
    const mirt_node& n = nd[ci == kPNone ? c : ci];  // nothing below can hit: an empty slot with c's own box
    for (int a = 0; a < 3; a++) {
        box[a] = n.bmin[a];
        box[3 + a] = n.bmax[a];
    }
    if (ci == kPNone || (n.skip & MIRT_NODE_EMPTY)) return kPNone;  // a 0-sphere leaf: passes, never hits
    if (n.sphere >= 0) return n.sphere >= ns || (uint32_t)n.sphere > kPIndex ? kPNone : (kPLeaf | (uint32_t)n.sphere);
    if (grow > 0.0 && pidx != kPNone)
        for (int a = 0; a < 3; a++) {
            box[a] = grown_lo(box[a], grow);
            box[3 + a] = grown_hi(box[3 + a], grow);
        }
    return pidx;
}

// The four slots of HNode(y): y's live children, then the inner slot with the
// largest box replaced by its two live children while a slot is free (every
// slot stays inside y's flat subtree, which HAux walks). Returns their number;
// the bounds are not reached for a validated tree.
MIRT_HD inline int hnode_cut(const mirt_node* nd, int nn, int ns, uint32_t y, uint32_t* cut)
{
    int m = 0;
    auto add = [&](uint32_t c) {
        const uint32_t ci = live_node(nd, nn, ns, c);
        if (ci != kPNone) cut[m++] = ci;
    };
    if (y + 1 >= (uint32_t)nn) return 0;
    add(y + 1);
    add(skip_of(nd[y + 1]));
    for (int step = 0; step < nn && m < 4; step++) {
        int best = -1;
        float best_area = -1.0f;
        for (int j = 0; j < m; j++) {
            const mirt_node& n = nd[cut[j]];
            if (n.sphere >= 0) continue;
            const float area = box_half_area(n.bmax[0] - n.bmin[0], n.bmax[1] - n.bmin[1], n.bmax[2] - n.bmin[2]);
            if (area > best_area || best < 0) {
                best = j;
                best_area = area;
            }
        }
        if (best < 0) break;
        const uint32_t c = cut[best];
        cut[best] = cut[--m];
        if (c + 1 >= (uint32_t)nn) break;
        add(c + 1);
        add(skip_of(nd[c + 1]));
    }
    return m;
}

// an HNode slot's box: grown by `grow` on each face when grow > 0 (the bounce walks' bounded slab test), then
// per axis fp16 lo (bits 0-15) | fp16 hi (bits 16-31), rounded outward
MIRT_HD inline void hnode_slot_box(const mirt_node& n, double grow, uint32_t* box)
{
    for (int a = 0; a < 3; a++) {
        float lo = n.bmin[a], hi = n.bmax[a];
        if (grow > 0.0) {
            lo = grown_lo(lo, grow);
            hi = grown_hi(hi, grow);
        }
        box[a] = half_down(lo) | (half_up(hi) << 16);
    }
}

// The margin-free box tests (bounce walks, camera packets): C bounds every box coordinate and every sphere point
// (so every bounce-ray origin, up to rounding: the margin 2^-10 C + 2^-10), and the slot boxes grow by 2^-19 C
// (trace.h slab_cons_fast<BND>). box_max: the largest finite |coordinate| of a non-empty node's box.
struct LayoutBound {
    double cb;      // C
    bool bounded;   // the boxes nest and the grown boxes stay finite in fp16
    float o_bound;  // C, or 0: every bounce ray takes the exact test
    double grow;    // 2^-19 C, or 0: nothing is grown
};
inline LayoutBound layout_bound(float c_max, float box_max, bool encloses)
{
    LayoutBound b;
    b.cb = std::max((double)c_max, (double)box_max) * (1.0 + 0x1p-10) + 0x1p-10;
    b.bounded = encloses && b.cb < 6.0e4;
    b.o_bound = b.bounded ? (float)b.cb : 0.0f;
    b.grow = b.bounded ? b.cb * 0x1p-19 : 0.0;
    return b;
}

}  // namespace mirt

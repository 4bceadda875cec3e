// The rules of the flat pre-order tree (mirt_node, include/mirt.h) and of its
// spheres, each stated once for the host builders (bvh_build.cpp, bvh_refit.cpp,
// bvh_quality.cpp, scene_layout.cpp) and the kernels that must give the host's
// bytes (bvh_device.hip, refit_device.hip, quality_device.hip,
// scene_device.hip). Host and device, no HIP includes: a plain host compiler
// builds it for the CPU tests and the sanitizer drivers. Every float expression
// below is contraction-sensitive: all users build with
// -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/mirt.h"

// (the walk headers take theirs, which carries `inline`, from rng.h: no file includes both families)
#if defined(__HIPCC__)
#define MIRT_HD __host__ __device__
#else
#define MIRT_HD
#endif

namespace mirt {

MIRT_HD inline uint32_t float_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}
MIRT_HD inline float bits_float(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// ---- nodes

MIRT_HD inline uint32_t skip_of(const mirt_node& n) { return n.skip & MIRT_SKIP_MASK; }

// A leaf that can hit: not a 0-sphere leaf, not the &spheres[N] sentinel.
MIRT_HD inline bool hitable(const mirt_node& n, int ns)
{
    return n.sphere >= 0 && !(n.skip & MIRT_NODE_EMPTY) && n.sphere < ns;
}

// A leaf the fast walks may drop: the &spheres[N] sentinel (never hits), or
// a 0-sphere leaf. hit.c:96-97 does test a 0-sphere leaf's sphere (its box,
// create_empty_aabb's, always passes): spheres[start] of its range when the
// SAH fallback split left it empty (mid == start: the first sphere of its
// sibling's range), spheres[end] when it split right (mid == end: a sphere
// of some LATER subtree). Dropping it is exact when that sphere is the
// tested sphere of a non-empty leaf (upload checks this, `orphan_phantoms`;
// otherwise only the reference-order DFS walk runs) and the ray reaches that
// leaf whenever it hits the sphere: the leaf's box holds the sphere's box
// fl(c -+ r) (checked, tree_encloses), the reference slab test is monotone
// under containment, so this rests on ONE assumption -- hit.c:49-82's
// division slab test passes the box fl(c -+ r) of every sphere that
// hit.c:19-39 reports hit. Both are exact-rounding computations of the same
// chord; tests/test_gpu_parity.py test_phantom_grazing_rays aims grazing rays
// at the spheres of both kinds of 0-sphere leaf and compares the fast walks
// with the DFS walk and the oracle.
MIRT_HD inline bool dead_leaf(const mirt_node& n, int ns) { return n.sphere >= 0 && !hitable(n, ns); }

constexpr uint32_t kNoNode = 0xffffffffu;  // live_node: nothing below can hit (layout.h's kPNone)

// The node a walk may take in place of flat node ci: an inner node one of
// whose children is dead adds nothing but its box test, which its live
// child's (nested, hence stricter) box test implies -- so the chains of
// one-sided splits the reference's SAH fallback builds (bvh.c:139-141,
// runs of nodes each with a 0-sphere leaf beside the rest of the range)
// collapse to the subtree that can hit. kNoNode: nothing below can hit.
// Every step moves to a later node, so nn steps bound it; a validated tree
// never reaches the bounds.
MIRT_HD inline uint32_t live_node(const mirt_node* nd, int nn, int ns, uint32_t ci)
{
    for (int step = 0; step < nn && ci < (uint32_t)nn; step++) {
        if (nd[ci].sphere >= 0) return dead_leaf(nd[ci], ns) ? kNoNode : ci;
        const uint32_t l = ci + 1;
        if (l >= (uint32_t)nn) break;
        const uint32_t r = skip_of(nd[l]);
        if (r >= (uint32_t)nn) break;
        const bool dl = dead_leaf(nd[l], ns), dr = dead_leaf(nd[r], ns);
        if (dl && dr) return kNoNode;
        if (!dl && !dr) return ci;
        ci = dl ? r : l;
    }
    return kNoNode;
}

// ---- boxes

struct Box {
    float lo[3], hi[3];
};

MIRT_HD inline Box box_empty()  // bvh.c:19-24
{
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = INFINITY;
        b.hi[a] = -INFINITY;
    }
    return b;
}

// the sphere's box fl(c -+ r) folded in (bvh.c:26-46)
MIRT_HD inline void box_add(Box& b, float cx, float cy, float cz, float r)
{
    const float c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fminf(b.lo[a], c[a] - r);
        b.hi[a] = fmaxf(b.hi[a], c[a] + r);
    }
}
MIRT_HD inline void box_add(Box& b, const mirt_sphere& s) { box_add(b, s.center.x, s.center.y, s.center.z, s.radius); }

MIRT_HD inline void box_merge(Box& b, const Box& o)
{
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fminf(b.lo[a], o.lo[a]);
        b.hi[a] = fmaxf(b.hi[a], o.hi[a]);
    }
}

MIRT_HD inline Box node_box(const mirt_node& n)
{
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = n.bmin[a];
        b.hi[a] = n.bmax[a];
    }
    return b;
}

MIRT_HD inline void store_box(mirt_node& n, const Box& b)
{
    for (int a = 0; a < 3; a++) {
        n.bmin[a] = b.lo[a];
        n.bmax[a] = b.hi[a];
    }
}

// bvh.c:48-57 from the three extents; the half is what the HNode cut compares (layout_rules.h)
MIRT_HD inline float box_half_area(float dx, float dy, float dz)
{
    float s = dx * dy;
    s = s + dy * dz;
    s = s + dz * dx;
    return s;
}
MIRT_HD inline float box_area(float dx, float dy, float dz) { return 2.0f * box_half_area(dx, dy, dz); }
MIRT_HD inline float box_area(const Box& b)
{
    return box_area(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]);
}
MIRT_HD inline float box_area(const mirt_node& n)
{
    return box_area(n.bmax[0] - n.bmin[0], n.bmax[1] - n.bmin[1], n.bmax[2] - n.bmin[2]);
}

// ---- the SAH split

// candidate plane i of 1..7 between lo and hi (bvh.c:150/154/158)
MIRT_HD inline float split_plane(float lo, float hi, int i) { return lo + ((float)i / 8.0f) * (hi - lo); }

// bvh.c:96 and the traversal constant: nl spheres in a box of area la, nr in one of area ra
MIRT_HD inline float sah_cost(int nl, float la, int nr, float ra)
{
    float sum = (float)nl * la;
    sum = sum + (float)nr * ra;
    return 0.125f + sum;
}

// ---- spheres

// A sphere (its centre's and its radius' float words) the kernels decline and
// the host takes instead: a NaN or an infinity, or a box coordinate fl(c -+ r)
// that is -0.0 -- fmin(-0, +0) depends on operand order, and the kernels
// combine in no fixed order -- or a negative radius: its box is inverted
// (c - r > c + r), the split planes of a node of such spheres decrease, and
// the kernels' bins assume that they increase (bvh_build.cpp has the direct
// form for that axis).
MIRT_HD inline bool sphere_declined(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t rad)
{
    const uint32_t w[4] = {cx, cy, cz, rad};
    bool bad = false;
    for (int k = 0; k < 4; k++) bad |= (w[k] & 0x7f800000u) == 0x7f800000u;
    const float r = bits_float(rad);
    bad |= r < 0.0f;
    for (int a = 0; a < 3; a++) {
        const float c = bits_float(w[a]);
        bad |= float_bits(c - r) == 0x80000000u || float_bits(c + r) == 0x80000000u;
    }
    return bad;
}

}  // namespace mirt

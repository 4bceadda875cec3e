// The device layouts of a scene (layout.h), built on the host from the
// caller's spheres and validated flat tree: what mirt_scene_upload_flat sends
// to the device, and what mirt_scene_layout returns to a test. Pure host C++:
// these builders decide whether every fast walk is exact, so they are kept
// where the CPU tests and the sanitizer driver (tests/c/san_host.cpp) reach.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "internal.h"
#include "layout.h"

using namespace mirt;

namespace {

// The pruning bound (trace.h Prune) holds for a tree in which every leaf box
// holds its sphere's box as bvh.c:26-46 computes it, fl(c -+ r), and every
// inner box holds both children's boxes; the reference's own trees are built
// that way. Also returns the scene constants of the bound. A NaN anywhere,
// a non-finite sphere or a tree that does not nest turns pruning off.
// A 0-sphere leaf whose sphere (hit.c:96-97 tests it) is no non-empty leaf's
// tested sphere: a tree built over part of an array (benchmark.c:317 builds
// over [0, n - 1)) whose SAH fallback left a last leaf empty points at the
// element after the range, which only that leaf tests. The pruned and
// ordered walks drop 0-sphere leaves (dead_leaf), so such a tree is walked
// in the reference's DFS order instead.
bool orphan_phantoms(const mirt_node* nd, int nn, int ns)
{
    std::vector<char> tested((size_t)ns + 1, 0);
    for (int i = 0; i < nn; i++)
        if (nd[i].sphere >= 0 && nd[i].sphere < ns && !(nd[i].skip & MIRT_NODE_EMPTY)) tested[nd[i].sphere] = 1;
    for (int i = 0; i < nn; i++)
        if (nd[i].sphere >= 0 && nd[i].sphere < ns && (nd[i].skip & MIRT_NODE_EMPTY) && !tested[nd[i].sphere])
            return true;
    return false;
}

bool tree_encloses(const mirt_sphere* sp, int ns, const mirt_node* nd, int nn, float* r_max, float* c_max)
{
    float rm = 0.0f, cm = 0.0f;
    for (int i = 0; i < ns; i++) {
        const float c[3] = {sp[i].center.x, sp[i].center.y, sp[i].center.z};
        const float r = std::fabs(sp[i].radius);
        if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]) || !std::isfinite(r)) return false;
        rm = std::max(rm, r);
        cm = std::max(cm, std::max(std::fabs(c[0]), std::max(std::fabs(c[1]), std::fabs(c[2]))) + r);
    }
    auto holds = [](const mirt_node& outer, const mirt_node& inner) {
        if (inner.skip & MIRT_NODE_EMPTY) return true;  // +inf/-inf box, no sphere
        for (int k = 0; k < 3; k++)
            if (!(outer.bmin[k] <= inner.bmin[k] && outer.bmax[k] >= inner.bmax[k])) return false;
        return true;
    };
    for (int i = 0; i < nn; i++) {
        const mirt_node& n = nd[i];
        if (n.skip & MIRT_NODE_EMPTY) continue;
        if (n.sphere >= 0) {
            if (n.sphere >= ns) continue;  // the never-hit sentinel
            const mirt_sphere& s = sp[n.sphere];
            const float c[3] = {s.center.x, s.center.y, s.center.z};
            const float r = std::fabs(s.radius);
            for (int k = 0; k < 3; k++)
                if (!(n.bmin[k] <= c[k] - r && n.bmax[k] >= c[k] + r)) return false;
        } else {
            const uint32_t left = (uint32_t)i + 1, right = nd[left].skip & MIRT_SKIP_MASK;
            if (!holds(n, nd[left]) || (right < (uint32_t)nn && right < (n.skip & MIRT_SKIP_MASK) && !holds(n, nd[right])))
                return false;
        }
    }
    *r_max = rm;
    *c_max = cm;
    return true;
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
bool dead_leaf(const mirt_node* nd, uint32_t i, int ns)
{
    return nd[i].sphere >= 0 && ((nd[i].skip & MIRT_NODE_EMPTY) || nd[i].sphere >= ns);
}

// The node a walk may take in place of flat node ci: an inner node one of
// whose children is dead adds nothing but its box test, which its live
// child's (nested, hence stricter) box test implies -- so the chains of
// one-sided splits the reference's SAH fallback builds (bvh.c:139-141,
// runs of nodes each with a 0-sphere leaf beside the rest of the range)
// collapse to the subtree that can hit. kPNone: nothing below can hit.
uint32_t live_node(const mirt_node* nd, uint32_t ci, int ns)
{
    for (;;) {
        if (nd[ci].sphere >= 0) return dead_leaf(nd, ci, ns) ? kPNone : ci;
        const uint32_t l = ci + 1, r = nd[ci + 1].skip & MIRT_SKIP_MASK;
        const bool dl = dead_leaf(nd, l, ns), dr = dead_leaf(nd, r, ns);
        if (dl && dr) return kPNone;
        if (!dl && !dr) return ci;
        ci = dl ? r : l;
    }
}

// PNode layout (layout.h) of a validated flat tree. Returns whether ordered
// walks may use it: hit-able leaves must carry strictly increasing sphere
// indices in DFS order (then the index is hit.c:108's tie key -- true of the
// reference's trees, whose build partitions the array in place) and the
// inner depth must leave the packet walk's stack (one entry per level)
// within 64.
// grow > 0: an inner child's box grown by `grow` on each face (rounded
// outward): the camera packets' margin-free test (trace.h); leaf children keep
// their exact boxes, which gate every sphere.
bool build_pnodes(const mirt_node* nd, int nn, const mirt_sphere* sp, int ns, std::vector<PNode>& pn, double grow)
{
    std::vector<uint32_t> pidx((size_t)nn, kPNone);
    uint32_t np = 1;
    for (int i = 0; i < nn; i++)
        if (nd[i].sphere < 0) pidx[i] = np++;
    pn.assign(np, PNode{});
    auto set_child = [&](PNode& p, int k, uint32_t c) {
        const uint32_t ci = live_node(nd, c, ns);
        if (ci == kPNone) {  // nothing below can hit: an empty slot
            float* slot = k ? p.c1 : p.c0;
            std::memcpy(slot, nd[c].bmin, sizeof nd[c].bmin);
            std::memcpy(slot + 3, nd[c].bmax, sizeof nd[c].bmax);
            (k ? p.ref1 : p.ref0) = kPNone;
            return;
        }
        const mirt_node& n = nd[ci];
        float* slot = k ? p.c1 : p.c0;
        uint32_t ref = pidx[ci];
        std::memcpy(slot, n.bmin, sizeof n.bmin);
        std::memcpy(slot + 3, n.bmax, sizeof n.bmax);
        if (n.skip & MIRT_NODE_EMPTY) {
            ref = kPNone;  // a 0-sphere leaf: passes, never hits
        } else if (n.sphere >= 0) {
            if (n.sphere >= ns || (uint32_t)n.sphere > kPIndex) {
                ref = kPNone;
            } else {
                ref = kPLeaf | (uint32_t)n.sphere;
            }
        }
        if (grow > 0.0 && ref != kPNone && !(ref & kPLeaf))
            for (int a = 0; a < 3; a++) {
                slot[a] = std::nextafter((float)((double)slot[a] - grow), -INFINITY);
                slot[3 + a] = std::nextafter((float)((double)slot[3 + a] + grow), INFINITY);
            }
        (k ? p.ref1 : p.ref0) = ref;
    };
    pn[0].ref0 = pn[0].ref1 = kPNone;
    pn[0].flat = 0xffffffffu;  // flat + 1 == 0: the whole tree
    pn[0].end = (uint32_t)nn;
    if (nn > 0) set_child(pn[0], 0, 0);
    bool mono = nn > 0;
    int last = -1;
    std::vector<uint32_t> ends;  // subtree ends of the open inner nodes
    size_t depth = 0;
    for (int i = 0; i < nn; i++) {
        while (!ends.empty() && ends.back() <= (uint32_t)i) ends.pop_back();
        if (nd[i].sphere < 0) {
            PNode& p = pn[pidx[i]];
            set_child(p, 0, (uint32_t)i + 1);
            set_child(p, 1, nd[i + 1].skip & MIRT_SKIP_MASK);
            p.flat = (uint32_t)i;
            p.end = nd[i].skip & MIRT_SKIP_MASK;
            ends.push_back(nd[i].skip & MIRT_SKIP_MASK);
            depth = std::max(depth, ends.size());
        } else if (!(nd[i].skip & MIRT_NODE_EMPTY) && nd[i].sphere < ns) {
            if (nd[i].sphere <= last) mono = false;
            last = nd[i].sphere;
        }
    }
    return mono && depth + 2 <= 64;
}

// fp16 bits of the largest half <= v / the smallest half >= v (a value
// beyond the fp16 range rounds out to -inf / +inf: still a superset).
uint16_t half_bits(float v)
{
    const _Float16 h = (_Float16)v;
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}
float half_value(uint16_t b)
{
    _Float16 h;
    std::memcpy(&h, &b, 2);
    return (float)h;
}
uint16_t half_down(float v)
{
    uint16_t b = half_bits(v);
    while (half_value(b) > v) b = b == 0x0000 ? 0x8001 : (b & 0x8000) ? b + 1 : b - 1;
    return b;
}
uint16_t half_up(float v)
{
    uint16_t b = half_bits(v);
    while (half_value(b) < v) b = b == 0x8000 ? 0x0001 : (b & 0x8000) ? b - 1 : b + 1;
    return b;
}

// HNode layout (layout.h) of a validated flat tree: HNode 0 holds the root;
// an HNode for each inner node that is some HNode's slot holds that node's
// grandchildren (a leaf child standing in for its own); one leaf (sphere +
// exact box) per leaf slot. Used only when the PNode conditions hold and the boxes nest.
// grow > 0 (the bounce walks' bounded slab test): every slot box grown by `grow` on each face
// before the outward fp16 rounding.
void build_hnodes(const mirt_node* nd, int nn, const mirt_sphere* sp, int ns, std::vector<HNode>& hn,
                  std::vector<HAux>& aux, std::vector<Geo4>& lgeo, std::vector<LeafBox>& lbox, double grow)
{
    hn.assign(1, HNode{});
    aux.assign(1, HAux{0xffffffffu, (uint32_t)nn});  // flat + 1 == 0: the whole tree
    lgeo.clear();
    lbox.clear();
    std::vector<uint32_t> todo;  // inner nodes waiting for their HNode: HNode 1 + i is todo[i]
    auto fill = [&](size_t hi, int k, uint32_t c) {
        HNode& h = hn[hi];
        const uint32_t ci = live_node(nd, c, ns);
        if (ci == kPNone) {
            h.slot[k].ref = kPNone;
            return;
        }
        const mirt_node& n = nd[ci];
        for (int a = 0; a < 3; a++) {
            float lo = n.bmin[a], hi = n.bmax[a];
            if (grow > 0.0) {   // rounded outward again: the float of lo - grow may lie above it
                lo = std::nextafter((float)((double)lo - grow), -INFINITY);
                hi = std::nextafter((float)((double)hi + grow), INFINITY);
            }
            h.slot[k].box[a] = (uint32_t)half_down(lo) | ((uint32_t)half_up(hi) << 16);
        }
        uint32_t ref;
        if (n.skip & MIRT_NODE_EMPTY) {
            ref = kPNone;
        } else if (n.sphere >= 0) {
            if (n.sphere >= ns) {
                ref = kPNone;
            } else {
                LeafBox l{};
                std::memcpy(l.lo, n.bmin, sizeof l.lo);
                std::memcpy(l.hi, n.bmax, sizeof l.hi);
                l.sphere = n.sphere;
                const mirt_sphere& s = sp[n.sphere];
                ref = kPLeaf | (uint32_t)lbox.size();
                lbox.push_back(l);
                lgeo.push_back(Geo4{s.center.x, s.center.y, s.center.z, s.radius});
            }
        } else {
            todo.push_back(ci);
            ref = (uint32_t)todo.size();
        }
        h.slot[k].ref = ref;
    };
    for (int k = 0; k < 4; k++) hn[0].slot[k].ref = kPNone;
    if (nn == 0) return;
    fill(0, 0, 0);
    for (size_t next = 0; next < todo.size(); next++) {
        const uint32_t y = todo[next];
        HNode h{};
        for (int k = 0; k < 4; k++) h.slot[k].ref = kPNone;
        hn.push_back(h);
        aux.push_back(HAux{y, nd[y].skip & MIRT_SKIP_MASK});
        // the four slots: y's live children, then the inner slot with the
        // largest box replaced by its two live children while a slot is
        // free (every slot stays inside y's flat subtree, which HAux walks)
        uint32_t cut[4];
        int m = 0;
        auto add = [&](uint32_t c) {
            const uint32_t ci = live_node(nd, c, ns);
            if (ci != kPNone) cut[m++] = ci;
        };
        add(y + 1);
        add(nd[y + 1].skip & MIRT_SKIP_MASK);
        while (m < 4) {
            int best = -1;
            float best_area = -1.0f;
            for (int j = 0; j < m; j++) {
                const mirt_node& n = nd[cut[j]];
                if (n.sphere >= 0) continue;
                const float dx = n.bmax[0] - n.bmin[0], dy = n.bmax[1] - n.bmin[1], dz = n.bmax[2] - n.bmin[2];
                const float area = dx * dy + dy * dz + dz * dx;
                if (area > best_area || best < 0) {
                    best = j;
                    best_area = area;
                }
            }
            if (best < 0) break;
            const uint32_t c = cut[best];
            cut[best] = cut[--m];
            add(c + 1);
            add(nd[c + 1].skip & MIRT_SKIP_MASK);
        }
        for (int k = 0; k < m; k++) fill(hn.size() - 1, k, cut[k]);
    }
}

}  // namespace

namespace mirt {

void build_scene_layout(const mirt_sphere* spheres, int ns, const mirt_node* nodes, int nn, SceneLayout& out)
{
    out.r_max = out.c_max = 0.0f;
    out.encloses = tree_encloses(spheres, ns, nodes, nn, &out.r_max, &out.c_max) && !orphan_phantoms(nodes, nn, ns);
    std::vector<Geo4>& geo = out.geo;
    geo.resize((size_t)ns + 1);
    out.color.resize((size_t)ns + 1);
    for (int i = 0; i < ns; i++) {
        geo[i] = Geo4{spheres[i].center.x, spheres[i].center.y, spheres[i].center.z, spheres[i].radius};
        std::memcpy(&out.color[i], &spheres[i].color, 4);
    }
    geo[ns] = Geo4{NAN, NAN, NAN, NAN};  // &spheres[N] sentinel: never hits
    out.color[ns] = 0xff000000u;
    // device layout: 64-B nodes with each leaf's sphere inline (layout.h DNode)
    out.dnodes.resize((size_t)nn);
    for (int i = 0; i < nn; i++) {
        DNode& d = out.dnodes[i];
        std::memset(&d, 0, sizeof d);
        std::memcpy(d.bmin, nodes[i].bmin, sizeof d.bmin);
        std::memcpy(d.bmax, nodes[i].bmax, sizeof d.bmax);
        d.sphere = nodes[i].sphere;
        d.skip = nodes[i].skip;
        std::memcpy(&d.geo, &geo[nodes[i].sphere >= 0 ? nodes[i].sphere : ns], sizeof d.geo);  // float4 under HIP
    }
    // the margin-free box tests (bounce walks, camera packets): C bounds every box coordinate and every sphere point
    // (so every bounce-ray origin, up to rounding: the margin 2^-10 C + 2^-10),
    // and the slot boxes grow by 2^-19 C (trace.h slab_cons_fast<BND>)
    double cb = out.c_max;
    for (int i = 0; i < nn; i++) {
        if (nodes[i].skip & MIRT_NODE_EMPTY) continue;
        for (int a = 0; a < 3; a++)
            for (float v : {nodes[i].bmin[a], nodes[i].bmax[a]})
                if (std::isfinite(v)) cb = std::max(cb, (double)std::fabs(v));
    }
    cb = cb * (1.0 + 0x1p-10) + 0x1p-10;
    const bool bounded = out.encloses && cb < 6.0e4;   // fp16 range: the grown boxes stay finite
    out.o_bound = bounded ? (float)cb : 0.0f;   // 0: every bounce ray takes the exact test
    out.ordered = build_pnodes(nodes, nn, spheres, ns, out.pnodes, bounded ? cb * 0x1p-19 : 0.0);
    build_hnodes(nodes, nn, spheres, ns, out.hnodes, out.haux, out.leaf_geo, out.leaf_box,
                 bounded ? cb * 0x1p-19 : 0.0);
    const size_t nl = out.leaf_box.size();
    out.leaf_box_off = (sizeof(Geo4) * nl + 255) & ~(size_t)255;
    // node depths (pre-order: the children of inner node i are i + 1 and the
    // left subtree's skip), clamped to 255 -- the overlay's colour key
    std::vector<uint8_t>& ndepth = out.ndepth;
    ndepth.assign((size_t)std::max(nn, 1), 0);
    for (int i = 0; i < nn; i++) {
        if (nodes[i].sphere >= 0) continue;
        const uint8_t d = ndepth[i] == 255 ? 255 : (uint8_t)(ndepth[i] + 1);
        ndepth[i + 1] = d;
        ndepth[nodes[i + 1].skip & MIRT_SKIP_MASK] = d;
    }
    out.leaf_big = sizeof(HNode) * out.hnodes.size() + (sizeof(Geo4) + sizeof(LeafBox)) * nl > ((size_t)32 << 20);
    {
        const uint32_t r = out.hnodes[0].slot[0].ref;
        out.wide_root = (r != kPNone && !(r & kPLeaf)) ? r : 0u;
    }
}

}  // namespace mirt

extern "C" int64_t mirt_scene_layout(const mirt_sphere* spheres, int ns, const mirt_node* nodes, int nn, int part,
                                     void* out, size_t cap, mirt_scene_layout_info* info)
try {
    if (ns < 0 || nn < 0 || (ns > 0 && !spheres) || (nn > 0 && !nodes)) {
        set_error("mirt_scene_layout: invalid arguments");
        return MIRT_E_INVALID;
    }
    if (int rc = validate_flat(nodes, nn, ns, 0, "mirt_scene_layout")) return rc;
    SceneLayout lay;
    build_scene_layout(spheres, ns, nodes, nn, lay);
    const void* src = nullptr;
    size_t bytes = 0;
    auto part_of = [&](const auto& v) {
        src = v.data();
        bytes = sizeof v[0] * v.size();
    };
    switch (part) {
    case MIRT_LAYOUT_DNODES: part_of(lay.dnodes); break;
    case MIRT_LAYOUT_GEO: part_of(lay.geo); break;
    case MIRT_LAYOUT_COLOR: part_of(lay.color); break;
    case MIRT_LAYOUT_PNODES: part_of(lay.pnodes); break;
    case MIRT_LAYOUT_HNODES: part_of(lay.hnodes); break;
    case MIRT_LAYOUT_HAUX: part_of(lay.haux); break;
    case MIRT_LAYOUT_LEAF_GEO: part_of(lay.leaf_geo); break;
    case MIRT_LAYOUT_LEAF_BOX: part_of(lay.leaf_box); break;
    case MIRT_LAYOUT_NDEPTH: part_of(lay.ndepth); break;
    default: set_error("mirt_scene_layout: unknown part %d", part); return MIRT_E_INVALID;
    }
    if (info) {
        info->encloses = lay.encloses;
        info->ordered = lay.ordered;
        info->leaf_big = lay.leaf_big;
        info->r_max = lay.r_max;
        info->c_max = lay.c_max;
        info->o_bound = lay.o_bound;
        info->num_pnodes = (uint32_t)lay.pnodes.size();
        info->num_hnodes = (uint32_t)lay.hnodes.size();
        info->num_leaves = (uint32_t)lay.leaf_box.size();
        info->wide_root = lay.wide_root;
        info->leaf_box_off = lay.leaf_box_off;
    }
    if (out && cap >= bytes && bytes) std::memcpy(out, src, bytes);
    return (int64_t)bytes;
} catch (const std::bad_alloc&) {
    set_error("mirt_scene_layout: out of host memory");
    return MIRT_E_NOMEM;
}

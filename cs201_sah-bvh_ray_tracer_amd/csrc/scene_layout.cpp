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
#include "layout_rules.h"

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
        if (hitable(nd[i], ns)) tested[nd[i].sphere] = 1;
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
            const uint32_t left = (uint32_t)i + 1, right = skip_of(nd[left]);
            if (!holds(n, nd[left]) || (right < (uint32_t)nn && right < skip_of(n) && !holds(n, nd[right])))
                return false;
        }
    }
    *r_max = rm;
    *c_max = cm;
    return true;
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
        const uint32_t ci = live_node(nd, nn, ns, c);
        (k ? p.ref1 : p.ref0) = pnode_child(nd, ns, grow, c, ci, ci == kPNone ? kPNone : pidx[ci], k ? p.c1 : p.c0);
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
            set_child(p, 1, skip_of(nd[i + 1]));
            p.flat = (uint32_t)i;
            p.end = skip_of(nd[i]);
            ends.push_back(skip_of(nd[i]));
            depth = std::max(depth, ends.size());
        } else if (hitable(nd[i], ns)) {
            if (nd[i].sphere <= last) mono = false;
            last = nd[i].sphere;
        }
    }
    return mono && depth + 2 <= 64;
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
    // a slot's reference is numbered as slots are filled (scene_device.hip's fill_slot takes its numbers from
    // prefix sums and guards its arrays' capacity): the two numberings stay apart
    auto fill = [&](size_t hi, int k, uint32_t c) {
        HNode& h = hn[hi];
        const uint32_t ci = live_node(nd, nn, ns, c);
        if (ci == kPNone) {
            h.slot[k].ref = kPNone;
            return;
        }
        const mirt_node& n = nd[ci];
        hnode_slot_box(n, grow, h.slot[k].box);
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
        aux.push_back(HAux{y, skip_of(nd[y])});
        uint32_t cut[4];
        const int m = hnode_cut(nd, nn, ns, y, cut);
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
    float box_max = 0.0f;  // the largest finite |coordinate| of a non-empty node's box
    for (int i = 0; i < nn; i++) {
        if (nodes[i].skip & MIRT_NODE_EMPTY) continue;
        for (int a = 0; a < 3; a++)
            for (float v : {nodes[i].bmin[a], nodes[i].bmax[a]})
                if (std::isfinite(v)) box_max = std::max(box_max, std::fabs(v));
    }
    const LayoutBound bound = layout_bound(out.c_max, box_max, out.encloses);
    out.o_bound = bound.o_bound;
    out.ordered = build_pnodes(nodes, nn, spheres, ns, out.pnodes, bound.grow);
    build_hnodes(nodes, nn, spheres, ns, out.hnodes, out.haux, out.leaf_geo, out.leaf_box, bound.grow);
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

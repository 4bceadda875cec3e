// The device layouts of a scene and the host-side record that holds them
// (scene_layout.cpp builds it, mirt_scene_upload_flat copies it to the device,
// trace.h walks it; scene_device.hip derives the same bytes by kernels). No
// HIP in here: a plain host compiler builds this header and scene_layout.cpp
// for the CPU tests and the sanitizer driver.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIP__
#include <hip/hip_vector_types.h>
#endif

#include "../../include/mirt.h"

namespace mirt {

// A sphere as the kernels load it (centre.xyz, radius): the host's stand-in
// for float4, same size, alignment and field order.
struct alignas(16) Geo4 {
    float x, y, z, w;
};
static_assert(sizeof(Geo4) == 16 && alignof(Geo4) == 16, "a sphere is one 16-B load");
static_assert(offsetof(Geo4, x) == 0 && offsetof(Geo4, y) == 4 && offsetof(Geo4, z) == 8 && offsetof(Geo4, w) == 12,
              "Geo4 is float4's layout");
#ifdef __HIP__
static_assert(sizeof(float4) == sizeof(Geo4) && alignof(float4) == alignof(Geo4), "Geo4 is float4's layout");
#endif

// Device copy of a flattened node (mirt_node, include/mirt.h) padded to 64 B,
// with the leaf's sphere (centre, radius) inline so a leaf step needs no
// second, dependent load. Inner nodes and the &spheres[N] sentinel carry NaN
// geometry (never hits).
struct __attribute__((aligned(64))) DNode {
    float bmin[3];
    float bmax[3];
    int32_t sphere;   // leaf: sphere index; inner: -1
    uint32_t skip;    // next node after this subtree | MIRT_NODE_EMPTY
#ifdef __HIP__
    float4 geo;       // leaf sphere centre.xyz, radius
#else
    Geo4 geo;         // (a HIP translation unit sees float4: the same 16 bytes, pinned above)
#endif
    uint32_t pad[4];
};
static_assert(sizeof(DNode) == 64, "device node is 64 B");
static_assert(alignof(DNode) == 64 && offsetof(DNode, bmin) == 0 && offsetof(DNode, bmax) == 12 &&
                  offsetof(DNode, sphere) == 24 && offsetof(DNode, skip) == 28 && offsetof(DNode, geo) == 32 &&
                  offsetof(DNode, pad) == 48,
              "device node fields");

// The same tree re-laid for ordered walks: one node per inner node of the
// reference tree holding BOTH children, so one load tests both and the walk
// can enter the nearer child first. PNode 0 is a virtual parent whose only
// child is the root. A child reference is an inner PNode index, kPLeaf |
// sphere index (a leaf that can hit), or kPNone (no child that can ever hit:
// a 0-sphere leaf or the &spheres[N] sentinel of hit.c). A child slot holds
// the child's box (lo.xyz, hi.xyz) -- for a leaf that is the box of the
// node's whole sphere range, not of its one sphere (a depth-40 leaf keeps
// the range's bounds but tests only node->sphere, bvh.c:122-136), so the
// sphere itself is fetched when the box passes.
// `flat` and `end` locate the node in the flat pre-order tree, [flat + 1,
// end) being its children's subtrees, which a walk can take in DFS order
// without a stack.
constexpr uint32_t kPLeaf = 0x80000000u;
constexpr uint32_t kPNone = 0xffffffffu;
constexpr uint32_t kPIndex = 0x7fffffffu;
struct __attribute__((aligned(64))) PNode {
    float c0[6];
    float c1[6];
    uint32_t ref0, ref1;
    uint32_t flat, end;
};
static_assert(sizeof(PNode) == 64, "ordered node is 64 B");
static_assert(alignof(PNode) == 64 && offsetof(PNode, c0) == 0 && offsetof(PNode, c1) == 24 &&
                  offsetof(PNode, ref0) == 48 && offsetof(PNode, ref1) == 52 && offsetof(PNode, flat) == 56 &&
                  offsetof(PNode, end) == 60,
              "ordered node fields");

// Four-wide layout for per-lane walks: HNode(Y), for an inner node Y of the
// reference tree, holds Y's grandchildren (a child that is a leaf stands in
// for its own slot), so a walk takes half the dependent steps. The skipped
// children's boxes need no test: the tree's boxes nest (checked at upload)
// and hit.c's slab test is monotone under containment (correctly rounded
// subtraction and division are monotone, so a box inside another gets a
// later entry and an earlier exit), so a ray that passes a box passes every
// enclosing one -- the leaves reached are exactly those hit.c:91-109
// reaches. The same argument lets slot boxes be CONSERVATIVE: each is
// stored in fp16 rounded outward (a superset) and tested with a fast test
// that passes when undecided -- entering an inner node too eagerly costs
// work, never a result, because every leaf is still gated by its exact box.
// A leaf slot's sphere and its exact box live in two arrays (structure of
// arrays, round 6): the gate reads the 16-B sphere first and the 32-B box only
// for a hit that could win, so the spheres the walks read are packed eight to
// a 128-B line (a 48-B record per leaf held 2.7) and the hot part of a large
// tree -- HNodes + spheres -- is two thirds of the bytes it was. 64 B per node = the bytes of two fp32 boxes: divergent
// per-lane loads are bound by the bytes the texture path returns.
// HNode 0 is a virtual node whose only slot is the root; slot references: an
// inner HNode index, kPLeaf | leaf index, or kPNone. HAux holds the
// node's flat DFS segment [flat + 1, end), read only when the stack is full.
struct __attribute__((aligned(64))) HNode {
    struct Slot {
        uint32_t box[3];  // per axis: fp16 lo (bits 0-15) | fp16 hi (bits 16-31)
        uint32_t ref;
    } slot[4];            // 16 B per slot: one dwordx4 each
};
static_assert(sizeof(HNode) == 64, "wide node is 64 B");
static_assert(alignof(HNode) == 64 && sizeof(HNode::Slot) == 16 && offsetof(HNode::Slot, box) == 0 &&
                  offsetof(HNode::Slot, ref) == 12 && offsetof(HNode, slot) == 0,
              "wide node fields");
struct HAux {
    uint32_t flat, end;
};
static_assert(sizeof(HAux) == 8 && alignof(HAux) == 4 && offsetof(HAux, flat) == 0 && offsetof(HAux, end) == 4,
              "wide node segment fields");
struct __attribute__((aligned(32))) LeafBox {
    float lo[3], hi[3];  // the leaf's exact box (bvh.c bounds)
    int32_t sphere;
    uint32_t pad;
};
static_assert(sizeof(LeafBox) == 32, "leaf box is 32 B");
static_assert(alignof(LeafBox) == 32 && offsetof(LeafBox, lo) == 0 && offsetof(LeafBox, hi) == 12 &&
                  offsetof(LeafBox, sphere) == 24 && offsetof(LeafBox, pad) == 28,
              "leaf box fields");

// Everything mirt_scene_upload_flat sends to the device for one scene, built
// on the host by build_scene_layout (scene_layout.cpp).
struct SceneLayout {
    std::vector<DNode> dnodes;       // one per flat node
    std::vector<Geo4> geo;           // ns + 1, NaN sentinel last
    std::vector<uint32_t> color;     // ns + 1, 0xff000000 last
    std::vector<PNode> pnodes;
    std::vector<HNode> hnodes;
    std::vector<HAux> haux;          // one per HNode
    std::vector<Geo4> leaf_geo;      // one per four-wide leaf: its sphere
    std::vector<LeafBox> leaf_box;   // one per four-wide leaf: its exact box
    std::vector<uint8_t> ndepth;     // max(nn, 1) node depths, clamped to 255
    bool encloses = false;           // the boxes nest and no phantom is orphaned: pruning allowed
    bool ordered = false;            // ordered walks allowed (build_pnodes)
    float r_max = 0.0f;              // largest sphere radius
    float c_max = 0.0f;              // largest |centre|_inf + radius
    float o_bound = 0.0f;            // |coordinate| bound C the slot boxes were grown for (0: not grown)
    size_t leaf_box_off = 0;         // byte offset of leaf_box behind leaf_geo in the device array
    uint32_t wide_root = 0;          // the root's HNode, 0 for a leaf root
    bool leaf_big = false;           // the four-wide layout is larger than the chip's L2
};

// The layouts of a tree that has passed validate_flat (internal.h); nn == 0:
// no tree. May throw std::bad_alloc.
void build_scene_layout(const mirt_sphere* spheres, int ns, const mirt_node* nodes, int nn, SceneLayout& out);

}  // namespace mirt

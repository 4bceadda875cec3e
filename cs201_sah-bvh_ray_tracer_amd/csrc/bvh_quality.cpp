// The SAH quality of a flat pre-order tree (mirt_bvh_quality_flat): the host
// statement of the definition quality_device.hip's kernel implements on the
// resident tree (quality.h has the shared operations, DESIGN.md 9.3 the why).
//
//   overhead  sum of area(inner nodes) / sum of area(hit-able leaves);
//   cost      0.125 * overhead + 1, the builder's own constants
//             (bvh_build.cpp: cost = 0.125f + nl * la + nr * ra per unit of the
//             parent's area; a leaf costs 1).
// In a builder tree a hit-able leaf's box is its sphere's own box, so the leaf
// sum is the same for a refit tree and for any rebuild of the same spheres:
// only the inner sum can be improved, and cost / cost at build time says by how
// much the tree has decayed.
#include <cstring>

#include "internal.h"
#include "quality.h"

namespace mirt {

void quality_finish(const QualitySums& q, mirt_tree_quality* out)
{
    std::memset(out, 0, sizeof *out);
    const float a0 = bits_float(q.root_area_bits);
    out->root_area = a0;
    out->inner_nodes = q.inner_nodes;
    out->leaves = q.leaves;
    out->dead_leaves = q.dead_leaves;
    if (!quality_root_ok(a0)) {
        out->degenerate = 1;
        return;
    }
    const int e = quality_exponent(a0);
    out->clamped = q.clamped;
    out->inner_area = quality_sum_value(q.inner_hi, q.inner_lo, e);
    out->leaf_area = quality_sum_value(q.leaf_hi, q.leaf_lo, e);
    if (out->leaf_area == 0.0)
        out->overhead = out->inner_area == 0.0 ? 0.0 : INFINITY;
    else
        out->overhead = out->inner_area / out->leaf_area;
    out->cost = 0.125 * out->overhead + 1.0;
}

}  // namespace mirt

extern "C" {

int mirt_bvh_quality_flat(const mirt_node* nodes, int num_nodes, int num_spheres, mirt_tree_quality* out)
{
    const char* fn = "mirt_bvh_quality_flat";
    if (!out || num_nodes < 0 || num_spheres < 0 || (num_nodes > 0 && !nodes)) {
        mirt::set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (int rc = mirt::validate_flat(nodes, num_nodes, num_spheres, 0, fn)) return rc;
    std::memset(out, 0, sizeof *out);
    if (num_nodes == 0) return MIRT_OK;
    mirt::QualitySums q{};
    const float a0 = mirt::box_area(nodes[0]);
    q.root_area_bits = mirt::float_bits(a0);
    const bool ok = mirt::quality_root_ok(a0);
    const double scale = ok ? mirt::quality_scale(mirt::quality_exponent(a0)) : 0.0;
    for (int i = 0; i < num_nodes; i++) {
        const mirt_node& n = nodes[i];
        const bool inner = n.sphere < 0;
        if (mirt::dead_leaf(n, num_spheres)) {
            q.dead_leaves++;
            continue;
        }
        (inner ? q.inner_nodes : q.leaves)++;
        if (!ok) continue;
        const uint64_t t = mirt::quality_term(mirt::box_area(n), a0, scale, &q.clamped);
        (inner ? q.inner_hi : q.leaf_hi) += t >> 24;
        (inner ? q.inner_lo : q.leaf_lo) += t & 0xffffffu;
    }
    mirt::quality_finish(q, out);
    return MIRT_OK;
}

}  // extern "C"

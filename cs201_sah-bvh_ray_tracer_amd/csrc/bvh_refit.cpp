// Refit of a flat pre-order tree (mirt_node) to spheres that have moved: the
// topology (sphere, skip) stays, every box is recomputed bottom-up. The host
// statement of the definition refit_device.hip's kernels implement, and the
// path for the inputs they decline.
//
//   hit-able leaf  a leaf without MIRT_NODE_EMPTY whose sphere < num_spheres;
//                  every other leaf is dead and keeps all its bytes;
//   precondition   the hit-able leaves' spheres s_0 < s_1 < ... < s_{k-1}
//                  increase strictly in pre-order and s_{k-1} < end <=
//                  num_spheres (property (2));
//   range          of hit-able leaf j: [s_j, s_{j+1}), of the last one
//                  [s_{k-1}, end): the builder's own ranges. A depth-40 leaf
//                  keeps the bounds of its whole range though it tests one
//                  sphere (layout.h, PNode);
//   leaf box       the empty box (+inf / -inf) folded with fl(c - r), fl(c + r)
//                  of the range's spheres in index order (bvh.c:120-125);
//   inner box      fmin / fmax of the boxes of its children i + 1 and
//                  skip(i + 1); a dead leaf contributes the empty box.
// For a tree the builder made and unchanged spheres these are the builder's
// own operations on the builder's own operands: the same bits.
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "internal.h"
#include "tree.h"

using namespace mirt;

extern "C" {

int mirt_bvh_refit_flat(mirt_node* nodes, int num_nodes, const mirt_sphere* spheres, int num_spheres, int end)
try {
    const char* fn = "mirt_bvh_refit_flat";
    if (num_nodes < 0 || num_spheres < 0 || (num_nodes > 0 && !nodes) || (num_spheres > 0 && !spheres)) {
        mirt::set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (int rc = mirt::validate_flat(nodes, num_nodes, num_spheres, 0, fn)) return rc;
    if (end < 0 || end > num_spheres) {
        mirt::set_error("%s: end %d outside [0, %d]", fn, end, num_spheres);
        return MIRT_E_INVALID;
    }
    const int nn = num_nodes, ns = num_spheres;
    int last = -1;  // the last hit-able leaf's sphere
    for (int i = 0; i < nn; i++) {
        if (!hitable(nodes[i], ns)) continue;
        if (nodes[i].sphere <= last) {
            mirt::set_error("%s: node %d holds sphere %d after sphere %d: the leaves' spheres do not increase", fn, i,
                            nodes[i].sphere, last);
            return MIRT_E_INVALID;
        }
        last = nodes[i].sphere;
    }
    if (end <= last) {
        mirt::set_error("%s: end %d does not lie behind the last leaf's sphere %d", fn, end, last);
        return MIRT_E_INVALID;
    }
    if (nn == 0) return MIRT_OK;
    // last to first: a node's children come after it, and a leaf's range ends where the next leaf's begins
    std::vector<Box> box((size_t)nn);
    int range_end = end;
    for (int i = nn - 1; i >= 0; i--) {
        const mirt_node& n = nodes[i];
        Box b = box_empty();
        if (n.sphere < 0) {
            const uint32_t l = (uint32_t)i + 1, r = skip_of(nodes[l]);
            b = box[l];
            box_merge(b, box[r]);
        } else if (hitable(n, ns)) {
            for (int k = n.sphere; k < range_end; k++) box_add(b, spheres[k]);
            range_end = n.sphere;
        }
        box[(size_t)i] = b;
    }
    for (int i = 0; i < nn; i++) {
        mirt_node& n = nodes[i];
        if (dead_leaf(n, ns)) continue;
        store_box(n, box[(size_t)i]);
    }
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    mirt::set_error("mirt_bvh_refit_flat: out of host memory");
    return MIRT_E_NOMEM;
}

}  // extern "C"

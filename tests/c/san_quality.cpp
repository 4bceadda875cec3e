// The host quality measure (csrc/bvh_quality.cpp) under the sanitizers:
// `make -C cs201_sah-bvh_ray_tracer_amd/csrc san_quality` links this driver with
// bvh_quality.cpp, bvh_refit.cpp, bvh_build.cpp and host_scene.cpp built
// -fsanitize=address,undefined (build/san_quality). It drives
// mirt_bvh_quality_flat on identity (a refit to unchanged spheres), moved,
// clamped (a leaf box larger than the root's, a NaN coordinate) and invalid
// inputs, on builder trees with stuck groups and 0-sphere leaves, a single
// leaf, a degenerate root and no tree. Exit 0 = every check held and no
// sanitizer fired (they abort on a finding). The last line also carries the
// sizes of the two new structs, for the test that compares abi.py with them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mirt.h"

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                               \
        }                                                             \
    } while (0)

static std::vector<mirt_sphere> scene(bool bench, int n, unsigned seed)
{
    std::vector<mirt_sphere> s((size_t)n);
    mirt_rand_state st;
    mirt_srand(&st, seed);
    if (bench)
        CHECK(mirt_scene_benchmark(&st, s.data(), n, 1000.0f) == MIRT_OK);
    else
        CHECK(mirt_scene_random(&st, s.data(), n) == MIRT_OK);
    return s;
}

static std::vector<mirt_node> flat_build(std::vector<mirt_sphere>& s, int start, int end, int depth)
{
    mirt_node* nodes = nullptr;
    int n = 0;
    CHECK(mirt_bvh_build_flat(s.data(), start, end, depth, &nodes, &n) == MIRT_OK);
    std::vector<mirt_node> out(nodes, nodes + n);
    mirt_bvh_free_flat(nodes);
    return out;
}

// a deterministic shake of the centres by up to +-amp
static std::vector<mirt_sphere> moved(const std::vector<mirt_sphere>& s, float amp, unsigned seed)
{
    std::vector<mirt_sphere> out = s;
    mirt_rand_state st;
    mirt_srand(&st, seed);
    auto unit = [&] { return (float)(mirt_rand(&st) % 20001) / 10000.0f - 1.0f; };
    for (mirt_sphere& p : out) {
        p.center.x += amp * unit();
        p.center.y += amp * unit();
        p.center.z += amp * unit();
    }
    return out;
}

static mirt_tree_quality quality(const std::vector<mirt_node>& nd, int ns)
{
    mirt_tree_quality q;
    std::memset(&q, 0xab, sizeof q);
    CHECK(mirt_bvh_quality_flat(nd.empty() ? nullptr : nd.data(), (int)nd.size(), ns, &q) == MIRT_OK);
    return q;
}

static bool same(const mirt_tree_quality& a, const mirt_tree_quality& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void identity_and_moved(std::vector<mirt_sphere> s, int start, int end, int depth, bool decays)
{
    const std::vector<mirt_node> tree = flat_build(s, start, end, depth);
    const int ns = (int)s.size();
    const mirt_tree_quality q = quality(tree, ns);
    CHECK(q.inner_nodes + q.leaves + q.dead_leaves == (int)tree.size());
    CHECK(q.clamped == 0 && (q.degenerate == 0 || tree.size() == 1));
    CHECK(q.cost == 0.125 * q.overhead + 1.0 || q.degenerate);
    std::vector<mirt_node> work = tree;
    CHECK(mirt_bvh_refit_flat(work.data(), (int)work.size(), s.data(), ns, end) == MIRT_OK);
    CHECK(same(quality(work, ns), q));
    double last = q.cost;
    for (float amp : {3.0f, 30.0f}) {
        const std::vector<mirt_sphere> s2 = moved(s, amp, 7);
        CHECK(mirt_bvh_refit_flat(work.data(), (int)work.size(), s2.data(), ns, end) == MIRT_OK);
        const mirt_tree_quality m = quality(work, ns);
        CHECK(m.inner_nodes == q.inner_nodes && m.leaves == q.leaves && m.dead_leaves == q.dead_leaves);
        CHECK(m.clamped == 0);
        if (decays) CHECK(m.cost > last);  // a shake of a dense scene: the tree gets worse
        last = m.cost;
    }
}

static mirt_node node(int32_t sphere, uint32_t skip)
{
    mirt_node n{};
    n.bmax[0] = n.bmax[1] = n.bmax[2] = 1.0f;
    n.sphere = sphere;
    n.skip = skip;
    return n;
}

int main()
{
    identity_and_moved(scene(false, 1000, 1), 0, 1000, 0, true);
    identity_and_moved(scene(false, 10000, 1), 0, 10000, 0, true);
    identity_and_moved(scene(true, 1000, 1), 0, 999, 20, false);  // benchmark.c:317
    {
        std::vector<mirt_sphere> s = scene(false, 64, 5);  // one stuck group of 32
        for (int i = 9; i < 40; i++) s[(size_t)i] = s[8];
        identity_and_moved(s, 0, 64, 0, false);
        std::vector<mirt_sphere> one(s.begin(), s.begin() + 1);
        const std::vector<mirt_node> leaf = flat_build(one, 0, 1, 0);
        const mirt_tree_quality q = quality(leaf, 1);
        CHECK(leaf.size() == 1 && q.leaves == 1 && q.inner_nodes == 0 && q.overhead == 0.0 && q.cost == 1.0);
        one[0].radius = 0.0f;  // the root's area is 0
        const mirt_tree_quality d = quality(flat_build(one, 0, 1, 0), 1);
        CHECK(d.degenerate == 1 && d.leaves == 1 && d.cost == 0.0 && d.leaf_area == 0.0 && d.root_area == 0.0f);
    }
    {   // clamped terms: a leaf box larger than the root's, a NaN coordinate
        std::vector<mirt_sphere> s = scene(false, 1000, 1);
        std::vector<mirt_node> tree = flat_build(s, 0, 1000, 0);
        const mirt_tree_quality q = quality(tree, 1000);
        size_t leaf = 0;
        while (tree[leaf].sphere < 0 || (tree[leaf].skip & MIRT_NODE_EMPTY) || tree[leaf].sphere >= 1000) leaf++;
        const mirt_node keep = tree[leaf];
        for (int a = 0; a < 3; a++) {
            tree[leaf].bmin[a] = tree[0].bmin[a] - 1.0f;
            tree[leaf].bmax[a] = tree[0].bmax[a] + 1.0f;
        }
        const mirt_tree_quality big = quality(tree, 1000);
        CHECK(big.clamped == 1 && big.leaf_area > q.leaf_area && big.inner_area == q.inner_area);
        CHECK(big.leaf_area < q.leaf_area + 2.0 * (double)q.root_area);  // the term is 2^48: less than twice the root
        tree[leaf] = keep;
        tree[leaf].bmin[1] = NAN;
        const mirt_tree_quality nan = quality(tree, 1000);
        CHECK(nan.clamped == 1 && nan.leaf_area < q.leaf_area && nan.leaf_area == nan.leaf_area);
        tree[leaf] = keep;
        CHECK(same(quality(tree, 1000), q));
    }
    {   // no tree, bad arguments, a malformed tree
        mirt_tree_quality q;
        std::memset(&q, 0xab, sizeof q);
        CHECK(mirt_bvh_quality_flat(nullptr, 0, 5, &q) == MIRT_OK);
        const mirt_tree_quality zero{};
        CHECK(same(q, zero));
        std::vector<mirt_node> ok = {node(-1, 3), node(0, 2), node(1, 3)};
        CHECK(mirt_bvh_quality_flat(ok.data(), 3, 2, nullptr) == MIRT_E_INVALID);
        CHECK(mirt_bvh_quality_flat(nullptr, 3, 2, &q) == MIRT_E_INVALID);
        CHECK(mirt_bvh_quality_flat(ok.data(), -1, 2, &q) == MIRT_E_INVALID);
        CHECK(mirt_bvh_quality_flat(ok.data(), 3, -1, &q) == MIRT_E_INVALID);
        CHECK(mirt_bvh_quality_flat(ok.data(), 3, 2, &q) == MIRT_OK);
        CHECK(q.inner_nodes == 1 && q.leaves == 2 && q.overhead == 0.5 && q.cost == 1.0625);
        CHECK(mirt_bvh_quality_flat(ok.data(), 3, 1, &q) == MIRT_OK);  // sphere 1 is now the never-hit sentinel
        CHECK(q.leaves == 1 && q.dead_leaves == 1 && q.overhead == 1.0);
        std::vector<mirt_node> bad = {node(-1, 3), node(0, 2), node(9, 3)};
        CHECK(mirt_bvh_quality_flat(bad.data(), 3, 3, &q) == MIRT_E_INVALID);
        CHECK(std::strstr(mirt_last_error(), "mirt_bvh_quality_flat: malformed node 2") != nullptr);
    }
    if (failures) {
        std::fprintf(stderr, "san_quality: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("san_quality: ok sizeof %zu %zu\n", sizeof(mirt_tree_quality), sizeof(mirt_update_result));
    return 0;
}

// Host half of libmirt (csrc/host_scene.cpp, bvh_build.cpp, bvh_cache.cpp,
// scene_layout.cpp) under the sanitizers: `make -C cs201_sah-bvh_ray_tracer_amd/csrc san`
// links this driver with those sources built -fsanitize=address,undefined
// (build/san_asan) and -fsanitize=thread (build/san_tsan). It exercises the
// threaded build (subtrees forked above 32k spheres), the pointer-tree build
// and flatten, tree validation on malformed input, the tree cache file
// on good, corrupt, truncated and unwritable paths, and the scene layout
// builders (build_scene_layout) on the tree shapes that steer their indexing. Exit 0 = every check held
// and no sanitizer fired (the sanitizers abort on a finding).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../cs201_sah-bvh_ray_tracer_amd/csrc/layout.h"
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

static bool same(const std::vector<mirt_node>& a, const std::vector<mirt_node>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(mirt_node)) == 0;
}

// build_scene_layout on a validated tree: every reference the walks would
// follow stays inside its array, and the arrays have the sizes the upload
// copies. Returns the number of 0-sphere leaves (MIRT_NODE_EMPTY).
static int check_layout(const std::vector<mirt_sphere>& s, int ns, const std::vector<mirt_node>& nd)
{
    using namespace mirt;
    const int nn = (int)nd.size();
    CHECK(mirt_bvh_validate_flat(nn ? nd.data() : nullptr, nn, ns) == MIRT_OK);
    SceneLayout lay;
    build_scene_layout(ns ? s.data() : nullptr, ns, nn ? nd.data() : nullptr, nn, lay);
    CHECK(lay.dnodes.size() == (size_t)nn && lay.geo.size() == (size_t)ns + 1 && lay.color.size() == (size_t)ns + 1);
    CHECK(lay.ndepth.size() == (size_t)(nn > 0 ? nn : 1));
    CHECK(lay.haux.size() == lay.hnodes.size() && lay.leaf_geo.size() == lay.leaf_box.size());
    CHECK(!lay.pnodes.empty() && !lay.hnodes.empty() && lay.wide_root < lay.hnodes.size());
    CHECK(lay.leaf_box_off % 256 == 0 && lay.leaf_box_off >= sizeof(Geo4) * lay.leaf_geo.size());
    for (const PNode& p : lay.pnodes)
        for (uint32_t ref : {p.ref0, p.ref1})
            CHECK(ref == kPNone || ((ref & kPLeaf) ? (ref & kPIndex) < (uint32_t)ns : ref < lay.pnodes.size()));
    for (const HNode& h : lay.hnodes)
        for (const HNode::Slot& sl : h.slot)
            CHECK(sl.ref == kPNone ||
                  ((sl.ref & kPLeaf) ? (sl.ref & kPIndex) < lay.leaf_box.size() : sl.ref < lay.hnodes.size()));
    for (const LeafBox& l : lay.leaf_box) CHECK(l.sphere >= 0 && l.sphere < ns);
    int empty = 0;
    for (const mirt_node& n : nd) empty += (n.skip & MIRT_NODE_EMPTY) != 0;
    return empty;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    // threaded flat build == pointer-tree build + flatten, for a scene large
    // enough to fork (render 60k) and the benchmark build [0, n-1) at depth 20
    for (int k = 0; k < 2; k++) {
        const bool bench = k == 1;
        const int n = bench ? 40000 : 60000;
        std::vector<mirt_sphere> s1 = scene(bench, n, 3), s2 = s1;
        const int end = bench ? n - 1 : n, depth = bench ? 20 : 0;
        std::vector<mirt_node> f = flat_build(s1, 0, end, depth);
        mirt_bvh_node* root = mirt_build_bvh_node(s2.data(), 0, end, depth);
        CHECK(root != nullptr);
        const int cnt = mirt_bvh_count(root);
        std::vector<mirt_node> g((size_t)cnt);
        CHECK(mirt_bvh_flatten(root, s2.data(), g.data(), cnt) == cnt);
        CHECK(same(f, g));
        CHECK(std::memcmp(s1.data(), s2.data(), s1.size() * sizeof(mirt_sphere)) == 0);
        CHECK(mirt_bvh_validate_flat(f.data(), (int)f.size(), n) == MIRT_OK);
        mirt_free_bvh(root);
        check_layout(s1, n, f);
    }

    // a benchmark scene built over [0, n - 1) from depth 20 (benchmark.c:317)
    // whose last spheres in range coincide: the SAH fallback's trailing
    // 0-sphere leaves point at spheres[n - 1], past the range -- a real sphere
    // when the array is declared whole, the never-hit sentinel when not
    {
        const int n = 2000, end = n - 1;
        std::vector<mirt_sphere> s = scene(true, n, 3);
        for (mirt_sphere& sp : s) sp.center.x -= 1000.0f;  // all x < 0: the fallback leaves its right child empty
        for (int i = end - 3; i < end; i++) {
            s[i].center = mirt_vec3{-1.0f, 600.0f, 600.0f};  // beyond the rest on every axis: last in the range
            s[i].radius = 1.0f;
        }
        std::vector<mirt_node> f = flat_build(s, 0, end, 20);
        int past = 0;
        for (const mirt_node& nd : f) past += (nd.skip & MIRT_NODE_EMPTY) && nd.sphere == end;
        CHECK(past > 0);
        check_layout(s, n, f);
        check_layout(s, end, f);
    }

    // negative radii: inverted boxes (c - r > c + r), so the builder's direct
    // form runs (every fourth radius: mixed nodes; all of them: every node).
    // The flat build equals the pointer-tree build, stays valid and lays out;
    // large enough to fork, so the direct form runs on the child threads too
    for (int every : {4, 1}) {
        const int n = 40000;
        std::vector<mirt_sphere> s1 = scene(false, n, 5);
        for (int i = 0; i < n; i += every) s1[i].radius = -s1[i].radius;
        std::vector<mirt_sphere> s2 = s1;
        std::vector<mirt_node> f = flat_build(s1, 0, n, 0);
        mirt_bvh_node* root = mirt_build_bvh_node(s2.data(), 0, n, 0);
        CHECK(root != nullptr);
        const int cnt = mirt_bvh_count(root);
        std::vector<mirt_node> g((size_t)cnt);
        CHECK(mirt_bvh_flatten(root, s2.data(), g.data(), cnt) == cnt);
        CHECK(same(f, g));
        mirt_free_bvh(root);
        int inverted = 0;
        for (const mirt_node& nd : f) inverted += nd.sphere < 0 && nd.bmax[0] < nd.bmin[0];
        CHECK(every == 4 || inverted > 0);
        check_layout(s1, n, f);
    }

    // scene layouts of the degenerate shapes: no tree, nothing at all, a single
    // leaf, a small built tree, and coincident spheres (one-sided chains of
    // 0-sphere leaves down to the depth cap)
    {
        std::vector<mirt_sphere> s = scene(false, 5, 1);
        check_layout(s, 5, {});
        check_layout({}, 0, {});
        std::vector<mirt_sphere> one = scene(false, 1, 1);
        std::vector<mirt_node> f = flat_build(one, 0, 1, 0);
        CHECK(f.size() == 1);
        check_layout(one, 1, f);
        s = scene(false, 1000, 2);
        f = flat_build(s, 0, 1000, 0);
        check_layout(s, 1000, f);
        s = scene(false, 300, 7);
        for (int k = 0; k < 40; k++)
            for (int j = 0; j < 6; j++) s.push_back(s[k]);
        f = flat_build(s, 0, (int)s.size(), 0);
        CHECK(check_layout(s, (int)s.size(), f) > 100);
    }

    // malformed trees are rejected, never walked out of bounds
    {
        std::vector<mirt_sphere> s = scene(false, 500, 5);
        std::vector<mirt_node> f = flat_build(s, 0, 500, 0);
        const int nn = (int)f.size();
        CHECK(mirt_bvh_validate_flat(f.data(), nn - 1, 500) == MIRT_E_INVALID);  // truncated
        std::vector<mirt_node> b = f;
        b[0].skip = (uint32_t)nn + 5;
        CHECK(mirt_bvh_validate_flat(b.data(), nn, 500) == MIRT_E_INVALID);  // root skip past the end
        b = f;
        for (int i = 0; i < nn; i++)
            if (b[i].sphere < 0) {
                b[i + 1].skip = (b[i + 1].skip & MIRT_NODE_EMPTY) | (uint32_t)nn;  // left subtree swallows all
                break;
            }
        CHECK(mirt_bvh_validate_flat(b.data(), nn, 500) == MIRT_E_INVALID);
        b = f;
        for (int i = 0; i < nn; i++)
            if (b[i].sphere >= 0) {
                b[i].sphere = 501;  // beyond the sentinel
                break;
            }
        CHECK(mirt_bvh_validate_flat(b.data(), nn, 500) == MIRT_E_INVALID);
        mirt_node two[2] = {};
        two[0].sphere = -1;
        two[0].skip = 2;
        two[1].sphere = 0;
        two[1].skip = 2;  // an inner node with one child
        CHECK(mirt_bvh_validate_flat(two, 2, 1) == MIRT_E_INVALID);
    }

    // tree cache file: miss -> write, hit -> same bytes, corrupt / truncated -> rebuild
    {
        const std::string path = dir + "/san_host_tree.cache";
        std::remove(path.c_str());
        std::vector<mirt_sphere> s0 = scene(false, 40000, 9);
        std::vector<mirt_sphere> s1 = s0;
        std::vector<mirt_node> want = flat_build(s1, 0, 40000, 0);
        for (int pass = 0; pass < 4; pass++) {
            if (pass == 2) {  // flip a payload byte
                FILE* fp = std::fopen(path.c_str(), "r+b");
                CHECK(fp != nullptr);
                if (fp) {
                    std::fseek(fp, -100, SEEK_END);
                    int c = std::fgetc(fp);
                    std::fseek(fp, -100, SEEK_END);
                    std::fputc(c ^ 0x5a, fp);
                    std::fclose(fp);
                }
            }
            if (pass == 3) {  // truncate to half
                FILE* fp = std::fopen(path.c_str(), "rb");
                std::vector<char> buf(1 << 20);
                size_t got = fp ? std::fread(buf.data(), 1, buf.size(), fp) : 0;
                if (fp) std::fclose(fp);
                fp = std::fopen(path.c_str(), "wb");
                if (fp) {
                    std::fwrite(buf.data(), 1, got / 2, fp);
                    std::fclose(fp);
                }
            }
            std::vector<mirt_sphere> s = s0;
            mirt_node* nodes = nullptr;
            int n = 0, cached = -2;
            CHECK(mirt_bvh_build_flat_cached(path.c_str(), s.data(), 0, 40000, 0, &nodes, &n, &cached) == MIRT_OK);
            CHECK(cached == (pass == 1 ? 1 : 0));
            CHECK(n == (int)want.size() && std::memcmp(nodes, want.data(), want.size() * sizeof(mirt_node)) == 0);
            CHECK(std::memcmp(s.data(), s1.data(), s.size() * sizeof(mirt_sphere)) == 0);
            mirt_bvh_free_flat(nodes);
        }
        std::vector<mirt_sphere> s = s0;
        mirt_node* nodes = nullptr;
        int n = 0, cached = -2;
        CHECK(mirt_bvh_build_flat_cached("/nonexistent-dir/x/tree.cache", s.data(), 0, 40000, 0, &nodes, &n, &cached) ==
              MIRT_OK);
        CHECK(cached == -1 && n == (int)want.size());
        mirt_bvh_free_flat(nodes);
        std::remove(path.c_str());
    }
    std::printf("san_host: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}

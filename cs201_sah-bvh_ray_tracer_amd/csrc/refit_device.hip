// Refit of a resident scene on the device (mirt_scene_refit_device[_ptr]): the
// boxes of the resident 32-B tree recomputed from moved spheres into a scratch
// tree, by the definition bvh_refit.cpp states on the host, then the device
// layouts derived again by scene_device.hip's layout_device and installed.
//
//   mark     per node: the node copied to the scratch tree (dead leaves keep
//            their bytes, sphere and skip never change); a hit-able leaf marks
//            its sphere as the start of a range; the smallest and largest such
//            sphere and the deepest inner node are reduced into ctl;
//   spheres  per sphere of [s_0, end): the inputs the kernels decline;
//   leaves   per hit-able leaf: its range runs from its sphere to the next
//            marked sphere (or end). A lane folds up to kShort spheres; a longer
//            range (a stuck group) is queued and folded by one wave, 64 spheres
//            a step, so a scene of identical spheres costs ns / 64 steps;
//   levels   one launch per depth, deepest first (design A of DESIGN.md 9.2):
//            a node's children are one level down, written by the launch
//            before. The kernel boundary is the only hand-off.
// The resident scene is `ordered` (else the host refits), so the leaves'
// spheres increase in pre-order, every mark is set once, and no node is deeper
// than 62: ndepth is exact. A box is fmin / fmax over finite values none of
// which is -0.0 (declined), so the order of combination does not show: the
// host's bits, from the box operations of tree.h that bvh_refit.cpp folds with.
// Every loop is bounded at launch; no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "device_util.h"
#include "internal.h"
#include "quality.h"
#include "tree.h"

#pragma clang fp contract(off)

namespace {

using namespace mirt;

constexpr int kBlock = 256;
constexpr int kShort = 64;  // spheres a single lane folds before the leaf goes to a wave

// ctl words (device, read back by the host)
enum {
    kMinLive = 0,  // smallest / largest sphere of a hit-able leaf (INT_MAX / -1: none)
    kMaxLive,
    kMaxDepth,     // depth of the deepest inner node (-1: none)
    kDeclined,     // a sphere the kernels decline
    kLong,         // leaves queued for the wave kernel
    kCtlWords = 8
};

__device__ __forceinline__ void add_sphere(Box& b, const uint32_t* aos, int k)
{
    const uint32_t* s = aos + 5 * (size_t)k;
    box_add(b, __uint_as_float(s[0]), __uint_as_float(s[1]), __uint_as_float(s[2]), __uint_as_float(s[3]));
}

// a child's box into its parent's; a dead leaf contributes the empty box
__device__ __forceinline__ void merge_child(Box& b, const mirt_node& child, int ns)
{
    if (!dead_leaf(child, ns)) box_merge(b, node_box(child));
}

// mark: ns + 1 bytes, zeroed
__global__ void mark_kernel(const mirt_node* nd, int nn, int ns, const uint8_t* ndepth, mirt_node* out, uint8_t* mark,
                            int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    const mirt_node n = nd[i];
    out[i] = n;
    if (n.sphere < 0) {
        const int d = ndepth[i];
        global_max(&ctl[kMaxDepth], d);
    } else if (hitable(n, ns)) {
        mark[n.sphere] = 1;
        global_min(&ctl[kMinLive], n.sphere);
        global_max(&ctl[kMaxLive], n.sphere);
    }
}

__global__ void decline_kernel(const uint32_t* aos, int end, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= end || i < ctl[kMinLive]) return;
    const uint32_t* s = aos + 5 * (size_t)i;
    if (sphere_declined(s[0], s[1], s[2], s[3])) flag(ctl, kDeclined);
}

// queue: nn ints
__global__ void leaves_kernel(const mirt_node* nd, int nn, int ns, const uint32_t* aos, int end, const uint8_t* mark,
                              mirt_node* out, int* queue, int* ctl)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn) return;
    const mirt_node n = nd[i];
    if (!hitable(n, ns) || n.sphere >= end) return;  // end <= a leaf's sphere: the host refuses the call
    Box b = box_empty();
    int k = n.sphere;
    for (int step = 0; step < kShort && k < end && (k == n.sphere || !mark[k]); step++, k++) add_sphere(b, aos, k);
    if (k < end && !mark[k]) {
        const int q = atomicAdd(&ctl[kLong], 1);
        if (q < nn) queue[q] = i;
        return;
    }
    store_box(out[i], b);
}

// one wave per queued leaf
__global__ void long_leaves_kernel(const mirt_node* nd, int nn, const uint32_t* aos, int end, const uint8_t* mark,
                                   mirt_node* out, const int* queue, int count)
{
    const int w = (int)((blockIdx.x * (unsigned)kBlock + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (w >= count) return;
    const int i = queue[w];
    if (i < 0 || i >= nn) return;
    const int first = nd[i].sphere;
    Box b = box_empty();
    for (int base = first; base < end; base += 64) {
        const int k = base + lane;
        const bool in = k < end && (k == first || !mark[k]);
        const unsigned long long stop = __ballot(!in);
        const bool mine = stop ? lane < __builtin_ctzll(stop) : true;
        if (mine) add_sphere(b, aos, k);
        if (stop) break;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; a++) {
            b.lo[a] = fminf(b.lo[a], __shfl_xor(b.lo[a], off));
            b.hi[a] = fmaxf(b.hi[a], __shfl_xor(b.hi[a], off));
        }
    if (lane == 0) store_box(out[i], b);
}

// the inner nodes of depth d from their children, which the launches before finished
__global__ void level_kernel(mirt_node* out, int nn, int ns, const uint8_t* ndepth, int d)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nn || ndepth[i] != d || out[i].sphere >= 0 || i + 1 >= nn) return;
    const mirt_node l = out[i + 1];
    const uint32_t ri = skip_of(l);
    if (ri >= (uint32_t)nn) return;
    const mirt_node r = out[ri];
    Box b = box_empty();
    merge_child(b, l, ns);
    merge_child(b, r, ns);
    store_box(out[i], b);
}

// mirt_scene_update_device's rebuild: the build ran on spheres whose colour word held their index, and the
// builders never read it. perm[i] = the index that travelled to place i; the sphere's own colour goes back.
__global__ void perm_kernel(uint32_t* aos, int ns, const uint32_t* colour, int32_t* perm)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ns) return;
    const uint32_t from = aos[5 * (size_t)i + 4];
    perm[i] = (int32_t)from;
    if (from < (uint32_t)ns) aos[5 * (size_t)i + 4] = colour[from];
}

// mirt_scene_update_device_ptr's refit branch: the identity permutation, written on the device
__global__ void iota_kernel(int32_t* perm, int ns)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < ns) perm[i] = i;
}

// ---- host side

// The refit kernels on stream s: d_tree[nn] from the resident tree and the spheres at d_aos. *verdict = 0: d_tree is
// the refit tree once the stream has run; 1: an input the kernels decline. Blocking (one read-back).
int refit_kernels(hipStream_t s, const ResidentScene& rs, const uint32_t* d_aos, int end, mirt_node* d_tree,
                  int* verdict, const char* fn)
{
    const int nn = rs.num_nodes, ns = rs.num_spheres;
    // scratch, one allocation: the ctl words, the queue of long leaves, the range marks
    const size_t bytes = ((size_t)kCtlWords + (size_t)nn) * 4 + (size_t)ns + 1;
    DevMem scratch;
    HIP_TRY(hipMalloc(&scratch.p, bytes));
    int* ctl = (int*)scratch.p;
    int* queue = ctl + kCtlWords;
    uint8_t* mark = (uint8_t*)(queue + nn);
    int h[kCtlWords] = {};
    h[kMinLive] = INT_MAX;
    h[kMaxLive] = h[kMaxDepth] = -1;
    HIP_TRY(hipMemsetAsync(scratch.p, 0, bytes, s));
    HIP_TRY(hipMemcpyAsync(ctl, h, sizeof h, hipMemcpyHostToDevice, s));
    const unsigned gn = blocks((size_t)nn, kBlock);
    mark_kernel<<<gn, kBlock, 0, s>>>(rs.nodes32, nn, ns, rs.ndepth, d_tree, mark, ctl);
    if (end > 0) decline_kernel<<<blocks((size_t)end, kBlock), kBlock, 0, s>>>(d_aos, end, ctl);
    leaves_kernel<<<gn, kBlock, 0, s>>>(rs.nodes32, nn, ns, d_aos, end, mark, d_tree, queue, ctl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (end <= h[kMaxLive]) {
        set_error("%s: end %d does not lie behind the last leaf's sphere %d", fn, end, h[kMaxLive]);
        return MIRT_E_INVALID;
    }
    if (h[kLong] < 0 || h[kLong] > nn || h[kMaxDepth] > 62) {
        set_error("%s: the refit kernels queued %d of %d leaves below depth %d", fn, h[kLong], nn, h[kMaxDepth]);
        return MIRT_E_DEVICE;
    }
    *verdict = h[kDeclined] ? 1 : 0;
    if (*verdict) return MIRT_OK;
    if (h[kLong] > 0)
        long_leaves_kernel<<<blocks((size_t)h[kLong] * 64, kBlock), kBlock, 0, s>>>(rs.nodes32, nn, d_aos, end, mark,
                                                                                    d_tree, queue, h[kLong]);
    for (int d = h[kMaxDepth]; d >= 0; d--) level_kernel<<<gn, kBlock, 0, s>>>(d_tree, nn, ns, rs.ndepth, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));  // the scratch is free again; layout_ms starts behind the kernels
    return MIRT_OK;
}

// The checked entry of both calls: the ctx, the counts (`args_ok`: the caller's own test of them) and the
// resident scene, which must hold `ns` spheres.
int resident_scene(mirt_ctx* c, bool args_ok, int ns, ResidentScene* rs, const char* fn)
{
    if (!c) {
        set_error("%s: null context", fn);
        return MIRT_E_INVALID;
    }
    if (!args_ok) {
        set_error("%s: invalid arguments", fn);
        return MIRT_E_INVALID;
    }
    if (!ctx_resident_scene(c, rs)) {
        set_error("%s: no scene uploaded", fn);
        return MIRT_E_NOSCENE;
    }
    if (ns != rs->num_spheres) {
        set_error("%s: %d spheres for a resident scene of %d", fn, ns, rs->num_spheres);
        return MIRT_E_INVALID;
    }
    return MIRT_OK;
}

// The refit stage of both calls: the moved spheres on the device at d_aos (the caller's d_spheres, else `spheres`
// uploaded into `aos`) and the resident tree refit to them in `tree`. declined: the resident scene is not ordered or
// the kernels decline an input; there is no refit tree and the host refits. Nothing is installed.
struct Refit {
    DevMem aos, tree;
    const uint32_t* d_aos = nullptr;
    int declined = 0;
};
int refit_stage(hipStream_t s, const ResidentScene& rs, const mirt_sphere* spheres, const void* d_spheres, int end,
                Refit& r, const char* fn)
{
    const int nn = rs.num_nodes, ns = rs.num_spheres;
    const size_t sph_bytes = sizeof(mirt_sphere) * (size_t)ns, tree_bytes = sizeof(mirt_node) * (size_t)nn;
    r.declined = nn > 0 && !rs.ordered;
    if (r.declined) return MIRT_OK;
    r.d_aos = (const uint32_t*)d_spheres;
    if (!r.d_aos) {
        HIP_TRY(hipMalloc(&r.aos.p, std::max<size_t>(sph_bytes, 4)));
        if (ns > 0) HIP_TRY(hipMemcpyAsync(r.aos.p, spheres, sph_bytes, hipMemcpyHostToDevice, s));
        r.d_aos = (const uint32_t*)r.aos.p;
    }
    HIP_TRY(hipMalloc(&r.tree.p, std::max<size_t>(tree_bytes, sizeof(mirt_node))));
    int rc = MIRT_OK;
    if (nn > 0) rc = refit_kernels(s, rs, r.d_aos, end, (mirt_node*)r.tree.p, &r.declined, fn);
    if (rc || r.declined) (void)hipStreamSynchronize(s);  // the arrays are freed on the caller's way out
    return rc;
}

// The declined path's refit, on the host: the resident tree into `nodes`, refit there by mirt_bvh_refit_flat.
// *spheres null: the caller's spheres are on the device, and are fetched into `copy` first.
int host_refit(hipStream_t s, const ResidentScene& rs, const mirt_sphere** spheres, const void* d_spheres, int end,
               std::vector<mirt_sphere>& copy, std::vector<mirt_node>& nodes)
{
    const int nn = rs.num_nodes, ns = rs.num_spheres;
    nodes.resize((size_t)nn);
    HIP_TRY(hipStreamSynchronize(s));
    if (!*spheres && ns > 0) {
        copy.resize((size_t)ns);
        HIP_TRY(hipMemcpy(copy.data(), d_spheres, sizeof(mirt_sphere) * (size_t)ns, hipMemcpyDeviceToHost));
        *spheres = copy.data();
    }
    if (nn > 0) HIP_TRY(hipMemcpy(nodes.data(), rs.nodes32, sizeof(mirt_node) * (size_t)nn, hipMemcpyDeviceToHost));
    return mirt_bvh_refit_flat(nodes.data(), nn, *spheres, ns, end);
}

// The installs a refit or an update makes between here and the scope's end are ones a history can be carried over
// (MIRT_OPT_HISTORY_MOTION, ctx_link_intent): every path of both calls, the declined inputs' host uploads included.
struct LinkIntent {
    mirt_ctx* c;
    explicit LinkIntent(mirt_ctx* ctx) : c(ctx) { ctx_link_intent(c, false, nullptr, nullptr); }
    ~LinkIntent() { ctx_link_intent_clear(c); }
    void rebuild(const int32_t* d_perm, const int32_t* h_perm) { ctx_link_intent(c, true, d_perm, h_perm); }
};

// exactly one of `spheres` (host) and `d_spheres` (device) is set, unless ns == 0
int refit(mirt_ctx* c, const mirt_sphere* spheres, const void* d_spheres, int ns, int end, mirt_node* out_nodes,
          const char* fn)
try {
    ResidentScene rs{};
    if (int rc = resident_scene(c, ns >= 0 && (ns == 0 || spheres || d_spheres) && end >= 0 && end <= ns, ns, &rs, fn))
        return rc;
    LinkIntent link(c);
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    const int nn = rs.num_nodes;
    const size_t tree_bytes = sizeof(mirt_node) * (size_t)nn;
    mirt_refit_stats st{};
    st.nodes = nn;
    int declined;
    {
        Refit r;
        int rc = refit_stage(s, rs, spheres, d_spheres, end, r, fn);
        if (rc) return rc;
        declined = r.declined;
        if (!declined) {
            st.refit_ms = since(t0);
            const auto t1 = std::chrono::steady_clock::now();
            rc = layout_device(c, s, r.d_aos, ns, (const mirt_node*)r.tree.p, nn, fn);
            hipError_t e = hipSuccess;
            if (!rc && out_nodes && nn > 0)
                e = hipMemcpyAsync(out_nodes, r.tree.p, tree_bytes, hipMemcpyDeviceToHost, s);
            const hipError_t e2 = hipStreamSynchronize(s);
            if (rc) return rc;
            if (e != hipSuccess || e2 != hipSuccess) return hip_fail(e != hipSuccess ? e : e2, fn);
            st.layout_ms = since(t1);
            st.on_device = 1;
        }
    }
    if (declined) {
        // the host refit and the host upload on the resident tree: the same result
        std::vector<mirt_sphere> copy;
        std::vector<mirt_node> nodes;
        if (int rc = host_refit(s, rs, &spheres, d_spheres, end, copy, nodes)) return rc;
        if (int rc = mirt_scene_upload_flat(c, spheres, ns, nodes.data(), nn)) return rc;
        if (out_nodes) std::memcpy(out_nodes, nodes.data(), tree_bytes);
    }
    st.total_ms = since(t0);
    ctx_set_refit_stats(c, st);
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", fn);
    return MIRT_E_NOMEM;
}

// the spheres with the colour word of each replaced by its index: what a build is run on to learn its permutation
std::vector<mirt_sphere> indexed(const mirt_sphere* spheres, int ns)
{
    std::vector<mirt_sphere> out(spheres, spheres + ns);
    for (int32_t i = 0; i < ns; i++) std::memcpy(&out[(size_t)i].color, &i, 4);
    return out;
}

void identity(const mirt_sphere* spheres, int ns, mirt_sphere* reordered, int32_t* perm)
{
    if (reordered && ns > 0) std::memcpy(reordered, spheres, sizeof(mirt_sphere) * (size_t)ns);
    if (perm)
        for (int32_t i = 0; i < ns; i++) perm[i] = i;
}

// mirt_scene_update_device[_ptr]: refit into the scratch tree, measure it, then install either
// it or a rebuild. Nothing is installed, and the slot's base cost is not touched, before the decision's own tree is
// complete. Host form: `spheres`, `reordered`, `perm` in host memory. Device form (d_spheres set, or ptr_form with
// ns == 0): the spheres are read on the ctx's stream and d_reordered / d_perm written there; on the paths the
// kernels accept no sphere, colour or permutation crosses the host link.
int update(mirt_ctx* c, const mirt_sphere* spheres, const void* d_spheres, bool ptr_form, int ns, int start, int end,
           double max_decay, mirt_sphere* reordered, int32_t* perm, void* d_reordered, int32_t* d_perm_out,
           mirt_update_result* out, const char* fn)
try {
    ResidentScene rs{};
    const bool args_ok = ns >= 0 && (ns == 0 || spheres || d_spheres) && start >= 0 && end >= start && end <= ns &&
                         !(d_reordered && d_reordered == d_spheres);
    if (int rc = resident_scene(c, args_ok, ns, &rs, fn)) return rc;
    LinkIntent link(c);
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(ctx_device(c)));
    hipStream_t s = (hipStream_t)mirt_ctx_stream(c);
    const int nn = rs.num_nodes;
    const size_t sph_bytes = sizeof(mirt_sphere) * (size_t)ns;
    mirt_update_result res;
    std::memset(&res, 0, sizeof res);
    double base = 0.0;
    if (!ctx_base_cost(c, &base)) {  // the resident tree came from another call: its cost is the base
        mirt_tree_quality q;
        if (int rc = quality_device(s, rs.nodes32, nn, ns, &q, fn)) return rc;
        base = q.cost;
    }
    res.base_cost = base;
    double new_base = base;
    auto wants_rebuild = [&](const mirt_tree_quality& q) {
        res.cost = q.cost;
        res.decay = quality_decay(q.cost, base);
        return max_decay > 0.0 && res.decay > max_decay;
    };
    int declined;
    {
        Refit r;
        int rc = refit_stage(s, rs, spheres, d_spheres, end, r, fn);
        if (rc) return rc;
        declined = r.declined;
        const mirt_node* tree = (const mirt_node*)r.tree.p;
        mirt_tree_quality q;
        if (!declined && (rc = quality_device(s, tree, nn, ns, &q, fn))) return rc;
        if (!declined && !wants_rebuild(q)) {
            rc = layout_device(c, s, r.d_aos, ns, tree, nn, fn);
            hipError_t e = hipSuccess;
            if (!rc && ptr_form && ns > 0) {
                if (d_reordered) e = hipMemcpyAsync(d_reordered, d_spheres, sph_bytes, hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess && d_perm_out) {
                    iota_kernel<<<blocks((size_t)ns, kBlock), kBlock, 0, s>>>(d_perm_out, ns);
                    e = hipGetLastError();
                }
            }
            const hipError_t e2 = hipStreamSynchronize(s);
            if (rc) return rc;
            if (e != hipSuccess || e2 != hipSuccess) return hip_fail(e != hipSuccess ? e : e2, fn);
            if (!ptr_form) identity(spheres, ns, reordered, perm);
            res.installed = q;
            res.on_device = 1;
        } else if (!declined) {
            // the spheres' own colours, then the permutation: one allocation
            DevMem extra;
            HIP_TRY(hipMalloc(&extra.p, std::max<size_t>((size_t)ns * 8, 8)));
            uint32_t* d_colour = (uint32_t*)extra.p;
            int32_t* d_perm = (int32_t*)(d_colour + ns);
            std::vector<mirt_sphere> copy;
            std::vector<uint32_t> colour;
            ResidentTree built{};
            if (ptr_form) {
                rc = build_resident_tagged(c, d_spheres, ns, start, end, 0, d_colour, &built, &declined);
            } else {
                copy = indexed(spheres, ns);
                rc = build_resident(c, copy.data(), ns, start, end, 0, &built, &declined);
            }
            if (rc) return rc;
            if (!declined) {
                hipError_t e = hipSuccess;
                if (!ptr_form && ns > 0) {
                    colour.resize((size_t)ns);
                    for (int i = 0; i < ns; i++) std::memcpy(&colour[(size_t)i], &spheres[i].color, 4);
                    e = hipMemcpyAsync(d_colour, colour.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s);
                }
                if (e == hipSuccess && ns > 0) {
                    perm_kernel<<<blocks((size_t)ns, kBlock), kBlock, 0, s>>>((uint32_t*)built.aos, ns, d_colour,
                                                                               d_perm);
                    e = hipGetLastError();
                }
                link.rebuild(d_perm, nullptr);   // (written by perm_kernel on `s`, ahead of the install's copy of it)
                mirt_tree_quality qb;
                if (e == hipSuccess) rc = quality_device(s, built.nodes, built.num_nodes, ns, &qb, fn);
                if (e == hipSuccess && !rc) rc = layout_device(c, s, built.aos, ns, built.nodes, built.num_nodes, fn);
                void* const to_reordered = ptr_form ? d_reordered : (void*)reordered;
                void* const to_perm = ptr_form ? (void*)d_perm_out : (void*)perm;
                const hipMemcpyKind kind = ptr_form ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
                if (e == hipSuccess && !rc && to_reordered && ns > 0)
                    e = hipMemcpyAsync(to_reordered, built.aos, sph_bytes, kind, s);
                if (e == hipSuccess && !rc && to_perm && ns > 0)
                    e = hipMemcpyAsync(to_perm, d_perm, (size_t)ns * 4, kind, s);
                const hipError_t e2 = hipStreamSynchronize(s);  // `copy`, `colour` and `extra` are free again
                if (rc) return rc;
                if (e != hipSuccess || e2 != hipSuccess) return hip_fail(e != hipSuccess ? e : e2, fn);
                res.rebuilt = 1;
                res.installed = qb;
                res.on_device = 1;
                new_base = qb.cost;
            } else {
                HIP_TRY(hipStreamSynchronize(s));
            }
        }
    }
    if (declined) {
        // the host refit, the host measure, then the host upload or the host build and upload: the same result
        // (device form: the spheres are fetched, and reordered and perm uploaded)
        std::vector<mirt_sphere> fetched, h_reordered;
        std::vector<int32_t> h_perm;
        if (ptr_form) {
            if (d_reordered) reordered = (h_reordered.resize((size_t)std::max(ns, 1)), h_reordered.data());
            if (d_perm_out) perm = (h_perm.resize((size_t)std::max(ns, 1)), h_perm.data());
        }
        std::vector<mirt_node> nodes;
        if (int rc = host_refit(s, rs, &spheres, d_spheres, end, fetched, nodes)) return rc;
        mirt_tree_quality q;
        if (int rc = mirt_bvh_quality_flat(nodes.data(), nn, ns, &q)) return rc;
        if (!wants_rebuild(q)) {
            if (int rc = mirt_scene_upload_flat(c, spheres, ns, nodes.data(), nn)) return rc;
            identity(spheres, ns, reordered, perm);
            res.installed = q;
        } else {
            std::vector<mirt_sphere> copy = indexed(spheres, ns);
            mirt_node* bn = nullptr;
            int bcount = 0;
            if (int rc = mirt_bvh_build_flat(copy.data(), start, end, 0, &bn, &bcount)) return rc;
            std::vector<int32_t> from((size_t)ns);
            for (int i = 0; i < ns; i++) {
                std::memcpy(&from[(size_t)i], &copy[(size_t)i].color, 4);
                copy[(size_t)i].color = spheres[from[(size_t)i]].color;
            }
            mirt_tree_quality qb;
            int rc = mirt_bvh_quality_flat(bn, bcount, ns, &qb);
            link.rebuild(nullptr, from.data());
            if (!rc) rc = mirt_scene_upload_flat(c, copy.data(), ns, bn, bcount);
            mirt_bvh_free_flat(bn);
            if (rc) return rc;
            if (reordered && ns > 0) std::memcpy(reordered, copy.data(), sph_bytes);
            if (perm && ns > 0) std::memcpy(perm, from.data(), (size_t)ns * 4);
            res.rebuilt = 1;
            res.installed = qb;
            new_base = qb.cost;
        }
        if (ptr_form && ns > 0) {
            if (d_reordered) HIP_TRY(hipMemcpy(d_reordered, reordered, sph_bytes, hipMemcpyHostToDevice));
            if (d_perm_out) HIP_TRY(hipMemcpy(d_perm_out, perm, (size_t)ns * 4, hipMemcpyHostToDevice));
        }
        res.on_device = 0;
    }
    ctx_set_base_cost(c, new_base);
    res.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (out) *out = res;
    return MIRT_OK;
} catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", fn);
    return MIRT_E_NOMEM;
}

}  // namespace

extern "C" {

int mirt_scene_update_device(mirt_ctx* c, const mirt_sphere* spheres, int num_spheres, int start, int end,
                             double max_decay, mirt_sphere* reordered, int32_t* perm, mirt_update_result* out)
{
    return update(c, spheres, nullptr, false, num_spheres, start, end, max_decay, reordered, perm, nullptr, nullptr, out,
                  "mirt_scene_update_device");
}

int mirt_scene_update_device_ptr(mirt_ctx* c, const void* d_spheres, int num_spheres, int start, int end,
                                 double max_decay, void* d_reordered, int32_t* d_perm, mirt_update_result* out)
{
    return update(c, nullptr, d_spheres, true, num_spheres, start, end, max_decay, nullptr, nullptr, d_reordered,
                  d_perm, out, "mirt_scene_update_device_ptr");
}

int mirt_scene_refit_device(mirt_ctx* c, const mirt_sphere* spheres, int num_spheres, int end, mirt_node* out_nodes)
{
    return refit(c, spheres, nullptr, num_spheres, end, out_nodes, "mirt_scene_refit_device");
}

int mirt_scene_refit_device_ptr(mirt_ctx* c, const void* d_spheres, int num_spheres, int end, mirt_node* out_nodes)
{
    return refit(c, nullptr, d_spheres, num_spheres, end, out_nodes, "mirt_scene_refit_device_ptr");
}

}  // extern "C"

/*
 * include/mirt.h -- C ABI of the MI355X-native primary-ray render path
 * (camera rays -> BVH traversal + ray/sphere intersection -> closest-hit
 * diffuse shading -> RGBA framebuffer) of ShivangNagta/CS201_SAH-BVH_Ray_Tracer.
 *
 * Every entry point is plain C: POD structs, pointers and sizes, int status.
 * Structs are layout-compatible with the reference's own types (sizes are
 * asserted in csrc/host_scene.cpp), so a caller can pass its arrays through
 * unchanged. The reference interface each entry point replaces is cited as
 * file:line under /root/reference/ (see also INTEGRATION.md).
 *
 * Threading: one host thread per mirt_ctx. Blocking calls return with the
 * result in host memory; *_device calls enqueue on the given HIP stream.
 * Errors: negative status, message in mirt_last_error(); the library never
 * aborts and never falls back to a CPU path.
 *
 * Diagnostic surface (for the test suite; may change between releases):
 * mirt_box_form_pairs and mirt_sphere_form_pairs run the walks' filtered box
 * and sphere tests on caller-given pairs; mirt_build_partition_probe runs the
 * device build's partition on caller-given keys; mirt_scene_layout returns
 * the device layouts an upload derives from a scene, computed on the host.
 */
#ifndef MIRT_H
#define MIRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ types */

typedef struct mirt_vec3 { float x, y, z; } mirt_vec3;            /* vec3.h:3-7 (12 B)   */
typedef struct mirt_rgba8 { uint8_t r, g, b, a; } mirt_rgba8;     /* SDL_Color (4 B)     */
typedef struct mirt_sphere {                                      /* sphere.h:7-11 (20 B) */
    mirt_vec3 center;
    float radius;
    mirt_rgba8 color;
} mirt_sphere;
typedef struct mirt_ray { mirt_vec3 origin, direction; } mirt_ray; /* ray.h:5-8 (24 B)   */
typedef struct mirt_camera {                                      /* camera.h:5-14 (64 B) */
    mirt_vec3 position, forward, right, up;
    float yaw, pitch, fov;
    int move;
} mirt_camera;
typedef struct mirt_aabb { mirt_vec3 min, max; } mirt_aabb;       /* bvh.h:7-10 (24 B)   */
typedef struct mirt_bvh_node {                                    /* bvh.h:12-18 (56 B)  */
    mirt_aabb bounds;
    struct mirt_bvh_node *left, *right;
    mirt_sphere *sphere;
    int sphere_count;
} mirt_bvh_node;
typedef struct mirt_hit_record {                                  /* hit.h:8-14 (40 B)   */
    float t;
    mirt_vec3 point, normal;
    int hit_something;
    mirt_sphere *object;
} mirt_hit_record;

/* HitRecord for batch calls: the object pointer becomes an index into the
   uploaded sphere array (-1: no hit). 40 B. */
typedef struct mirt_hit {
    float t;
    mirt_vec3 point, normal;
    int32_t hit;
    int32_t sphere;
    int32_t pad;
} mirt_hit;

/* Flattened BVH node, the layout the kernel walks (32 B, 32-B aligned).
   Depth-first pre-order of the reference tree (bvh.c:203-204: left subtree,
   then right): the left child of inner node i is i+1 and `skip` is the index
   that follows i's subtree, so the reference DFS order (hit.c:102-103) is a
   forward scan that jumps to `skip` when a box is missed or a leaf is done.
   sphere  >= 0: leaf testing spheres[sphere] (bvh.c:133; == num_spheres is the
            never-hit sentinel of SURVEY §8.H7); -1: inner node.
   skip bit 31 (MIRT_NODE_EMPTY): the leaf holds 0 spheres; its box is the
            inverted create_empty_aabb() box (bvh.c:19-24), which always passes
            ray_aabb_intersect (hit.c:49-82). */
typedef struct mirt_node {
    float bmin[3];
    float bmax[3];
    int32_t sphere;
    uint32_t skip;
} mirt_node;
#define MIRT_NODE_EMPTY 0x80000000u
#define MIRT_SKIP_MASK 0x7fffffffu

/* glibc TYPE_3 rand() state (the reference seeds glibc with srand(),
   main.c:90, benchmark.c:287). */
typedef struct mirt_rand_state {
    int32_t r[34];
    int32_t f, b;
} mirt_rand_state;

/* One frame (or one shard of one frame). */
typedef struct mirt_frame_desc {
    int32_t width, height;   /* the reference's compile-time WIDTH/HEIGHT (constants.h:7-8) */
    int32_t max_depth;       /* trace_ray depth argument (main.c:366, MAX_DEPTH = 5) */
    int32_t use_bvh;         /* main.c:366 `use_bvh ? root : NULL`; 0 = brute force */
    uint64_t seed;           /* RNG contract seed */
    uint32_t sample;         /* RNG contract sample index (frame number) */
    int32_t accumulate;      /* 0: fresh frame main.c:358-374; 1: accumulate main.c:379-408 */
    int32_t frames;          /* accumulate: divisor accumulated_frames (main.c:380) */
    int32_t row_block;       /* rows per interleave block (default 8) */
    int32_t shard;           /* this shard renders row blocks b with b % num_shards == shard */
    int32_t num_shards;
    int32_t samples;         /* frames rendered by this call, samples sample .. sample+samples-1 of the
                                RNG contract (0 or 1: one; at most 64). The sum is taken in uint32_t:
                                frame j uses (sample + j) mod 2^32, so four frames from sample
                                0xFFFFFFFE use 0xFFFFFFFE, 0xFFFFFFFF, 0 and 1 -- what four calls
                                with a uint32_t counter would pass. One launch covers all of them, so the
                                bounce pass's tail (its longest chains) is paid once, not per frame.
                                Output: `samples` consecutive slabs, one per frame; with an
                                accumulation buffer, the frames are folded into it in order (as
                                `samples` successive calls would: frame j has divisor frames + j)
                                and slab j holds the display main.c:379-408 shows after frame j
                                (the blocking / async calls return the last one) */
    int32_t jitter;          /* 1: camera rays through (x + jx, y + jy), j in [0, 1)^2 from the pixel's
                                RNG contract stream (rng.h; BASELINE configs[4] "4 spp jittered" --
                                the reference samples pixel corners only); 0: main.c:362-363 */
    int32_t lead_skip;       /* shard weighting (mirt 0.6; 0 = none): blocks are dealt in periods of 8
                                rounds, one block per shard per round, and shard 0 sits out the first
                                lead_skip (0..7) rounds of every period -- so shard 0 renders
                                (8 - lead_skip) / (8 num_shards - lead_skip) of the frame
                                (csrc/shard.h). 0 = block b to shard b % num_shards. num_shards >= 2 */
} mirt_frame_desc;

/* Work counters of the walk as configured; with MIRT_OPT_PRUNE = 0 they are
   exactly the reference DFS (hit.c:91-109) node and sphere tests. */
typedef struct mirt_counts {
    uint64_t rays;       /* rays traced (primary + bounces) */
    uint64_t nodes;      /* ray_aabb_intersect calls */
    uint64_t spheres;    /* ray_sphere_intersect calls from leaves (or brute force) */
    uint64_t hits;       /* rays that found a closest hit */
    uint64_t lane_steps; /* traversal loop iterations x 64 lanes executed by the
                            default schedule; nodes / lane_steps = SIMD efficiency */
    /* the camera-ray level alone (depth level 0 = the wavefront schedule's
       primary pass); nodes - nodes_primary etc. is the bounce pass */
    uint64_t nodes_primary;
    uint64_t spheres_primary;
    uint64_t hits_primary;
} mirt_counts;

enum {
    MIRT_OK = 0,
    MIRT_E_INVALID = -1,
    MIRT_E_NOMEM = -2,
    MIRT_E_NOSCENE = -3,
    MIRT_E_DEVICE = -4   /* HIP runtime error; see mirt_last_error() */
};

typedef struct mirt_ctx mirt_ctx;

const char *mirt_version(void);
const char *mirt_last_error(void);

/* ------------------------------------------------- host: scene inputs */

/* glibc srand()/rand() restated (TYPE_3 additive feedback), so scenes are
   reproducible from a seed on any host. */
void mirt_srand(mirt_rand_state *st, unsigned int seed);
int mirt_rand(mirt_rand_state *st);

/* n x create_random_sphere() (sphere.c:52-59) as main.c:218-221. */
int mirt_scene_random(mirt_rand_state *st, mirt_sphere *out, int n);
/* n x benchmark centre + create_benchmark_sphere() (benchmark.c:307-314, sphere.c:34-41). */
int mirt_scene_benchmark(mirt_rand_state *st, mirt_sphere *out, int n, float world_size);
/* n benchmark rays (benchmark.c:176-185, 228-237): origin 0, direction
   vec3_normalize of three (float)rand()/RAND_MAX*2-1 draws. */
int mirt_bench_rays(mirt_rand_state *st, mirt_ray *out, int n);
/* The default camera of main.c:203-211. */
void mirt_camera_default(mirt_camera *cam);
/* camera_update (camera.c:10-18): basis from yaw/pitch. */
void mirt_camera_update(mirt_camera *cam);

/* --------------------------------------------- host: BVH (bit-identical) */

/* build_bvh_node (bvh.c:117-209): same signature, same pointer tree, same
   in-place reordering of `spheres`. Free with mirt_free_bvh. */
mirt_bvh_node *mirt_build_bvh_node(mirt_sphere *spheres, int start, int end, int depth);
/* free_bvh (benchmark.c:81-88) */
void mirt_free_bvh(mirt_bvh_node *node);
/* Number of nodes in a pointer tree. */
int mirt_bvh_count(const mirt_bvh_node *root);
/* Flatten a pointer tree (built by the reference's build_bvh_node or by
   mirt_build_bvh_node) whose leaf pointers index `base`. Returns the node
   count, or -needed if cap is too small. */
int mirt_bvh_flatten(const mirt_bvh_node *root, const mirt_sphere *base, mirt_node *out, int cap);
/* Build straight into the flat layout: same tree as
   mirt_bvh_flatten(build_bvh_node(spheres, start, end, depth)) bit for bit,
   with the SAH planes of bvh.c:143-170 evaluated by one binned pass per axis.
   *out_nodes is malloc'd; release with mirt_bvh_free_flat. */
int mirt_bvh_build_flat(mirt_sphere *spheres, int start, int end, int depth,
                        mirt_node **out_nodes, int *out_count);
void mirt_bvh_free_flat(mirt_node *nodes);
/* Check that nodes[0, num_nodes) is a well-formed flat pre-order tree over
   num_spheres spheres: root skip == num_nodes, every skip in (i, num_nodes],
   leaves skip to i + 1 and index spheres in [0, num_spheres] (num_spheres =
   the never-hit sentinel), MIRT_NODE_EMPTY only on leaves, and every inner
   node's two subtrees [i+1, r) and [r, skip) nest exactly inside it.
   MIRT_OK or MIRT_E_INVALID (mirt_last_error names the first bad node). The
   uploads run this check; it never touches the GPU. */
int mirt_bvh_validate_flat(const mirt_node *nodes, int num_nodes, int num_spheres);
/* mirt_bvh_build_flat through a flattened-tree cache file (SURVEY.md §8(f)
   rank 3; replaces the build_bvh_node call at main.c:225 / benchmark.c:317 on
   a rerun). If `path` holds the tree of exactly these input spheres
   (FNV-1a 64 of spheres[start,end) + start, end, depth; payload hash checked)
   the reordered spheres are copied into spheres[start,end), the nodes are
   returned and *out_cached = 1. Otherwise the tree is built, written to
   `path` (temp file + rename) and *out_cached = 0, or -1 if the file could
   not be written (the build result is still returned; mirt_last_error says
   why). Same outputs as mirt_bvh_build_flat, bit for bit. */
int mirt_bvh_build_flat_cached(const char *path, mirt_sphere *spheres, int start, int end, int depth,
                               mirt_node **out_nodes, int *out_count, int *out_cached);

/* ------------------------------------------------------ device context */

int mirt_create(int device, mirt_ctx **out);
void mirt_destroy(mirt_ctx *ctx);

/* Copy the (already built, hence reordered) spheres and the caller's tree to
   the device. The library keeps no pointer into caller memory. */
int mirt_scene_upload(mirt_ctx *ctx, const mirt_sphere *spheres, int num_spheres, const mirt_bvh_node *root);
int mirt_scene_upload_flat(mirt_ctx *ctx, const mirt_sphere *spheres, int num_spheres,
                           const mirt_node *nodes, int num_nodes);

/* ------------------------------------------- device: BVH (bit-identical) */

/* mirt_bvh_build_flat on the device of ctx (mirt 0.7): same tree, same in-place
   reordering of spheres[start,end), bit for bit. *out_nodes is malloc'd
   (mirt_bvh_free_flat). Needs no uploaded scene and leaves an uploaded one
   alone. Blocking; the scratch it needs stays with the ctx until mirt_destroy.
   Arguments are checked as mirt_bvh_build_flat checks them; a NULL ctx is
   MIRT_E_INVALID before any HIP call, a HIP failure MIRT_E_DEVICE.
   Declined inputs: the kernels combine boxes in no fixed order, which gives the
   host's bits only where min/max are exact and symmetric. A range holding a NaN
   or infinite centre or radius, a sphere whose box fl(c - r), fl(c + r) has a
   coordinate equal to -0.0 (fmin(-0, +0) depends on operand order), or a
   negative radius (its box is inverted: c - r > c + r, and the kernels' bins
   need split planes that increase) is detected by the first pass; the host builder then runs on the untouched
   input (mirt_build_stats.on_device = 0), so the result is the same either way. */
int mirt_bvh_build_flat_device(mirt_ctx *ctx, mirt_sphere *spheres, int start, int end, int depth,
                               mirt_node **out_nodes, int *out_count);

typedef struct mirt_build_stats {
    int32_t on_device;   /* 1: built by the kernels; 0: input declined, host builder ran */
    int32_t levels;      /* tree levels processed (0 when on_device == 0) */
    int32_t nodes;
    float   device_ms;   /* HIP-event time of the build's kernels (0 when on_device == 0) */
    float   total_ms;    /* call to return, host clock: H2D + kernels + D2H */
} mirt_build_stats;
/* Of the ctx's last finished mirt_bvh_build_flat_device (MIRT_E_INVALID: none). */
int mirt_last_build_stats(mirt_ctx *ctx, mirt_build_stats *out);

/* The finish of the device build (MIRT_OPT_BUILD_FINISH): the build runs level
   by level, round 0 at `depth`, until a round's open (inner) nodes all hold at
   most F spheres; one wave per open node then builds that node's whole subtree.
   `levels` of mirt_build_stats and mirt_scene_build_stats counts the rounds run
   level by level: round + 1 when the finish ran. */
typedef struct mirt_build_finish_stats {
    int32_t range;      /* F in effect for the build (0: finish off) */
    int32_t round;      /* host-loop round at which the finish took over; -1: it did not run */
    int32_t subtrees;   /* open inner nodes handed to it */
    int32_t nodes;      /* tree nodes it wrote (roots included) */
    int32_t moved;      /* spheres pass B would have moved: always 0 */
    float   finish_ms;  /* HIP-event time of the finish passes */
} mirt_build_finish_stats;
/* Of the ctx's last finished device build, whichever entry point ran it
   (mirt_bvh_build_flat_device, mirt_scene_build_device, the rebuild of
   mirt_scene_update_device[_ptr]); a declined input reports round -1.
   MIRT_E_INVALID, before any HIP call: NULL ctx or out, or no build has run. */
int mirt_last_build_finish(mirt_ctx *ctx, mirt_build_finish_stats *out);

/* ------------------------------ device: spheres in, scene resident (mirt 0.8) */

/* Build and lay out a scene on the device of ctx in one call: the tree of
   spheres[start, end) from `depth` is built by the kernels of
   mirt_bvh_build_flat_device, the device layouts (csrc/layout.h) are derived
   from it by kernels (csrc/scene_device.hip), byte for byte what
   mirt_scene_upload_flat derives on the host, and the scene -- all num_spheres
   spheres in reordered order, plus the sentinel -- is installed in the ctx. The
   tree never leaves the device. Afterwards the ctx is as if
   mirt_bvh_build_flat(copy, start, end, depth, ...) and
   mirt_scene_upload_flat(ctx, copy, num_spheres, ...) had run. `spheres` is
   not written; `reordered` (may be NULL) receives the num_spheres spheres as
   reordered, which a caller needs to interpret mirt_hit.sphere. Frames already
   enqueued on the ctx finish first. Inputs the device build declines (see
   mirt_bvh_build_flat_device) take the host build and the host upload: the
   result is the same (mirt_scene_build_stats.on_device = 0). Arguments are
   checked as mirt_bvh_build_flat_device checks them, plus end <= num_spheres;
   MIRT_E_INVALID comes before any HIP call. */
int mirt_scene_build_device(mirt_ctx *ctx, const mirt_sphere *spheres, int num_spheres, int start, int end,
                            int depth, mirt_sphere *reordered);
/* mirt_scene_upload_flat with the layouts derived on the device: same
   contract, same host-side check of the tree, but only the raw spheres and
   nodes cross the link (a tree from mirt_bvh_build_flat_cached, say). */
int mirt_scene_upload_flat_device(mirt_ctx *ctx, const mirt_sphere *spheres, int num_spheres,
                                  const mirt_node *nodes, int num_nodes);

typedef struct mirt_scene_build_stats {
    int32_t on_device;   /* 1: built and laid out by the kernels; 0: input declined, host build + host upload */
    int32_t levels;      /* tree levels the build processed (0 when on_device == 0) */
    int32_t nodes;
    float   build_ms;    /* HIP-event time of the build's kernels (0 when on_device == 0) */
    float   layout_ms;   /* host clock over the layout kernels, their read-backs and allocations (0 likewise) */
    float   total_ms;    /* call to return, host clock */
} mirt_scene_build_stats;
/* Of the ctx's last finished mirt_scene_build_device (MIRT_E_INVALID: none). */
int mirt_last_scene_build_stats(mirt_ctx *ctx, mirt_scene_build_stats *out);

/* ------------------------------------------ refit: the spheres have moved */

/* Refit nodes[0, num_nodes) in place to `spheres`, which are in the scene's
   order (the reordered order the build returned): sphere and skip of every
   node stay, every box is recomputed bottom-up. `end` is one past the last
   sphere the tree was built over (mirt_bvh_build_flat's end).
     hit-able leaf  a leaf without MIRT_NODE_EMPTY whose sphere < num_spheres.
                    Every other leaf is dead and keeps all its bytes.
     precondition   the hit-able leaves' spheres s_0 < s_1 < ... < s_{k-1}
                    increase strictly in pre-order and s_{k-1} < end <=
                    num_spheres (no hit-able leaf: 0 <= end <= num_spheres).
     leaf box       leaf j's range is [s_j, s_{j+1}), the last leaf's
                    [s_{k-1}, end) -- the builder's own ranges. Its box is the
                    empty box (+inf / -inf) folded with fl(c - r), fl(c + r) of
                    the range's spheres in index order (bvh.c:120-125).
     inner box      fmin / fmax of the boxes of children i + 1 and skip(i + 1);
                    a dead leaf contributes the empty box.
   For a tree the builder made and unchanged spheres the result is the input,
   bit for bit. What a refit is NOT: the tree the reference would build for the
   moved spheres -- it would choose new SAH planes. Frames of a refit scene are
   exactly hit.c:91-109 on the refit tree (ties, leaf gates), not the
   reference's frame of a rebuilt scene, and the tree's SAH quality decays as
   the spheres travel: mirt_bvh_quality_flat / mirt_scene_quality measure by
   how much, and mirt_scene_update_device refits or rebuilds by that measure.
   The tree is checked as by mirt_bvh_validate_flat, then the precondition;
   MIRT_E_INVALID leaves `nodes` untouched and mirt_last_error names the first
   offending node. num_nodes == 0 is MIRT_OK. Never touches the GPU. */
int mirt_bvh_refit_flat(mirt_node *nodes, int num_nodes, const mirt_sphere *spheres, int num_spheres, int end);

/* Refit the ctx's resident scene to `spheres` (host memory, the scene's order,
   as many as the resident scene holds) on the device: as if
   mirt_bvh_refit_flat had run on the resident tree and mirt_scene_upload_flat
   on its result -- byte for byte the same resident arrays and
   mirt_scene_layout_info. Kernels (csrc/refit_device.hip) recompute the boxes
   from the resident 32-B tree into a scratch tree: the leaf boxes, then the
   inner boxes one launch per depth, deepest first. The device layouts are then
   derived again by the kernels of mirt_scene_build_device -- they cannot be
   patched in place: the four-wide layout splits the slot of largest area, so
   its slot references move with the boxes -- and the new scene is installed.
   Frames already enqueued finish on the old scene; a failure leaves the old
   scene installed (for a declined input, whose last step is
   mirt_scene_upload_flat itself, a failure up to that call does); the
   accumulation buffer is the caller's to restart, as after an upload. `out_nodes` (may be NULL) receives the refit tree, the
   resident scene's num_nodes nodes. A resident scene without a tree just gets
   its spheres replaced.
   Declined inputs (mirt_refit_stats.on_device = 0) take the resident tree to
   the host, mirt_bvh_refit_flat and mirt_scene_upload_flat, with the same
   result: a NaN or infinite centre or radius in [s_0, end); a sphere box
   coordinate equal to -0.0 or a negative radius (see
   mirt_bvh_build_flat_device); a resident scene whose `ordered` flag is 0 -- the host refit then decides: a tree that is
   monotone but deeper than 62 levels is refit there, one that is not monotone
   is MIRT_E_INVALID.
   MIRT_E_NOSCENE without a resident scene; MIRT_E_INVALID if num_spheres is
   not the resident scene's or end is out of range. A NULL ctx or bad
   arguments are MIRT_E_INVALID before any HIP call. */
int mirt_scene_refit_device(mirt_ctx *ctx, const mirt_sphere *spheres, int num_spheres, int end,
                            mirt_node *out_nodes);
/* The same with the spheres already on the ctx's device: d_spheres points at
   num_spheres 20-byte spheres in device memory, read on the ctx's stream (a
   caller that animates on the GPU). */
int mirt_scene_refit_device_ptr(mirt_ctx *ctx, const void *d_spheres, int num_spheres, int end,
                                mirt_node *out_nodes);

typedef struct mirt_refit_stats {
    int32_t on_device;   /* 1: refit and laid out by the kernels; 0: input declined, host refit + host upload */
    int32_t nodes;
    float   refit_ms;    /* host clock over the sphere copy and the refit kernels (0 when on_device == 0) */
    float   layout_ms;   /* host clock over the layout kernels, their read-backs and allocations (0 likewise) */
    float   total_ms;    /* call to return, host clock */
} mirt_refit_stats;
/* Of the ctx's last finished mirt_scene_refit_device[_ptr] (MIRT_E_INVALID: none). */
int mirt_last_refit_stats(mirt_ctx *ctx, mirt_refit_stats *out);

/* ------------------------- quality: has the refit tree decayed? */

/* The SAH quality of a flat tree: the area of its inner nodes per unit of area
   of its hit-able leaves (a leaf without MIRT_NODE_EMPTY whose sphere <
   num_spheres; every other leaf is dead, contributes nothing and is counted in
   dead_leaves).
     area(i)   2 (dx dy + dy dz + dz dx) of node i's box in fp32, the builder's
               own box area (bvh.c:48-57), operation for operation.
     overhead  sum area(inner nodes) / sum area(hit-able leaves); +inf when the
               leaf sum is 0 and the inner sum is not, 0 when both are.
     cost      0.125 * overhead + 1, the builder's constants (bvh.c:96).
   In a builder tree a hit-able leaf's box is its sphere's own box, so the leaf
   sum is the same for a refit tree and for any rebuild of the same spheres:
   cost / (cost when the tree was built) says how far the refit tree has
   decayed. It is 1.000 under translation, uniform scaling and (to 0.5 %)
   rotation, and tracked the cost ratio of refit to rebuilt tree within 6 % for
   diffusing spheres on the host (10k spheres). The cost normalised by the
   root's area does not: it FALLS when diffusing spheres grow the root.
   The sums are exact and independent of the order of addition: with A0 =
   area(0) and e = ilogb(A0) + 1, a term is trunc((double)area(i) * 2^(48 - e))
   as a uint64; a term that is not >= 0 counts as 0, one above A0 as 2^48
   (both counted in `clamped`: the boxes do not nest); the terms' halves
   t >> 24 and t & 0xffffff are added apart in uint64 and a sum is
   ldexp((double)hi * 2^24 + (double)lo, e - 48). The host and the device
   (mirt_scene_quality) therefore return the same bytes. */
typedef struct mirt_tree_quality {
    double  inner_area, leaf_area;   /* the two sums, in the tree's own units */
    double  overhead, cost;          /* inner_area / leaf_area; 0.125 * overhead + 1 */
    float   root_area;
    int32_t inner_nodes, leaves, dead_leaves;  /* leaves: hit-able ones */
    int32_t clamped;                 /* terms outside [0, root_area] */
    int32_t degenerate;              /* 1: root_area is not a positive finite float; sums, overhead, cost and
                                        clamped are 0 */
} mirt_tree_quality;
/* The tree is checked as by mirt_bvh_validate_flat (MIRT_E_INVALID);
   num_nodes == 0 is MIRT_OK with *out all zero. Never touches the GPU. */
int mirt_bvh_quality_flat(const mirt_node *nodes, int num_nodes, int num_spheres, mirt_tree_quality *out);
/* The same of the ctx's resident tree, whichever call installed it and whether
   or not it admits ordered walks, by a kernel (csrc/quality_device.hip): one
   thread per node, one read-back. A scene without a tree gives all zeros.
   MIRT_E_NOSCENE without a scene; a NULL ctx or out is MIRT_E_INVALID before
   any HIP call. Blocking. */
int mirt_scene_quality(mirt_ctx *ctx, mirt_tree_quality *out);

/* Refit the resident scene to `spheres` (the scene's order, as for
   mirt_scene_refit_device), measure the refit tree, and rebuild instead when
   it has decayed past max_decay:
     base    the cost of the tree the ctx's last mirt_scene_update_device
             installed. Every other install (upload, build, plain refit) leaves
             the ctx without one; this call then measures the resident tree
             first and takes its cost.
     decay   cost of the refit tree / base; 1 when either is not a positive
             finite number.
     decay <= max_decay, or max_decay <= 0 (never rebuild): the refit tree is
             installed, exactly what mirt_scene_refit_device installs. The base
             stays, `reordered` is a copy of `spheres`, `perm` the identity.
     else    the tree of spheres[start, end) is built from depth 0 and installed,
             exactly what mirt_scene_build_device installs; its cost is the new
             base. reordered[i] is spheres[perm[i]]: perm is what the colour
             words hold after mirt_bvh_build_flat ran on a copy whose colour
             words were replaced by the spheres' indices, so a caller can carry
             its own per-sphere state through the rebuild.
   reordered and perm (num_spheres each) and out may be NULL. Inputs that
   mirt_scene_refit_device or the device build decline take the host path --
   mirt_bvh_refit_flat, mirt_bvh_quality_flat, then mirt_scene_upload_flat of
   the refit tree or of mirt_bvh_build_flat's -- with the same result and
   on_device = 0. Arguments are checked as mirt_scene_refit_device checks them,
   plus 0 <= start <= end. A failure leaves the old scene and the old base in
   place (on the host path: a failure up to mirt_scene_upload_flat does);
   frames already enqueued finish on the old scene. Blocking. What max_decay
   to choose: decay follows the SAH cost, and frame time grows faster than
   that -- measured on an MI355X at 1080p / 10k spheres, a refit scene at
   decay 1.04 / 1.25 / 2.8 rendered 1.12 / 1.64 / 5.8 times as long as a
   rebuild of the same spheres (MEASUREMENTS.md section E). */
typedef struct mirt_update_result {
    int32_t rebuilt;      /* 1: the scene was rebuilt; 0: refit */
    int32_t on_device;    /* 0: a declined input took the host path */
    double  base_cost, cost, decay;   /* cost is the refit tree's, measured before the decision */
    mirt_tree_quality installed;      /* of the tree now resident */
    float   total_ms;     /* call to return, host clock */
} mirt_update_result;
int mirt_scene_update_device(mirt_ctx *ctx, const mirt_sphere *spheres, int num_spheres, int start, int end,
                             double max_decay, mirt_sphere *reordered, int32_t *perm, mirt_update_result *out);
/* The same with the spheres read from device memory on the ctx's stream (not
   written), and `reordered` and `perm` (either may be NULL) written to device
   memory: for a caller that animates on the GPU. The decision, the resident
   arrays, the base cost rule and *out are mirt_scene_update_device's. On the
   paths the kernels accept no sphere, colour or permutation crosses the host
   link; declined inputs are fetched, take the host path and have reordered
   and perm uploaded. d_reordered == d_spheres is MIRT_E_INVALID. Blocking. */
int mirt_scene_update_device_ptr(mirt_ctx *ctx, const void *d_spheres, int num_spheres, int start, int end,
                                 double max_decay, void *d_reordered, int32_t *d_perm, mirt_update_result *out);

/* ---------------------------------------------------------- rendering */

/* Number of rows (and the row indices, if rows != NULL) a shard renders.
   Limits of a valid descriptor: width, height >= 1 with width * height *
   samples <= 2^31; max_depth 0..8; samples 0..64; row_block >= 1; 0 <= shard <
   num_shards; lead_skip 0..7, and 0 unless num_shards >= 2; frames >= 1 when
   accumulate is set. Every seed and every sample is valid.
   Empty shards: a valid descriptor may describe a shard without rows -- more
   shards than the image has row blocks (height 9, row_block 8: shards 2.. of
   3), or shard 0 sitting out a low frame under lead_skip. mirt_shard_rows
   returns 0 for it, and every frame call (mirt_render_frame, _device, _async,
   the three mirt_render_frame_planes calls, mirt_count_frame, and the launches
   of mirt_multi, which deals such shards to its ranks by itself) renders it as
   MIRT_OK:
     - nothing is written through the colour, accumulation or plane pointers;
       they are checked as for any other shard (non-NULL where required);
       mirt_count_frame writes all zeros;
     - the ctx's own accumulation buffer is treated as for any other change of
       frame geometry: a pending accumulation ends, the next frame starts one;
     - no kernel is launched, so mirt_last_kernel_ms keeps the value of the
       last frame that had rows;
     - under MIRT_OPT_PRIMARY_CACHE the frame is a BYPASS (SCHEDULE), which
       leaves the cache as it was;
     - the ctx stays usable for the next frame. */
int mirt_shard_rows(const mirt_frame_desc *fd, int32_t *rows);

/* The pixel loop of main.c:356-374 (fresh) / main.c:382-407 (accumulate) for
   the shard described by fd: writes the displayed RGBA8 colour of every pixel
   of the shard's rows, compacted in shard row order, to host memory `out`
   (num_rows * width). Accumulation state lives on the device (per ctx); with
   fd->samples > 1 the frames are accumulated in order and `out` receives the
   display after the last one. */
int mirt_render_frame(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, mirt_rgba8 *out);

/* Same, asynchronously on `stream` (a hipStream_t; NULL = the default stream),
   into device memory: d_out = samples * num_rows * width packed RGBA8 (frame
   j's slab at j * num_rows * width). d_accum is a device float buffer of
   num_rows * width * 3 (may be NULL when fd->accumulate == 0); given with
   samples > 1, the frames are folded into it and slab j receives the display
   after frame j. Given by ctxs that share their accumulation buffer
   (mirt_ctx_share_accum), the folds into d_accum follow call order across
   those ctxs' streams. Inputs are already resident in HBM. The ctx's frame scratch
   (bounce queue, deferral list) is one per ctx: a launch on a different
   stream than the ctx's previous launch first waits for that launch (an
   event), so frames of one ctx never overlap; use one ctx per stream for
   frames in flight. */
int mirt_render_frame_device(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd,
                             uint32_t *d_out, float *d_accum, void *stream);

/* Frames in flight to host memory (SURVEY §8(d) t_frame: call -> RGBA8 on
   the host). mirt_render_frame_async enqueues what mirt_render_frame does --
   the frame's kernels and the D2H copy of its display into `out` -- on the
   ctx's own stream and returns at once; `out` holds the frame once
   mirt_ctx_wait(ctx) returns (or after the next blocking call on the ctx).
   `out` should be page-locked memory from mirt_host_alloc: then the copy is a
   DMA that overlaps the next frame's kernels on another ctx; pageable memory
   works too but the runtime stages it. Rotating two or three ctxs (each with
   the scene uploaded) keeps the GPU busy while earlier frames drain and
   copy: for frame k use ctx k % n, mirt_ctx_wait it first (its buffer from
   frame k - n is then complete), then mirt_render_frame_async. For the
   accumulating loop (main.c:379-408) the rotated ctxs must share ONE
   accumulation buffer: mirt_ctx_share_accum(ctx[i], ctx[0]). */
int mirt_render_frame_async(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, mirt_rgba8 *out);
/* Block until every call enqueued on the ctx's stream has finished. */
int mirt_ctx_wait(mirt_ctx *ctx);
/* Page-locked host memory (hipHostMalloc) for frame outputs; mirt_host_free
   releases it (NULL is ignored). */
int mirt_host_alloc(size_t bytes, void **out);
void mirt_host_free(void *p);
/* Page-lock a caller-owned buffer in place (hipHostRegister) -- the frame
   buffer main.c:241-273's loop mallocs once and reuses every frame: the
   blocking mirt_render_frame's D2H into it is then one DMA instead of the
   runtime's staged pageable copy -- or none at all: with MIRT_OPT_ZERO_COPY
   (default) the frame kernels write the pixels straight into it. The
   registration pins the pages until mirt_host_unregister, which must come
   before the buffer is freed. */
int mirt_host_register(void *p, size_t bytes);
int mirt_host_unregister(void *p);

/* A frame that also returns each pixel's primary hit: the closest hit of the
   camera ray the frame traces for that pixel (with fd's jitter, sample and
   shard), found by the walk the frame uses (fd->use_bvh: ray_bvh_intersect on
   the resident tree, else the brute-force loop). Each plane is indexed exactly
   as the colour output of the device form: `samples` slabs of num_rows * width,
   pixel r * width + x in shard row order; slab j holds frame j's own hit (planes
   are never accumulated). Element i is, byte for byte, the t, sphere and normal
   of mirt_intersect_rays(mirt_camera_rays(fd))[i]. Sphere indices refer to the
   scene that was resident when the frame was enqueued (mirt_ctx_scene_id; the
   group's scene for members of a scene group). */
typedef struct mirt_primary_planes {
    float   *t;       /* HitRecord.t (hit.c:19-39) of the camera ray's closest hit; 0 on a miss      */
    int32_t *sphere;  /* index into the resident (reordered) spheres; -1 on a miss                    */
    float   *normal;  /* 3 floats per pixel, hit.c:32-33's normal; 0,0,0 on a miss                    */
} mirt_primary_planes; /* a NULL member is not written; at least one must be non-NULL */

/* mirt_render_frame / _device / _async with planes: the same arguments, checks
   and errors, the same colours and accumulation buffer byte for byte, and in
   addition MIRT_E_INVALID (before any device call) for a NULL ctx, NULL planes,
   planes without a member, or fd->max_depth < 1. The hit is stored by the
   frame's own camera walk, not by a second one. The blocking and async forms
   take host pointers (samples * num_rows * width elements each; `out` still
   receives the last display only) and copy the planes behind the frame on the
   ctx's stream from device memory the ctx keeps; the device form takes device
   pointers. */
int mirt_render_frame_planes(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, mirt_rgba8 *out,
                             const mirt_primary_planes *planes);
int mirt_render_frame_planes_device(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd,
                                    uint32_t *d_out, float *d_accum, const mirt_primary_planes *d_planes,
                                    void *stream);
int mirt_render_frame_planes_async(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, mirt_rgba8 *out,
                                   const mirt_primary_planes *planes);

/* Ray frames: a frame whose camera rays the caller gives -- a thin lens, a
   fisheye, an orthographic or stereo camera, a lens-distortion table, its own
   anti-aliasing pattern. A ray frame is a frame in every respect (fd's
   geometry, shard, row_block, lead_skip, samples, max_depth, use_bvh, seed,
   sample, accumulate, frames; the ctx's buffers, mirt_ctx_share_accum chains
   and the folds of samples > 1; every schedule of mirt_set_option) except that
   pixel i's camera ray is rays[i]. `rays` is indexed exactly as the colour
   output of the device form and as the planes are: `samples` slabs of
   num_rows * width, element r * width + x in shard row order, slab j holding
   frame j's rays (so the lens can be re-sampled per frame); indices are
   computed in size_t. Rays are used as given -- direction not normalised, any
   origin -- the contract of mirt_trace_rays. The pixel's RNG stream is the
   frame's (seed, pixel y * width + x of image row y, sample + j), hence:
     a ray frame fed mirt_camera_rays(fd) is mirt_render_frame(cam, fd) byte
       for byte;
     for any rays, an unsharded one-sample ray frame is mirt_trace_rays(rays,
       width * height, max_depth, use_bvh, seed, sample), and a shard's row y
       is mirt_trace_rays_at(..., pixel0 = y * width);
     with planes, element i is the t, sphere and normal of
       mirt_intersect_rays(rays)[i].
   Checks, errors and accumulation are those of mirt_render_frame_device /
   mirt_render_frame; in addition MIRT_E_INVALID, before any device call, for
   a NULL ctx, NULL rays, an invalid fd, fd->jitter != 0 (the caller owns the
   sample points), a planes struct without a member, or planes with
   fd->max_depth < 1. An empty shard is MIRT_OK, launches nothing and reads and
   writes nothing. On the default schedule (use_bvh) the camera pass walks one
   ray per lane, as mirt_intersect_rays does, and hands the first bounces to the
   bounce pass of a plain frame. With MIRT_OPT_PRIMARY_CACHE 1 a ray frame is a
   BYPASS (reason MIRT_PCACHE_RAYS) and leaves a valid cache valid.
   _device: rays in device memory (24-byte mirt_ray), read on `stream`; d_planes
   may be NULL. The blocking form takes host pointers: the rays are copied to a
   buffer the ctx keeps (grown like its other buffers), `out` receives the last
   display as mirt_render_frame's does, planes may be NULL. */
int mirt_render_rays_device(mirt_ctx *ctx, const mirt_ray *d_rays, const mirt_frame_desc *fd, uint32_t *d_out,
                            float *d_accum, const mirt_primary_planes *d_planes, void *stream);
int mirt_render_rays(mirt_ctx *ctx, const mirt_ray *rays, const mirt_frame_desc *fd, mirt_rgba8 *out,
                     const mirt_primary_planes *planes);

/* Lens frames: depth of field computed in the frame's own camera pass. Each
   pixel's thin-lens ray is made in the kernel from the pinhole's ray and the
   pixel's RNG contract stream, so no ray buffer exists anywhere and a lens
   frame is a frame in every respect: accumulation, shards, samples, planes, a
   stream, every schedule, frames in flight (_async) and mirt_multi
   (mirt_multi_render_lens_frames_async, mirt_multi.h). The lens is re-sampled
   with fd->sample, as the accumulating loop (main.c:379-408) needs.
   The definition (csrc/lens.h; every operation one correctly rounded binary32
   operation, in this order), for pixel (x, y) of RNG sample s:
     key = the frame's own key of (seed, y * width + x, s);
     (p, d) = the pinhole's ray of that pixel and sample, with fd->jitter's
       displacement when set (a lens frame MAY be jittered);
     (a, b) = a point of the unit disc by rejection: try i = 0 .. 15 takes
       a = (float)draw(key, 0x7fffff00 + 2i) / 2^31 * 2 - 1 and b likewise from
       draw 0x7fffff00 + 2i + 1; the first try with a * a + b * b < 1 is
       accepted, and a = b = 0 if none is. The bounce sampling's draws still
       start at 0;
     origin = (p + L * a) + U * b with L = cam->right * aperture and
       U = cam->up * aperture;
     direction = normalised ((p + d * focus) - origin), zero for a zero length.
   Hence mirt_render_lens_frame(cam, lens, fd) is, byte for byte,
   mirt_render_rays(mirt_lens_rays(cam, lens, fd), fd with jitter cleared), and
   with planes element i is mirt_intersect_rays(mirt_lens_rays(...))[i].
   aperture == 0 is the pinhole by definition: every form forwards to its plain
   counterpart (mirt_render_frame[_planes] / _device / _async,
   mirt_camera_rays), and the primary cache sees a plain frame. With
   aperture > 0 and MIRT_OPT_PRIMARY_CACHE 1 a lens frame is a BYPASS (reason
   MIRT_PCACHE_LENS) and leaves a valid cache valid.
   Checks, errors, accumulation, mirt_ctx_share_accum chains, the folds of
   samples > 1, empty shards and MIRT_OPT_ZERO_COPY are those of the plain call
   of the same form; in addition MIRT_E_INVALID, before any device call, for a
   NULL ctx, cam, lens or fd, an invalid lens (aperture not finite or < 0,
   focus not finite or <= 0), a planes struct without a member, or planes with
   fd->max_depth < 1. planes / d_planes may be NULL.
   mirt_lens_rays writes the rays a lens frame traces, indexed as its colour
   output (`samples` slabs of num_rows * width; slab j is sample + j). */
typedef struct mirt_lens {
    float aperture;  /* lens radius in world units; 0 = the pinhole */
    float focus;     /* distance along the normalised pinhole ray at which the pixel is sharp */
} mirt_lens;
int mirt_lens_rays(mirt_ctx *ctx, const mirt_camera *cam, const mirt_lens *lens, const mirt_frame_desc *fd,
                   mirt_ray *out);
int mirt_render_lens_frame(mirt_ctx *ctx, const mirt_camera *cam, const mirt_lens *lens, const mirt_frame_desc *fd,
                           mirt_rgba8 *out, const mirt_primary_planes *planes);
int mirt_render_lens_frame_device(mirt_ctx *ctx, const mirt_camera *cam, const mirt_lens *lens,
                                  const mirt_frame_desc *fd, uint32_t *d_out, float *d_accum,
                                  const mirt_primary_planes *d_planes, void *stream);
int mirt_render_lens_frame_async(mirt_ctx *ctx, const mirt_camera *cam, const mirt_lens *lens,
                                 const mirt_frame_desc *fd, mirt_rgba8 *out, const mirt_primary_planes *planes);

/* Denoising a frame where it lies: an edge-avoiding a-trous filter guided by
   the frame's primary-hit planes (mirt_primary_planes' sphere and normal). A
   one-sample frame is noisy -- each hit adds half of one random bounce chain
   (renderer.c:51-58) -- and the accumulating loop (main.c:379-408) needs many
   frames of a still camera; the filter averages a pixel with its neighbours on
   the same sphere and of like normal, in device memory, on the frame's stream.
   The definition (csrc/denoise.h; every operation one correctly rounded
   binary32 operation, in this order), for an image of width x height pixels,
   row-major, pixel i = y * width + x:
     colour source, exactly one of: rgba, packed RGBA8 as a frame's display,
       c[ch] = (float)u8 / 255.0f (main.c:368-370); or accum, float3 sums as
       the accumulation buffer holds them, with a divisor frames >= 1,
       c[ch] = a[ch] / (float)frames;
     guides: sphere (int32 per pixel, < 0 on a miss; required) and normal
       (three floats per pixel; may be NULL);
     pass i = 0 .. passes - 1 has tap spacing s = 2^i, reads the colours of the
       pass before it (pass 0: the source) and writes a new image. For pixel
       p = (x, y) the taps q = (x + dx s, y + dy s) are visited dy = -2 .. 2
       outermost, dx = -2 .. 2 innermost. A tap outside the image, or with
       sphere[q] != sphere[p], contributes nothing (two misses are equal).
       Else w = B[dy + 2] * B[dx + 2], B = {1/16, 1/4, 3/8, 1/4, 1/16}; the
       centre tap keeps exactly that (9/64: the weight sum is never zero);
       every other tap, with a normal plane and sphere[p] >= 0:
         d = nx_p nx_q; d = d + ny_p ny_q; d = d + nz_p nz_q; m = fmaxf(d, 0);
         m = m * m, normal_sharpness times; w = w * m
       and with sigma_colour > 0:
         e = c_p - c_q per channel, of this pass's input;
         g = er er; g = g + eg eg; g = g + eb eb;
         w = w * (1.0f / (1.0f + g * inv_i)),
         inv_0 = 1.0f / (sigma_colour * sigma_colour), inv_{i+1} = inv_i * 4.0f.
       sw = sw + w and sc[ch] = sc[ch] + c_q[ch] * w in visiting order from
       +0.0f; the pass's colour is sc[ch] / sw;
     after the last pass out_rgb (may be NULL) receives the three floats per
       pixel and out (may be NULL; not both) the RGBA8
       (uint8_t)(int)fminf(c * 255.0f, 255.0f) per channel (main.c:398-400's
       cast), alpha 255.
   Non-finite colours or normals give unspecified values, never an access
   outside the image or the scratch.
   MIRT_E_INVALID, before any device call: NULL ctx (not mirt_denoise_host),
   params or sphere plane; both or neither colour source; frames < 1 with
   accum; no output; width or height < 1, or width * height beyond 2^31 (the
   frame descriptor's limit); passes outside 1..5; normal_sharpness outside
   0..7; sigma_colour negative or not finite.
   mirt_denoise_host: the filter on the host (no device call, no ctx).
   mirt_denoise_device: everything in device memory; enqueued on `stream`
   (NULL: the default stream), returns without waiting; byte for byte the host
   form's result. The ping-pong images are scratch the ctx keeps (grown like
   its other buffers, released by mirt_destroy); a launch on another stream
   than the ctx's previous launch first waits for that one (an event), as
   frames do. d_out may alias d_rgba.
   mirt_denoise: blocking, host pointers: copies in, filters on the ctx's
   stream, copies out.
   mirt_render_frame_denoised: blocking; renders exactly what
   mirt_render_frame_planes (lens NULL or aperture 0) or mirt_render_lens_frame
   renders -- colours and accumulation buffer byte for byte the plain call's,
   the sphere and normal planes into buffers the ctx keeps -- then filters
   fd->accumulate ? the accumulation buffer after the last fold, with that
   frame's divisor : the last slab's display. `out` receives the filtered
   display, `raw` (may be NULL) the display mirt_render_frame would return.
   The accumulation buffer is not touched, so the loop of main.c:379-408
   continues unbiased. In addition MIRT_E_INVALID, before any device call, for
   a NULL cam, fd or out, an invalid fd or lens, fd->num_shards != 1,
   fd->max_depth < 1, or a ctx in a mirt_ctx_share_accum chain. Under
   MIRT_OPT_PRIMARY_CACHE the frame is a BYPASS (PLANES; LENS through a lens),
   as any planes frame is: a still camera keeps the first frame's planes and
   calls mirt_denoise_device behind plain cached frames.
   mirt_multi and sharded images are out of scope. */
typedef struct mirt_denoise_params {
    int32_t passes;            /* 1..5; pass i has tap spacing 2^i */
    int32_t normal_sharpness;  /* 0..7: the normals' cosine is squared this many times */
    float sigma_colour;        /* >= 0; 0 = no colour weight */
} mirt_denoise_params;
void mirt_denoise_params_default(mirt_denoise_params *out);   /* 3, 3, 0 */
int mirt_denoise_host(int width, int height, const mirt_rgba8 *rgba, const float *accum, int frames,
                      const int32_t *sphere, const float *normal, const mirt_denoise_params *params,
                      mirt_rgba8 *out, float *out_rgb);
int mirt_denoise_device(mirt_ctx *ctx, int width, int height, const uint32_t *d_rgba, const float *d_accum,
                        int frames, const int32_t *d_sphere, const float *d_normal,
                        const mirt_denoise_params *params, uint32_t *d_out, float *d_out_rgb, void *stream);
int mirt_denoise(mirt_ctx *ctx, int width, int height, const mirt_rgba8 *rgba, const float *accum, int frames,
                 const int32_t *sphere, const float *normal, const mirt_denoise_params *params, mirt_rgba8 *out,
                 float *out_rgb);
int mirt_render_frame_denoised(mirt_ctx *ctx, const mirt_camera *cam, const mirt_lens *lens,
                               const mirt_frame_desc *fd, const mirt_denoise_params *params, mirt_rgba8 *out,
                               mirt_rgba8 *raw);

/* Reprojecting a frame's history when the camera moves. The accumulating loop
   (main.c:379-408) converges only while the camera stands still: every move
   starts over at one sample (main.c:350-377). Here each pixel keeps a record
   of its own -- the mean of n samples -- and a new one-sample frame takes the
   record of the surface it shows from wherever the previous camera saw that
   surface, found by reprojecting the pixel's primary hit point. The definition
   (csrc/reproject.h; every operation one correctly rounded binary32 operation,
   in this order), for an unsharded image of width x height pixels, row-major,
   pixel i = y * width + x:
     cameras: cam, and cam_prev of the previous frame; of each the constants of
       a frame (ray.c:18-24): p, forward, right, up, sw = 2 half_w,
       sh = 2 half_h, hor = right * sw, ver = up * sh, aspect, wf, hf;
     current frame: rgba (a one-sample frame's display), t and sphere
       (mirt_primary_planes); previous frame: hist (mirt_history_px: the mean
       of n samples, n == 0 = none), t_prev, sphere_prev. cam_prev, hist,
       t_prev and sphere_prev are NULL together on the first frame: every
       pixel then takes "no history";
     1 c[ch] = (float)u8 / 255.0f; s = sphere[i]; s < 0: no history;
     2 d = the unjittered pinhole direction of (x, y) under cam (main.c:362-365,
       ray.c:26-31, normalised; zero for a zero length); X = p + d * t[i];
     3 e = X - p_prev; zf = dot(e, forward_prev), left to right;
       !(zf > 0): no history;
     4 a = dot(e, right_prev) / zf; b = dot(e, up_prev) / zf; u = a / sw_prev;
       v = b / sh_prev; xf = (u / aspect + 0.5f) * wf; yf = (0.5f - v) * hf;
     5 l = sqrtf(dot(e, e));
     6 taps == 1: the tap (floorf(xf + 0.5f), floorf(yf + 0.5f)), w = 1;
       taps == 4: gx = floorf(xf), gy = floorf(yf), ax = xf - gx, ay = yf - gy,
       the taps (gx, gy), (gx + 1, gy), (gx, gy + 1), (gx + 1, gy + 1) in this
       order with w = (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay;
     7 a tap (tx, ty), kept as floats, is inside iff tx >= 0 && tx < wf &&
       ty >= 0 && ty < hf, and only then becomes an index: a t of NaN, infinity
       or 1e38 never gives an access outside the image;
     8 an inside tap q is valid iff w > 0, sphere_prev[q] == s, hist[q].n >= 1
       and fabsf(l - t_prev[q]) <= t_tolerance * l;
     9 over the valid taps in order, from +0.0f: sw_ = sw_ + w,
       sc[ch] = sc[ch] + hist[q].c[ch] * w, nmin = min n; none valid: no
       history; else m[ch] = sc[ch] / sw_;
    10 n_new = min(nmin + 1, max_history),
       mean[ch] = m[ch] + (c[ch] - m[ch]) / (float)n_new; no history: n_new = 1,
       mean = c;
    11 hist_out[i] = {mean, n_new} (required; must not be hist); out (may be
       NULL): RGBA8 of mean by the denoiser's cast, alpha 255; out_rgb (may be
       NULL): mean's three floats -- what mirt_denoise_device takes as accum
       with frames = 1.
   MIRT_E_INVALID, before any device call: NULL ctx (not mirt_reproject_host),
   params, cam, rgba, t, sphere or hist_out; some but not all of cam_prev,
   hist, t_prev, sphere_prev; hist_out == hist; width or height < 1 or
   width * height beyond 2^31; max_history outside 1..65536; taps not 1 or 4;
   t_tolerance negative or not finite.
   mirt_reproject_host: on the host (no device call, no ctx).
   mirt_reproject_device: everything in device memory; enqueued on `stream`
   (NULL: the default stream), returns without waiting; byte for byte the host
   form's result. A launch on another stream than the ctx's previous launch
   first waits for that one, as frames and the denoiser do. d_out may alias
   d_rgba.
   mirt_reproject: blocking, host pointers.
   mirt_render_frame_reprojected: the moving-camera loop in one blocking call.
   Renders exactly what mirt_render_frame_planes renders (colours and
   accumulation buffer byte for byte the plain call's), t and sphere into
   buffers the ctx keeps, then reprojects from the ctx's history -- the
   previous call's camera, planes and records -- into the other half of a
   ping-pong pair, which becomes the history. `out` receives the display,
   `raw` (may be NULL) the one-sample display. The history starts empty after
   mirt_history_reset, a change of width or height, a change of
   mirt_ctx_scene_id (every install: sphere indices and positions may have
   changed) and mirt_create. In addition MIRT_E_INVALID, before any device
   call, for a NULL fd or out, an invalid fd, fd->accumulate != 0,
   fd->samples > 1, fd->num_shards != 1, fd->jitter != 0, fd->max_depth < 1, or
   a ctx in a mirt_ctx_share_accum chain. Under MIRT_OPT_PRIMARY_CACHE the
   frame is the BYPASS (PLANES) any planes frame is.
   mirt_history_stats_get: waits for the ctx's stream. mirt_history_read: the
   current records, n = width * height of them (MIRT_E_INVALID without a
   history or for another n).
   Lens and jittered frames (their primary ray is not the pinhole's), shards,
   mirt_multi and frames in flight are out of scope; moving spheres: the
   mirt_reproject_motion forms and MIRT_OPT_HISTORY_MOTION below. */
typedef struct mirt_history_px {
    float r, g, b;   /* the mean of n samples */
    int32_t n;       /* 0 = no history */
} mirt_history_px;   /* 16 B */
typedef struct mirt_reproject_params {
    int32_t max_history;   /* 1..65536: a record's n stops growing here */
    int32_t taps;          /* 1 = the nearest previous pixel, 4 = bilinear */
    float t_tolerance;     /* >= 0: a tap's stored distance may differ by this share of l */
} mirt_reproject_params;
typedef struct mirt_history_stats {
    uint64_t frames;     /* mirt_render_frame_reprojected calls since the history was last empty */
    uint64_t scene_id;   /* mirt_ctx_scene_id of the history (0: none) */
    uint64_t bytes;      /* device memory held for the history */
    uint64_t reused;     /* the last call's pixels with n_new > 1 */
    uint64_t fresh;      /* its hit pixels with n_new == 1 */
    uint64_t sky;        /* its pixels with sphere < 0 */
    int32_t width, height;   /* of the history (0: none) */
} mirt_history_stats;    /* 56 B */
void mirt_reproject_params_default(mirt_reproject_params *out);   /* 64, 4, 1/64 */
int mirt_reproject_host(int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                        const mirt_rgba8 *rgba, const float *t, const int32_t *sphere, const mirt_history_px *hist,
                        const float *t_prev, const int32_t *sphere_prev, const mirt_reproject_params *params,
                        mirt_history_px *hist_out, mirt_rgba8 *out, float *out_rgb);
int mirt_reproject_device(mirt_ctx *ctx, int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                          const uint32_t *d_rgba, const float *d_t, const int32_t *d_sphere,
                          const mirt_history_px *d_hist, const float *d_t_prev, const int32_t *d_sphere_prev,
                          const mirt_reproject_params *params, mirt_history_px *d_hist_out, uint32_t *d_out,
                          float *d_out_rgb, void *stream);
int mirt_reproject(mirt_ctx *ctx, int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                   const mirt_rgba8 *rgba, const float *t, const int32_t *sphere, const mirt_history_px *hist,
                   const float *t_prev, const int32_t *sphere_prev, const mirt_reproject_params *params,
                   mirt_history_px *hist_out, mirt_rgba8 *out, float *out_rgb);
int mirt_render_frame_reprojected(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd,
                                  const mirt_reproject_params *params, mirt_rgba8 *out, mirt_rgba8 *raw);
int mirt_history_reset(mirt_ctx *ctx);
int mirt_history_stats_get(mirt_ctx *ctx, mirt_history_stats *out);
int mirt_history_read(mirt_ctx *ctx, mirt_history_px *hist, size_t n);

/* Reprojecting when the SPHERES moved between the two frames, and a history
   that survives mirt_scene_refit_device / mirt_scene_update_device.
   A motion: geo[num_spheres] is the scene the current frame's `sphere` plane
   indexes, geo_prev[num_prev] the previous frame's scene, each sphere as four
   floats {centre.x, .y, .z, radius} (MIRT_LAYOUT_GEO's first num_spheres
   elements); prev_index[s] is the index in geo_prev of the sphere that is now
   s (NULL: the identity). With a motion steps 2, 3 and 8 above become
   (csrc/reproject.h; one binary32 operation each):
     2  X = p + d * t, as before;
     2a !(0 <= s < num_spheres): no history; sp = prev_index ? prev_index[s]
        : s; !(0 <= sp < num_prev): no history (both compared before either
        value indexes anything);
     2b g = geo[s], gp = geo_prev[sp]; all four floats equal (float ==, a NaN
        is unequal): Xp = X; else k = gp.r / g.r, o = X[j] - g.c[j], o = o * k,
        Xp[j] = gp.c[j] + o -- the same surface point where the sphere was,
        rescaled if its radius changed. A zero or non-finite radius gives a
        non-finite Xp; step 7 keeps every access inside the image;
     3  e = Xp - p_prev; the rest of 3 and 4 - 7 unchanged;
     8  ... sphere_prev[q] == sp (not s) ...
   A motion with geo_prev equal to geo and the identity map is the plain
   reprojection byte for byte.
   mirt_reproject_motion_host / _device / mirt_reproject_motion: the arguments
   and contracts of their plain counterparts (stream ordering, aliasing, the
   MIRT_E_INVALID cases before any device call, _device byte for byte the host
   form) plus `motion`, whose pointers are host pointers for the host and
   blocking forms and device pointers for _device. In addition MIRT_E_INVALID
   for a NULL motion, geo or geo_prev, a count below 1, a NULL prev_index with
   num_prev != num_spheres, and a motion without a previous frame.
   MIRT_OPT_HISTORY_MOTION 1 (mirt_set_option) on the INSTALLING ctx: every path
   of mirt_scene_refit_device[_ptr] and mirt_scene_update_device[_ptr] (the
   host paths of declined inputs included) records a link on the scene slot:
   the ids of the replaced and the installed scene, a device copy of the
   replaced scene's geo array, and on the rebuild branch the permutation, in
   device memory the slot keeps (it only grows, and goes with the slot). Every
   other install -- the uploads, mirt_scene_build_device, any install by a ctx
   with the option at 0 -- clears the link; a failed install leaves scene,
   base cost and link as they were. With the option 1 on the RENDERING ctx,
   mirt_render_frame_reprojected keeps a history whose scene id is the link's
   `from` when the resident scene is the link's `to`, and reprojects that frame
   with the motion {resident geo, the link's geo_prev, the link's map}. In
   every other case (two installs since the last frame, a cleared link,
   another width or height, mirt_history_reset) the history empties as before.
   Option 0 (default): exactly the behaviour without the option, no device
   work added to any install.
   mirt_history_motion_get: the slot's link (ids 0: none; bytes: device memory
   held for links; rebuilt: the link carries a permutation) and carried = this
   ctx's last mirt_render_frame_reprojected used a link. No device call.
   Out of scope: mirt_multi; shards; frames in flight (installs and reprojected
   frames are blocking calls of the group's one host thread); lens and
   jittered frames; composing several installs into one link; clamping the
   history where shading changed because a NEIGHBOUR moved (shadows,
   reflections): those samples are averaged as they are, as view-dependent
   shading already is. */
typedef struct mirt_sphere_motion {
    const float *geo, *geo_prev;
    const int32_t *prev_index;
    int32_t num_spheres, num_prev;
} mirt_sphere_motion;   /* 32 B */
typedef struct mirt_history_motion {
    uint64_t from_scene_id, to_scene_id, bytes;
    int32_t rebuilt, carried;
} mirt_history_motion;   /* 32 B */
int mirt_reproject_motion_host(int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                               const mirt_rgba8 *rgba, const float *t, const int32_t *sphere,
                               const mirt_history_px *hist, const float *t_prev, const int32_t *sphere_prev,
                               const mirt_reproject_params *params, mirt_history_px *hist_out, mirt_rgba8 *out,
                               float *out_rgb, const mirt_sphere_motion *motion);
int mirt_reproject_motion_device(mirt_ctx *ctx, int width, int height, const mirt_camera *cam,
                                 const mirt_camera *cam_prev, const uint32_t *d_rgba, const float *d_t,
                                 const int32_t *d_sphere, const mirt_history_px *d_hist, const float *d_t_prev,
                                 const int32_t *d_sphere_prev, const mirt_reproject_params *params,
                                 mirt_history_px *d_hist_out, uint32_t *d_out, float *d_out_rgb, void *stream,
                                 const mirt_sphere_motion *motion);
int mirt_reproject_motion(mirt_ctx *ctx, int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                          const mirt_rgba8 *rgba, const float *t, const int32_t *sphere, const mirt_history_px *hist,
                          const float *t_prev, const int32_t *sphere_prev, const mirt_reproject_params *params,
                          mirt_history_px *hist_out, mirt_rgba8 *out, float *out_rgb,
                          const mirt_sphere_motion *motion);
int mirt_history_motion_get(mirt_ctx *ctx, mirt_history_motion *out);

/* Filtering a reprojected frame by its own variance (spatio-temporal
   variance-guided filtering). A pixel's noise varies across the image -- a
   sphere facing the sky is calm, one among neighbours is not -- and a record
   of 64 samples needs less help than a pixel disoccluded this frame. The
   history therefore also carries the second moment of luminance, each pixel's
   variance is estimated from it, and that variance sets the luminance weight
   of an a-trous filter and is filtered along with the colour. Every operation
   below is one correctly rounded binary32 operation, in this order
   (csrc/reproject.h, csrc/vfilter.h); lum(c) is L = 0.2126f * c[0];
   L = L + 0.7152f * c[1]; L = L + 0.0722f * c[2].
   MOMENTS. m2, one float per pixel, is the running mean of lum(sample)^2,
   carried exactly as the record's colour is. mirt_reproject_moments_host /
   _device / mirt_reproject_moments take the arguments and contracts of the
   mirt_reproject_motion form of the same kind (stream ordering, d_out
   aliasing d_rgba, every MIRT_E_INVALID case before any device call), except:
   motion may be NULL (the plain reprojection then runs); m2_prev is NULL
   exactly when hist is; m2_out is required and must not be m2_prev. Steps
   1 - 11 of mirt_reproject are unchanged -- hist_out, out and out_rgb are byte
   for byte the plain or the motion form's -- and these join them:
     1' Lc = lum(c); q2 = Lc * Lc;
     9' over the same valid taps in the same order, from +0.0f:
        s2 = s2 + m2_prev[q] * w; then M2 = s2 / sw_;
    10' m2_out[i] = M2 + (q2 - M2) / (float)n_new; no history (sky, first
        frame, behind the camera, no valid tap): m2_out[i] = q2.
   VARIANCE, per pixel p of hist (the colour c = {r, g, b} and n), m2, sphere
   and normal (three floats, may be NULL):
     V1 Lp = lum(c_p). n_p >= min_history: vt = fmaxf(m2_p - Lp * Lp, 0.0f),
        var_p = vt / (float)n_p;
     V2 otherwise (every n_p <= 0 included) over the 7 x 7 window at spacing 1,
        dy = -3 .. 3 outermost, dx = -3 .. 3 innermost, centre included, each
        tap q inside the image with sphere[q] == sphere[p]: k = k + 1.0f,
        S1 = S1 + Lq, S2 = S2 + Lq * Lq, Lq = lum(c_q), all from +0.0f; then
        mu = S1 / k, var_p = fmaxf(S2 / k - mu * mu, 0.0f).
     var_out (may be NULL) receives var_p.
   FILTER. V3: pass i = 0 .. passes - 1 has spacing 2^i; taps, visiting order,
   B, the same-sphere rule, the normal weight and the centre's 9/64 are
   mirt_denoise's. With sigma_lum > 0 every other tap is also weighted by
   luminance, Lp and Lq of this pass's input colours:
        dl = Lp - Lq; g = dl * dl; den = sl2 * var_p; den = den + 1e-6f;
        w = w * (1.0f / (1.0f + g / den)),  sl2 = sigma_lum * sigma_lum
   (computed on the host; not rescaled per pass: the shrinking variance does
   that). sw = sw + w, sc[ch] = sc[ch] + c_q[ch] * w, sv = sv + var_q * (w * w);
   the pass writes the colour sc / sw and the variance sv / (sw * sw).
   V4: out (RGBA8) and out_rgb as mirt_denoise's, at least one required. With
   sigma_lum == 0 the colours are byte for byte mirt_denoise_host's on accum =
   the records' three floats, frames = 1, the same passes and normal_sharpness,
   sigma_colour = 0.
   Non-finite data gives unspecified values, never an access outside the image
   or the scratch.
   mirt_denoise_var_host / _device / mirt_denoise_var have the contracts of
   their mirt_denoise counterparts (the scratch is one allocation the ctx
   keeps, which only grows; MIRT_OPT_DENOISE_TILE picks the passes' kernel,
   either setting gives the same bytes). MIRT_E_INVALID, before any device
   call: NULL ctx (not the host form), params, hist, m2 or sphere; no output;
   width or height < 1 or width * height beyond 2^31; passes outside 1..5;
   normal_sharpness outside 0..7; sigma_lum negative or not finite;
   min_history outside 1..65536.
   mirt_render_frame_reprojected_denoised: the loop in one blocking call. It
   does everything mirt_render_frame_reprojected does -- the same checks (plus
   MIRT_E_INVALID for invalid var params), the history emptied by the same
   rules, MIRT_OPT_HISTORY_MOTION links honoured (through the moments form with
   the link's motion), the PLANES bypass of the primary cache, colours and
   accumulation buffer byte for byte the plain call's -- and also stores the
   frame's normal plane and carries m2 with the records, in a ping-pong pair
   the ctx keeps; then mirt_denoise_var runs on the new records. `out` receives
   the filtered display, `reprojected` (may be NULL) what
   mirt_render_frame_reprojected's `out` would have held, `raw` (may be NULL)
   the one-sample display. The filter's output is not fed back: the records
   after the call are the plain reprojected call's. The history is one per
   ctx, and the ctx remembers whether its last reprojected frame carried
   moments: a denoised call on a history without them empties it first; a plain
   mirt_render_frame_reprojected on a history with them proceeds as it always
   did and drops the flag. The m2 pair, the normal plane and the filtered
   display are a separate allocation made by the first denoised call, which
   mirt_history_stats.bytes counts once it exists; a ctx that never makes the
   call allocates exactly what it did.
   mirt_history_moments_read: the current m2 plane, n = width * height floats
   (MIRT_E_INVALID without a history that carries moments, or for another n).
   Out of scope: a 3 x 3 Gaussian prefilter of the variance; feeding the first
   pass back into the history; clamping the history where a neighbour's motion
   changed the shading; shards; mirt_multi; _async and frames in flight; lens
   and jittered frames; 4K. */
typedef struct mirt_denoise_var_params {
    int32_t passes;            /* 1..5; pass i has tap spacing 2^i */
    int32_t normal_sharpness;  /* 0..7 */
    float sigma_lum;           /* >= 0, finite; 0 = no luminance weight */
    int32_t min_history;       /* 1..65536: records of fewer samples take the spatial estimate */
} mirt_denoise_var_params;     /* 16 B */
void mirt_denoise_var_params_default(mirt_denoise_var_params *out);   /* 3, 3, 8, 4 */
int mirt_reproject_moments_host(int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                                const mirt_rgba8 *rgba, const float *t, const int32_t *sphere,
                                const mirt_history_px *hist, const float *t_prev, const int32_t *sphere_prev,
                                const mirt_reproject_params *params, mirt_history_px *hist_out, mirt_rgba8 *out,
                                float *out_rgb, const mirt_sphere_motion *motion, const float *m2_prev,
                                float *m2_out);
int mirt_reproject_moments_device(mirt_ctx *ctx, int width, int height, const mirt_camera *cam,
                                  const mirt_camera *cam_prev, const uint32_t *d_rgba, const float *d_t,
                                  const int32_t *d_sphere, const mirt_history_px *d_hist, const float *d_t_prev,
                                  const int32_t *d_sphere_prev, const mirt_reproject_params *params,
                                  mirt_history_px *d_hist_out, uint32_t *d_out, float *d_out_rgb, void *stream,
                                  const mirt_sphere_motion *motion, const float *d_m2_prev, float *d_m2_out);
int mirt_reproject_moments(mirt_ctx *ctx, int width, int height, const mirt_camera *cam, const mirt_camera *cam_prev,
                           const mirt_rgba8 *rgba, const float *t, const int32_t *sphere, const mirt_history_px *hist,
                           const float *t_prev, const int32_t *sphere_prev, const mirt_reproject_params *params,
                           mirt_history_px *hist_out, mirt_rgba8 *out, float *out_rgb,
                           const mirt_sphere_motion *motion, const float *m2_prev, float *m2_out);
int mirt_denoise_var_host(int width, int height, const mirt_history_px *hist, const float *m2, const int32_t *sphere,
                          const float *normal, const mirt_denoise_var_params *params, mirt_rgba8 *out,
                          float *out_rgb, float *var_out);
int mirt_denoise_var_device(mirt_ctx *ctx, int width, int height, const mirt_history_px *d_hist, const float *d_m2,
                            const int32_t *d_sphere, const float *d_normal, const mirt_denoise_var_params *params,
                            uint32_t *d_out, float *d_out_rgb, float *d_var_out, void *stream);
int mirt_denoise_var(mirt_ctx *ctx, int width, int height, const mirt_history_px *hist, const float *m2,
                     const int32_t *sphere, const float *normal, const mirt_denoise_var_params *params,
                     mirt_rgba8 *out, float *out_rgb, float *var_out);
int mirt_render_frame_reprojected_denoised(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd,
                                           const mirt_reproject_params *params,
                                           const mirt_denoise_var_params *var_params, mirt_rgba8 *out,
                                           mirt_rgba8 *reprojected, mirt_rgba8 *raw);
int mirt_history_moments_read(mirt_ctx *ctx, float *m2, size_t n);

/* Download the ctx's accumulation buffer (row-major float3 of the shard),
   after every fold enqueued into it so far. */
int mirt_accum_download(mirt_ctx *ctx, float *out, size_t count);

/* Frames in flight of ONE accumulating display loop (main.c:379-408) on
   several ctxs: ctx uses owner's accumulation buffer from now on (owner NULL
   or ctx itself: a private buffer again). Each frame's colours then go to
   the ctx's own slab and a fold kernel adds them to the shared buffer; the
   folds run in call order across the ctxs' streams (events), the tracing
   still overlaps. Without it every ctx accumulates only its own frames, so a
   rotation of n ctxs would average 1/n of the frames. Both ctxs must be on
   the same device; waits for ctx's enqueued frames first. Ctxs that share a
   buffer must be driven from ONE host thread (the call order is the fold
   order). */
int mirt_ctx_share_accum(mirt_ctx *ctx, mirt_ctx *owner);

/* A moving scene under frames in flight: several ctxs of one device render ONE
   resident scene. A ctx renders the scene in its scene slot, by default a slot
   of its own. After mirt_ctx_share_scene(ctx, owner), ctx uses owner's slot;
   the two, and whoever else shares it, form a group. owner NULL or ctx itself:
   ctx gets a private slot again, which still holds the scene the group had at
   that moment -- the arrays stay shared, and read-only, until either slot's
   next install. Both ctxs must be on the same device (else MIRT_E_INVALID); a
   NULL ctx is MIRT_E_INVALID before any HIP call. Waits for ctx's own enqueued
   frames first, as mirt_ctx_share_accum does.
     Installs are group-wide: mirt_scene_upload, _upload_flat,
       _upload_flat_device, mirt_scene_build_device,
       mirt_scene_refit_device[_ptr] and mirt_scene_update_device[_ptr],
       through any member, install the scene for every member.
     Reads are group-wide: the refit's input tree, mirt_scene_quality,
       mirt_scene_resident_layout, the overlay, the per-ray calls and the
       frames read the group's scene through any member. The base cost of
       mirt_scene_update_device belongs to the slot, not to the ctx.
     Per ctx stay: the options, the statistics (mirt_last_*_stats), the build
       scratch and the frame scratch.
     Frames in flight: a frame enqueued on any member before an install
       renders, to its last pixel, the scene that was resident when it was
       enqueued. No array of a replaced scene is released or rewritten while a
       frame enqueued on a member's stream can still read it: an install
       records an event on the stream of every member that has work in
       flight, and the replaced scene is freed once all have passed (looked
       at by the slot's later installs, and waited for when the slot's last
       member is destroyed).
     Publication: all scene calls are blocking; the new arrays are complete
       before any member can enqueue a frame on them.
     Destroying a member releases its reference: the scene lives as long as
       any member, or any frame in flight, holds it.
   The members of a group must be driven from ONE host thread.
   mirt_ctx_scene_id: a process-wide counter value stamped on a scene when it
   is installed, 0 for "no scene" (and for a NULL ctx). The members of a group,
   and a ctx that left with the scene, report the same id; every install gives
   a new one. */
int mirt_ctx_share_scene(mirt_ctx *ctx, mirt_ctx *owner);
uint64_t mirt_ctx_scene_id(mirt_ctx *ctx);

/* trace_ray (renderer.c:21-77) on n arbitrary rays; ray i uses RNG contract
   pixel index i.
   Rays are used as given -- here, in mirt_intersect_rays, mirt_any_hit_rays and
   mirt_render_rays* alike, and a mirt_camera is not validated either:
   components that are +-inf or NaN, a zero direction, a direction of any
   magnitude and any origin are admitted and give hit.c's and renderer.c's
   result for that ray, on every walk and schedule. That result need not be
   geometry: for |d| near 2^-78, d.d underflows to zero and the reference's tree
   walk records a hit with t = +inf, infinite point components and a NaN
   normal (its brute-force loop, with a strict `<`, records none); the walks
   record the same. hit, sphere, t and colours agree with the reference byte
   for byte; a NaN in point or normal agrees as a NaN, not in sign or payload
   (tests/test_hostile_rays_gpu.py). */
int mirt_trace_rays(mirt_ctx *ctx, const mirt_ray *rays, int n, int depth, int use_bvh,
                    uint64_t seed, uint32_t sample, mirt_rgba8 *out);
/* Same, ray i using RNG contract pixel index pixel0 + i (a caller's own pixel
   loop in chunks: pixel0 = y * width + x of the chunk's first pixel). */
int mirt_trace_rays_at(mirt_ctx *ctx, const mirt_ray *rays, int n, int depth, int use_bvh,
                       uint64_t seed, uint32_t sample, uint32_t pixel0, mirt_rgba8 *out);

/* Closest hit: ray_bvh_intersect (hit.c:91-109) when use_bvh, else the brute
   force loop of renderer.c:36-43. */
int mirt_intersect_rays(mirt_ctx *ctx, const mirt_ray *rays, int n, int use_bvh, mirt_hit *out);

/* benchmark.c:172-255 as batches. Any hit: out[i] = 1 if ray i hits some
   sphere (benchmark_no_bvh's hit_found, benchmark.c:190-199, when use_bvh =
   0; ray_bvh_intersect(...).hit_something, benchmark.c:239-241, when 1).
   Both intersect calls split the brute-force loop over sphere chunks across
   the chip (64-bit atomicMin of (t, index): the first sphere wins ties as in
   renderer.c:39; every sphere is tested, as the reference does). The device
   time of the call's kernels is mirt_last_kernel_ms(). */
int mirt_any_hit_rays(mirt_ctx *ctx, const mirt_ray *rays, int n, int use_bvh, int32_t *out);

/* Element-wise ray_sphere_intersect (hit.c:19-39) / ray_aabb_intersect
   (hit.c:49-82) on pairs; need no scene. */
int mirt_sphere_pairs(mirt_ctx *ctx, const mirt_ray *rays, const mirt_sphere *spheres, int n, mirt_hit *out);
int mirt_aabb_pairs(mirt_ctx *ctx, const mirt_ray *rays, const mirt_aabb *boxes, int n, int32_t *out);

/* The kernels' wave-cooperative bounce sampling on caller-given lanes (test
   probe; needs no scene). Lane i has RNG key keys[i], has consumed k0[i] draws
   and, where need[i] != 0, samples a direction in the hemisphere of
   normals[3i..]: out_dir[3i..] becomes that direction and out_k[i] the draws
   consumed after it. A lane with need[i] == 0 only helps: its out_dir keeps
   what the caller put there and its out_k is k0[i]. n lanes are launched as
   one workgroup of 64 threads (n == 64) or n / 256 workgroups of 256 threads
   (n a multiple of 256); any other n is MIRT_E_INVALID. */
int mirt_hemisphere_probe(mirt_ctx *ctx, const uint64_t *keys, const uint32_t *k0, const float *normals,
                          const int32_t *need, int n, float *out_dir, uint32_t *out_k);

/* Host only, no ctx: the index math the kernels share with the host.
   mirt_coop_geometry: the sampling groups of a wave with num_pending pending
   lanes (1..64) -- *group = the group size g, lane_rank[i] / lane_try[i]
   (64 each) = the rank of the owner lane i serves (>= num_pending: none) and
   the try offset it computes, first_accept[r] (num_pending entries) = the
   lowest try offset owner r's group accepted according to the ballot
   `accepted` (bit i: lane i accepted), -1 if none.
   mirt_pixel_rows: for each shard pixel index p = r * width + x of a launch
   of `samples` frames of shard_rows rows each (row blocks of row_block rows,
   shard `shard` of num_shards, lead_skip 0): out[4i..] = {r, x, the image row
   y of launch row r, r / shard_rows}, by the multiply-high divisions of the
   kernels. */
int mirt_coop_geometry(int num_pending, uint64_t accepted, int32_t *group, int32_t *lane_rank, int32_t *lane_try,
                       int32_t *first_accept);
int mirt_pixel_rows(int width, int shard_rows, int samples, int row_block, int shard, int num_shards,
                    const uint32_t *pixels, int64_t n, int32_t *out);

/* Diagnostic surface (tests; not part of the stable ABI): the walks' FILTERED
   forms of the two tests above on pairs -- the same device functions the
   kernels call, so their error bounds can be checked pair by pair against
   hit.c. The box forms need an uploaded scene: the pruning state comes from its
   largest radius / coordinate and MIRT_OPT_PRUNE as in the walks (none with
   pruning off; the start state for best[i] = +inf; else the state after a hit
   at t = best[i]), the origin bound of the margin-free forms from its boxes.
   mirt_box_form_pairs: out[i] = 1 if `form` passes box i for ray i.
   mirt_sphere_form_pairs: out[i] = the bits of the float the sphere test
   returns for a best hit so far of best[i] (t when the sphere would become
   the closest hit, else -1), from the exact test (fast = 0) or the filtered
   one of the walks (fast = 1). The filtered test takes t from float pairs
   (csrc/exact_t.h) and runs the binary64 expression only for the hit in some
   thousands it cannot certify, so two further values exist for the tests alone,
   compiled into this entry point's kernel only: fast = 2 is the filtered test
   with certification off -- every pair the filter leaves takes the binary64
   branch -- and fast = 3 returns, instead of t, 1 where fast = 1 ran the
   binary64 branch for the pair and 0 elsewhere. */
enum { MIRT_BOX_FORM_SLAB = 0,        /* leaf / node boxes: reciprocal filter, exact when undecided */
       MIRT_BOX_FORM_SLAB_BOX = 1,    /* the same with the pruning test for zero-component rays */
       MIRT_BOX_FORM_CONS = 2,        /* inner boxes: conservative, with margins */
       MIRT_BOX_FORM_CONS_BOUNCE = 3, /* margin-free on grown boxes; a ray whose origin lies beyond the scene's bound C
                                         (or any ray when the scene has none) takes the exact test, as a bounce ray */
       MIRT_BOX_FORM_CONS_CAMERA = 4  /* the same under the camera rays' rule, |o| <= 4C (a frame whose camera lies
                                         beyond it uses MIRT_BOX_FORM_CONS) */ };
int mirt_box_form_pairs(mirt_ctx *ctx, const mirt_ray *rays, const mirt_aabb *boxes, const float *best, int n,
                        int form, int32_t *out);
int mirt_sphere_form_pairs(mirt_ctx *ctx, const mirt_ray *rays, const mirt_sphere *spheres, const float *best,
                           int n, int fast, uint32_t *out);
/* csrc/exact_t.h on the host (needs no ctx and makes no HIP call): for each of
   n triples (b, disc, d2a = 2a of hit.c:22-25, disc > 0) and caller-given seeds
   s ~ sqrt(disc), rs ~ 1/s, rd ~ 1/d2a, th[i] = the float-pair t and
   certified[i] = 1 where it is certified to equal hit.c:28's t (else 0, th[i]
   without meaning). */
int mirt_exact_t_pairs(int64_t n, const float *b, const float *disc, const float *d2a, const float *s,
                       const float *rs, const float *rd, float *th, uint8_t *certified);
/* normalize3's binary32 square root against vec3.c:22's (float)sqrt((double)x)
   on every non-negative finite float, in one launch: the number of bit
   patterns whose results differ (expected 0) and the least of them
   (0xffffffff: none). */
int mirt_sqrt_form_sweep(mirt_ctx *ctx, uint64_t *mismatches, uint32_t *first);
/* The device build's partition kernels on caller-given keys (needs no scene):
   nseg segments [seg[k], seg[k+1]) of centre[0,n) (seg non-decreasing, within
   [0, n]), each partitioned by centre < split[k] as bvh.c:172-201's swap loop
   leaves it; perm[j] = source index of the element that ends at position j
   (j itself outside the segments). */
int mirt_build_partition_probe(mirt_ctx *ctx, const float *centre, int n, const int32_t *seg, int nseg,
                               const float *split, int32_t *perm);
/* The device layouts mirt_scene_upload_flat derives from a scene, computed on
   the host alone (csrc/scene_layout.cpp; needs no ctx and makes no HIP call):
   the tree is checked as the upload checks it (MIRT_E_INVALID), then `part`
   is exactly the bytes the upload would send for that array (csrc/layout.h
   has the structs). Returns the part's size in bytes, or a negative error;
   copies the part when out != NULL and cap >= size; info may be NULL. */
typedef struct mirt_scene_layout_info {
    int32_t  encloses, ordered, leaf_big;   /* boxes nest (pruning allowed) / ordered walks allowed /
                                               four-wide layout larger than the chip's L2 */
    float    r_max, c_max, o_bound;         /* largest radius, largest |centre|_inf + radius, the bounded
                                               slab tests' coordinate bound C (0: none) */
    uint32_t num_pnodes, num_hnodes, num_leaves, wide_root;
    uint64_t leaf_box_off;                  /* byte offset of the leaf boxes behind the leaf spheres */
} mirt_scene_layout_info;
enum { MIRT_LAYOUT_DNODES = 0, MIRT_LAYOUT_GEO = 1, MIRT_LAYOUT_COLOR = 2, MIRT_LAYOUT_PNODES = 3,
       MIRT_LAYOUT_HNODES = 4, MIRT_LAYOUT_HAUX = 5, MIRT_LAYOUT_LEAF_GEO = 6, MIRT_LAYOUT_LEAF_BOX = 7,
       MIRT_LAYOUT_NDEPTH = 8 };
int64_t mirt_scene_layout(const mirt_sphere *spheres, int num_spheres, const mirt_node *nodes, int num_nodes,
                          int part, void *out, size_t cap, mirt_scene_layout_info *info);
/* The same parts and the same info read back from the ctx's resident scene,
   whichever call installed it (waits for the ctx's stream): same part ids and
   return convention. MIRT_E_NOSCENE without a scene, MIRT_E_INVALID for an
   unknown part; a cap below the part's size writes nothing. */
int64_t mirt_scene_resident_layout(mirt_ctx *ctx, int part, void *out, size_t cap, mirt_scene_layout_info *info);

/* The camera ray of every pixel of the shard (ray.c:17-32 with the pixel
   mapping of main.c:356-365). */
int mirt_camera_rays(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, mirt_ray *out);
/* The BVH debug overlay (bvh_visualiser.c:16-126, 'o' in main.c:323-327):
   every node of the uploaded tree with depth < max_levels (all: -1) drawn as
   its box's 12 projected edges, 5 one-pixel-offset lines each, coloured by
   depth, over black; a pixel shows the last line drawn over it in the
   reference's order (pre-order nodes, draw_aabb's edge order). Lines are
   rasterised by Bresenham between the integer endpoints of world_to_screen
   (the reference leaves that to SDL's backend). Writes width * height RGBA8.
   A node's depth is its true depth in the tree, for every tree an upload
   accepts, in the level test and in the colour alike: MIRT_LAYOUT_NDEPTH
   keeps one byte per node clamped to 255, and a node that carries 255 takes
   its depth from the descent from the root (O(depth) on trees deeper than 254
   only). max_levels < 0 draws every node, 0 none; a max_levels above the
   tree's depth equals -1. The camera's fields are used as given (no
   camera_update): a corner behind z <= 0.1, outside [-W, 2W] x [-H, 2H] or
   with a NaN coordinate drops its edges as the reference's tests do.
   MIRT_E_NOSCENE without a scene (a scene without a tree gives the cleared
   canvas); MIRT_E_INVALID for a NULL cam or out, for width or height <= 0 or
   above 2^30 (world_to_screen forms 2 * width and 2 * height in int), and for
   more than 2^31 pixels: checked before anything is allocated. Runs on the
   ctx's stream, behind every frame enqueued on it, and reuses the ctx's frame
   output slab: a frame in flight has been copied out before it is written. */
int mirt_bvh_overlay(mirt_ctx *ctx, const mirt_camera *cam, int width, int height, int max_levels,
                     mirt_rgba8 *out);
/* get_camera_ray (ray.c:17-32) at n caller-given (u, v) pairs (uv[2i],
   uv[2i+1]), for a frame of width x height (the reference's compile-time
   WIDTH/HEIGHT, ray.c:18). (u, v) need not lie on the pixel grid, nor be
   finite: direction = normalize(forward + horizontal * u + vertical * v) in
   binary32 without contraction, whatever that gives. n = 0 returns MIRT_OK
   and writes nothing; n < 0, a NULL cam, a NULL uv or out with n > 0, and
   width or height <= 0 return MIRT_E_INVALID. Needs no scene. */
int mirt_camera_rays_uv(mirt_ctx *ctx, const mirt_camera *cam, int width, int height, const float *uv, int n,
                        mirt_ray *out);

/* Reference-DFS work counters of one frame (instrumented kernel build,
   untimed): the algorithmic-bytes numerator of SURVEY §8(d). */
int mirt_count_frame(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, mirt_counts *out);

/* Diagnostic: renders the frame with the instrumented kernel and writes, per
   8x8 tile (= wave), {tile, traversal loop steps, start, end} with start/end
   read from the 100 MHz s_memrealtime clock. Returns the number of waves
   (or -waves if cap is too small). */
int mirt_wave_stats(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, uint32_t *out, int cap);

/* Diagnostic: renders the frame (depth >= 2, BVH, wavefront schedule) with the
   instrumented bounce kernel and writes MIRT_BOUNCE_STATS_WORDS uint64 per bounce wave
   (size `out` from that constant: the record has grown between releases): loop
   iterations, walking lanes summed over them, the same two after the bounce
   queue ran dry, start / queue-dry / end time (100 MHz clock), longest
   chain << 32 | longest walk (steps) of the lane loop, quad-drain loop
   iterations, the time the quad drain began (0: none), lane-steps of the
   lane loop spent in DFS-segment fallbacks (a four-wide step whose pushes
   would overflow the LDS lane stack walks the node's subtree in DFS order)
   and the fallbacks entered; then, of the lane loop's leaf gates (the
   four-wide walk without leaf batching): gate executions (iterations of the
   per-step gate loop), the executions in which any lane ran the f64 t of a
   candidate, the lanes that did, the executions in which any lane loaded a
   LeafBox for the exact box test, the lanes that did, and the loop
   iterations that held a gate / an f64 t / a LeafBox load; then
   (MIRT_OPT_CONFIRM_ONCE) the closest hits confirmed, the confirmations that
   failed (each walks its level again) and the walks restarted because they
   would have entered a DFS-segment fallback. Returns the
   number of waves (or -waves if cap is too small). */
#define MIRT_BOUNCE_STATS_WORDS 23
int mirt_bounce_stats(mirt_ctx *ctx, const mirt_camera *cam, const mirt_frame_desc *fd, uint64_t *out, int cap);

/* The ctx's own stream (a hipStream_t, non-blocking): the blocking calls run
   on it; a caller may pass it to mirt_render_frame_device. */
void *mirt_ctx_stream(mirt_ctx *ctx);

/* Device time (ms) of the last render kernel launched by a blocking call. */
float mirt_last_kernel_ms(mirt_ctx *ctx);

/* Device time (ms) of the two passes of the last frame this ctx launched
   with the wavefront schedule (blocking or _device call; waits for it):
   phase[0] = deferral mark + primary kernel (camera rays), phase[1] = the
   bounce kernel. Returns MIRT_E_INVALID if no wavefront frame was launched. */
int mirt_last_phase_ms(mirt_ctx *ctx, float *phase);
/* The same two times for each of the ctx's last min(max, 64) wavefront
   frames, oldest first (out[2j], out[2j + 1]), recorded by HIP events on the
   frame's own stream -- so frames that ran while other ctxs' frames shared
   the chip report their passes' durations under that overlap. Waits for
   them; returns the number of frames written. */
int mirt_phase_log(mirt_ctx *ctx, float *out, int max);

/* Kernel schedule knobs (results are identical under every setting; only
   speed changes). MIRT_OPT_TRAVERSAL: MIRT_TRAV_WAVEFRONT (default: camera-ray
   packets, then persistent per-lane bounce chains fed by a queue, for BVH
   frames of depth >= 2) or MIRT_TRAV_TILE (one kernel: each wave traces the
   whole paths of an 8x8 tile; always used for depth 1 and brute force).
   MIRT_OPT_FAST_SLAB: 1 (default) = reciprocal-multiply slab test with an
   exact-division fallback for undecidable boxes; 0 = the division-only slab
   test of hit.c:49-82 (and the reference DFS order everywhere).
   MIRT_OPT_BLOCK_WAVES: 8x8 pixel tiles (waves) per workgroup of the tile
   kernel: 1, 2, 4 (default) or 8. MIRT_OPT_DEFER: 1 (default) = on a tree
   that does not admit ordered walks, camera rays with a zero/tiny direction
   component are traced first, one per wave (node-parallel walk).
   MIRT_OPT_PRUNE: 1 (default) = with the fast slab test, skip subtrees whose
   box the ray provably enters beyond the best hit so far (the closest hit and
   its tie rule are unchanged; active only for a tree whose boxes enclose
   their subtrees, checked at upload); 0 = the reference's exhaustive DFS.
   MIRT_OPT_ORDERED: 1 (default) = with pruning, walks enter the nearer child
   first -- camera rays as packets over both-children nodes, bounce rays over
   a four-wide re-layout of the same tree (exact because the reference slab
   test is monotone under box containment); same closest hit, ties still go
   to the later DFS leaf; active only for a tree whose leaves hold increasing
   sphere indices in DFS order, as the reference's builds do, and depth < 63;
   0 = DFS order. */
enum { MIRT_OPT_TRAVERSAL = 1, MIRT_OPT_FAST_SLAB = 2, MIRT_OPT_BLOCK_WAVES = 3, MIRT_OPT_DEFER = 4,
       MIRT_OPT_BOUNCE_THRESHOLD = 5, /* wavefront: shade finished bounce rays once fewer than
                                         this many lanes of a wave still walk (0..64, default 20) */
       MIRT_OPT_PRUNE = 6, MIRT_OPT_ORDERED = 7,
       MIRT_OPT_BOUNCE_BLOCKS = 9,  /* wavefront: persistent bounce workgroups, 0 = occupancy x CUs
                                       (default: best for one frame at a time); with several contexts
                                       keeping frames in flight, ~1.5 per CU (384 on MI355X) */
       MIRT_OPT_QUAD_DRAIN = 11,    /* four-wide bounce walk: 1 (default) = once the queue is dry
                                       and <= 16 lanes of a wave are busy, finish them as quads */
       MIRT_OPT_LEAF_BATCH = 14,    /* four-wide bounce walk: load a step's passing leaf spheres
                                       together: 0 never, 1 always, 2 (default) when the tree's
                                       four-wide layout exceeds the chip's 32 MiB of L2;
                                       mirt_get_option reads back 0/1: in effect for the scene) */
       MIRT_OPT_QUAD_BATCH = 15,    /* mirt_intersect_rays / mirt_any_hit_rays with the BVH: 1
                                       (default) = a batch too small to fill the chip one ray per
                                       lane walks one ray per four lanes (benchmark.c's 10k rays) */
       MIRT_OPT_ZERO_COPY = 17,     /* frames of one sample into PAGE-LOCKED memory
                                       (mirt_host_alloc / mirt_host_register; the ctx's own
                                       accumulation): the frame kernels store every pixel
                                       straight into it instead of a DMA copy after them --
                                       1 (default) for the blocking mirt_render_frame, 2 for
                                       mirt_render_frame_async too, 0 never. Pageable memory:
                                       a copy. */
       MIRT_OPT_QUEUE_ORDER = 18,   /* wavefront: order of a frame's first bounces in the bounce
                                       queue -- 0 (default) = tile order for the blocking
                                       mirt_render_frame (a frame alone on the chip), grouped by
                                       direction octant per workgroup for frames in flight;
                                       1 = always grouped; 2 = always tile order. Speed only. */
       MIRT_OPT_DEBUG_STALL_MS = 19, /* test hook: every frame of this context starts behind a
                                       kernel that waits this many ms (0..10000, default 0), then
                                       exits -- a frame that overruns a caller's deadline
                                       (mirt_multi's MIRT_MULTI_OPT_TIMEOUT_MS) without a hang */
       MIRT_OPT_CONFIRM_ONCE = 21,  /* four-wide bounce walk without leaf batching: 1 = a walk
                                       tests only its closest sphere hit against the leaf's exact
                                       box, once, when the level is shaded, and walks the level
                                       again the old way should that box fail; 0 = every
                                       candidate hit is tested at once; 2 (default) = 1 for a
                                       tree of at most 32,768 leaves (measured ahead at 10k
                                       spheres, not separable at 100k), else 0.
                                       mirt_get_option reads back 0/1: in effect for the scene.
                                       Speed only. */
       MIRT_OPT_DEBUG_FAIL_CONFIRM = 22, /* test hook: N > 0 = that one test reports failure for
                                       every chain whose pixel index is a multiple of N although
                                       the box passed, so the second walk runs on ordinary
                                       scenes (same frames, slower); 0 (default) = off */
       MIRT_OPT_BUILD_FINISH = 23,  /* device build: once the longest open range of a level is at
                                       most F spheres, one wave per open node builds the node's
                                       whole subtree in one launch instead of a level at a time
                                       (mirt_last_build_finish): 0 = never, 2..64 = F,
                                       1 (default) = automatic: F = 64 for a build of at most
                                       131,072 spheres (measured ahead at 10k spheres, level at
                                       100k), else 0 (behind at 1M). Every other value is
                                       MIRT_E_INVALID; mirt_get_option reads back the stored
                                       value. Speed only: the same bytes under every setting. */
       MIRT_OPT_PRIMARY_CACHE = 24, /* a still camera (main.c:379-408's accumulating loop): 1 = the
                                       ctx keeps the camera rays' closest hits (t, sphere) of one
                                       slab, 8 bytes per shard pixel, and a frame whose camera
                                       rays are those of the frame that stored them starts from
                                       them instead of walking the tree (below:
                                       mirt_primary_cache_stats); 0 (default) = off: waits for the
                                       ctx's frames and releases the memory. Every other value is
                                       MIRT_E_INVALID; mirt_get_option reads back the stored
                                       value. Speed only: the same bytes under either setting. */
       MIRT_OPT_DENOISE_TILE = 26   /* mirt_denoise*: the passes of spacing 1 and 2 take their taps
                                       from an LDS tile with halo (1, default:
                                       MEASUREMENTS.md E) or by direct loads (0). Every other value is
                                       MIRT_E_INVALID. Speed only: the same bytes under either
                                       setting. (25 is not assigned.) */,
       MIRT_OPT_HISTORY_MOTION = 27 /* 1 = refits and updates this ctx installs record a link on
                                       the scene slot, and mirt_render_frame_reprojected on this
                                       ctx carries its history over such a link
                                       (mirt_history_motion_get); 0 (default) = every install
                                       empties the history. Every other value is
                                       MIRT_E_INVALID. */,
       MIRT_OPT_PRIMARY_SCAN = 28,  /* the camera pass finds each pixel's closest hit by a
                                       depth-sorted scan of the leaves per 8x8 tile instead of
                                       the packet walk, for the frames that qualify (below:
                                       mirt_primary_scan_stats): 0 = off (waits for the ctx's
                                       frames and releases the memory), 1 = on, 2 (default) =
                                       automatic: on until a scanned frame of the scene shows
                                       it to be sparse (SPARSE below). Every other value is
                                       MIRT_E_INVALID; mirt_get_option reads back the stored
                                       value. Speed only: the same bytes under every setting. */
       MIRT_OPT_PRIMARY_SCAN_BUDGET = 29, /* the chunks of 64 leaf records that a tile of that scan
                                       with a pixel still without a hit (a sky pixel: such a
                                       tile can only end once it has met all its records) reads
                                       before it takes the packet walk instead: 1 .. 2^24,
                                       default 256 (MEASUREMENTS.md E). A tile whose pixels all
                                       hold a hit ends by depth and reads up to 1,024 chunks
                                       whatever this is. Speed only. */
       MIRT_OPT_PRIMARY_SCAN_REBUILD = 30 /* NOT a supported setting: a measurement hook kept for
                                       MEASUREMENTS.md E's "rebuilt every frame" figures, which
                                       may go without notice. 1 = the scan's per-camera data are
                                       rebuilt by every frame; 0 (default) = kept while the
                                       camera, the frame geometry and the scene stay. */ };
/* Traversal ids keep their first-release values (mirt 0.1: TILE 0, WAVEFRONT 5).
   ABI note: the mirt 0.2 header numbered WAVEFRONT 1; mirt_set_option accepts
   1 as a deprecated alias of MIRT_TRAV_WAVEFRONT (mirt_get_option reads back
   5), to be dropped in 1.0. The retired ids 2-4 (chunked / DFS-only schedules
   of mirt 0.1) and the retired option ids 8, 10, 12, 13, 20 (20: the bounce
   pass's continuation queue of mirt 0.5, measured slower and removed) return
   MIRT_E_INVALID. */
enum { MIRT_TRAV_TILE = 0, MIRT_TRAV_WAVEFRONT = 5, MIRT_TRAV_WAVEFRONT_V02 = 1 /* deprecated alias */ };
int mirt_set_option(mirt_ctx *ctx, int option, int value);
int mirt_get_option(mirt_ctx *ctx, int option);

/* MIRT_OPT_PRIMARY_CACHE 1: every frame the ctx enqueues (mirt_render_frame,
   _device, _async, and the frames mirt_multi issues on it) is classified on
   the host when it is enqueued.
     BYPASS: the frame runs exactly as with the option off; the cache is neither
       read nor written and stays valid if it was. First reason found, in this
       order: SCHEDULE -- the frame does not run the ordered camera-packet kernel
       (MIRT_TRAV_TILE, brute force, a tree without ordered walks,
       MIRT_OPT_FAST_SLAB / _PRUNE / _ORDERED 0, depth 0, mirt_count_frame,
       mirt_wave_stats, mirt_bounce_stats); JITTER -- fd->jitter; PLANES -- a
       mirt_render_frame_planes* frame; RAYS -- a mirt_render_rays* frame;
       LENS -- a mirt_render_lens_frame* frame with aperture > 0.
     The key of every other frame, compared bitwise: what its camera rays and
       its pixel -> row map are computed from (the camera as the frame sees it:
       position, forward, and the horizontal and vertical spans; aspect, width,
       height, row_block, shard, num_shards, lead_skip and the shard's rows)
       and mirt_ctx_scene_id at enqueue. Not in the key: seed, sample, samples,
       max_depth, accumulate, frames, the outputs, the stream, the speed options.
     HIT: the cache is valid and holds the hits of this key. The camera pass
       loads each pixel's (t, sphere) instead of walking; everything behind it
       is unchanged. The stored t is the walk's t, so the frame is the walked
       frame byte for byte.
     FILL: every other frame. Its camera pass walks and also stores the hits
       of its first frame; the key is recorded. First reason found, in this
       order: EMPTY -- no valid cache; SCENE -- another scene id (every
       install gives a new one: no install hook is needed); CAMERA -- the
       caller's mirt_camera differs; GEOMETRY -- the frame desc does.
   Frames of one ctx never overlap, whatever streams they run on, so the cache
   needs no synchronisation of its own. The slab grows like the ctx's other
   buffers: after waiting for the ctx's frames; never on a hit or a fill of the
   same size. mirt_destroy releases it. */
enum { MIRT_PCACHE_BYPASS = 0, MIRT_PCACHE_FILL = 1, MIRT_PCACHE_HIT = 2 };
enum { MIRT_PCACHE_EMPTY = 1, MIRT_PCACHE_SCENE = 2, MIRT_PCACHE_CAMERA = 3, MIRT_PCACHE_GEOMETRY = 4,
       MIRT_PCACHE_OFF = 5, /* the option is 0 (what mirt_primary_cache_stats_get then reports) */
       MIRT_PCACHE_SCHEDULE = 6, MIRT_PCACHE_JITTER = 7, MIRT_PCACHE_PLANES = 8,
       MIRT_PCACHE_RAYS = 9 /* a ray frame (mirt_render_rays*): no camera to key by */,
       /* 10: a lens frame with aperture > 0 (its rays change with every sample) */
       MIRT_PCACHE_LENS = MIRT_PCACHE_RAYS + 1 };
typedef struct mirt_primary_cache_stats {
    uint64_t hits, fills, bypassed;   /* frames classified since the option was last set to 1 */
    uint64_t scene_id;                /* of the key; 0 when not valid */
    uint64_t bytes;                   /* device memory the cache holds */
    int32_t  valid;                   /* 1: the cache holds the hits of a key */
    int32_t  last;                    /* of the last frame enqueued: MIRT_PCACHE_HIT / _FILL / _BYPASS */
    int32_t  reason;                  /* why it was not a hit (enum above); 0 on a hit */
    int32_t  width, rows;             /* geometry of the slab held; 0 when not valid */
} mirt_primary_cache_stats;
/* No HIP call. MIRT_E_INVALID for a NULL ctx or out. */
int mirt_primary_cache_stats_get(mirt_ctx *ctx, mirt_primary_cache_stats *out);
/* The slab itself, for tests: rows * width elements, pixel r * width + x in
   shard row order, t = 0 and sphere = -1 on a miss (the t and sphere planes of
   mirt_render_frame_planes for that frame). Both calls wait for the ctx's
   frames; both return MIRT_E_INVALID before any HIP call for a NULL argument,
   a cache that is not valid, or n != rows * width. _write replaces the slab
   after checking every element on the host: sphere in [-1, num_spheres) of the
   resident scene and, where sphere >= 0, t finite and > 0; otherwise
   MIRT_E_INVALID and nothing is written, so no slab can make a later frame
   index out of bounds. */
int mirt_primary_cache_read(mirt_ctx *ctx, float *t, int32_t *sphere, size_t n);
int mirt_primary_cache_write(mirt_ctx *ctx, const float *t, const int32_t *sphere, size_t n);

/* MIRT_OPT_PRIMARY_SCAN 1 or 2: every frame the ctx enqueues is classified on
   the host when it is enqueued.
     SCAN: the frame traces every camera ray, but not by the packet walk. Per
       (camera, frame geometry, scene id) -- the primary cache's key, compared
       bitwise -- the ctx keeps one 16-byte record per leaf (a depth key, the
       leaf, the rectangle of 8x8 tiles its sphere can be hit from) sorted by
       key, and per tile the number of records that hold it. Per frame one wave
       per tile reads the records in key order, tests the leaves that hold its
       tile with the walk's own sphere and box tests, and stops once every
       pixel's hit is nearer than every record left or the tile's records are
       exhausted; a tile that still has a pixel without a hit after
       MIRT_OPT_PRIMARY_SCAN_BUDGET chunks (any tile after 1,024) is walked
       instead. The hits go to a slab of the primary cache's format
       and the camera-packet kernel's cached form shades them: the frame is the
       walked frame byte for byte.
     BYPASS: the frame runs exactly as with the option off. First reason found,
       in this order: CACHE -- MIRT_OPT_PRIMARY_CACHE is 1; SCHEDULE, JITTER,
       PLANES, RAYS, LENS -- as for the primary cache; TREE -- the tree does not
       nest, is not ordered, or its coordinates are not bounded (beyond 6e4,
       infinite or NaN); SHARD -- num_shards > 1 (or lead_skip) with a row_block
       that is no multiple of 8; SIZE -- more than 65535 tiles along an axis;
       CAMERA -- not finite, a basis whose triple product (forward x up).right
       is zero or nearly so, or a field of view so wide that a corner ray is at
       right angles to forward or beyond; SPARSE -- option 2 only: an earlier
       scanned frame of this scene read more than 16 chunks per tile that holds
       a record, as a scene does whose spheres leave sky in most tiles (such a
       tile can only end on its count, and the walk is then faster:
       MEASUREMENTS.md E). The verdict reaches the host without a wait, so the
       frames enqueued before it lands are still scanned; it holds until another
       scene is installed or the option is set again.
   Memory: 8 bytes per shard pixel, 40 bytes per leaf plus the sort's scratch,
   4 bytes per tile; it grows like the ctx's other buffers, after waiting for
   the ctx's frames, never while the sizes stay. Option 0 and mirt_destroy
   release it. */
enum { MIRT_PSCAN_BYPASS = 0, MIRT_PSCAN_SCAN = 1 };
enum { MIRT_PSCAN_NONE = 0, MIRT_PSCAN_OFF = 1, MIRT_PSCAN_CACHE = 2, MIRT_PSCAN_SCHEDULE = 3, MIRT_PSCAN_JITTER = 4,
       MIRT_PSCAN_PLANES = 5, MIRT_PSCAN_RAYS = 6, MIRT_PSCAN_LENS = 7, MIRT_PSCAN_TREE = 8, MIRT_PSCAN_SHARD = 9,
       MIRT_PSCAN_SIZE = 10, MIRT_PSCAN_CAMERA = 11, MIRT_PSCAN_SPARSE = 12 };
typedef struct mirt_primary_scan_stats {
    uint64_t scanned, bypassed;       /* frames classified since the option was last set (OFF is not counted) */
    uint64_t rebuilds;                /* builds of the per-camera data since then */
    uint64_t bytes;                   /* device memory the scan holds */
    /* of the last frame enqueued, when it was a SCAN (else 0): */
    uint64_t tiles_scan;              /* tiles holding a record that finished in the scan */
    uint64_t tiles_walk;              /* tiles sent to the walk list */
    uint64_t tiles_empty;             /* tiles no record holds */
    uint64_t chunks;                  /* chunks of 64 records read */
    uint64_t leaves_tested;           /* leaves tested against a tile's 64 rays */
    uint64_t candidates;              /* records whose rectangle holds a tile, summed over the tiles that hold one */
    int32_t  last;                    /* of the last frame enqueued: MIRT_PSCAN_SCAN / _BYPASS */
    int32_t  reason;                  /* why it was a bypass (enum above); 0 on a scan */
    int32_t  budget;                  /* MIRT_OPT_PRIMARY_SCAN_BUDGET */
    int32_t  leaves;                  /* records of the per-camera data held; 0 when none */
} mirt_primary_scan_stats;
/* Waits for the ctx's frames and copies the counters only when the last frame
   was a SCAN; otherwise no HIP call. MIRT_E_INVALID for a NULL ctx or out. */
int mirt_primary_scan_stats_get(mirt_ctx *ctx, mirt_primary_scan_stats *out);
/* The scan's per-camera arithmetic on the host (csrc/pscan.h, the code the
   kernels compile), for tests; no ctx, no device. Both return MIRT_E_INVALID
   for invalid arguments, else 0 for a camera the scan accepts or 1 (not
   finite) / 2 (degenerate basis) / 3 (too wide) for one it bypasses.
   mirt_pscan_camera: g[3] = the unit forward the depth keys are measured
   along, *rho = the relative direction error allowed for camera_ray (either
   may be NULL). mirt_pscan_records: for each of n spheres geo[4k..] = (centre,
   radius): z[k] = its depth key, rect[4k..] = its tile rectangle i0, i1, j0, j1
   (i0 > i1: empty), reach[k] (may be NULL) = R', the distance from the centre
   within which every recorded hit lies. */
int mirt_pscan_camera(const mirt_camera *cam, int width, int height, float *g, double *rho);
int mirt_pscan_records(const mirt_camera *cam, int width, int height, const float *geo, int64_t n, float *z,
                       int32_t *rect, double *reach);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_H */

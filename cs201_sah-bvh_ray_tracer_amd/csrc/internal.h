// Internal helpers shared by the host translation units of libmirt.so.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/mirt.h"

struct ihipStream_t;  // hipStream_t is a pointer to it

namespace mirt {

// Thread-local last error (mirt_last_error()).
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// Shard geometry of mirt_frame_desc (csrc/shard.h): row r of the compacted
// shard is image row y = shard_block(shard, r / rb) * rb + r % rb.
int shard_row_count(const mirt_frame_desc* fd);
bool frame_desc_valid(const mirt_frame_desc* fd);

// A well-formed flat pre-order tree (mirt_node): root skip == nn; every skip
// in (i, nn]; leaves skip to i + 1 and index spheres in [sphere_lo,
// num_spheres] (num_spheres: the never-hit sentinel); the empty flag only on
// leaves; every inner node's two subtrees [i+1, r) and [r, skip) nest inside
// it. MIRT_OK or MIRT_E_INVALID with the message prefixed by `fn`.
int validate_flat(const mirt_node* nd, int nn, int num_spheres, int sphere_lo, const char* fn);

// render.hip: the frame of mirt_render_frame up to its D2H copy, enqueued on
// the ctx's own stream into d_out (fd->samples slabs of the shard; the ctx's
// own buffer when null) with the ctx's (possibly shared) accumulation buffer;
// *d_display = the slab holding the display after the last frame.
// independent (fd->samples > 1, !fd->accumulate): the samples are successive
// FRESH frames (main.c:358-374 each), left raw in their slabs, the last one
// folded into the accumulation buffer as a fresh frame; otherwise they fold in
// order (a frame of several samples / the accumulating display loop).
// lens (valid, aperture > 0): the frame is a lens frame (mirt_render_lens_frame*).
int enqueue_frame_device(mirt_ctx* c, const mirt_camera* cam, const mirt_frame_desc* fd, uint32_t* d_out,
                         uint32_t** d_display, const char* fn, bool independent = false,
                         const mirt_lens* lens = nullptr);
int ctx_device(const mirt_ctx* c);
int ctx_build_finish(const mirt_ctx* c);  // MIRT_OPT_BUILD_FINISH as stored: 0 off, 1 automatic, 2..64 = F
// bvh_device.hip: the device builder's scratch and statistics, kept on the ctx
// (created by the first build, released by mirt_destroy).
struct BuildState;
BuildState** ctx_build_state(mirt_ctx* c);
void build_state_free(BuildState* st);
// The same build left on the device (mirt_scene_build_device): all `total`
// spheres are copied to the build's scratch, the tree of [start, end) is built
// there, and *out points at the reordered 20-byte spheres and the flat nodes
// in that scratch -- valid until the ctx's next build. The kernels are
// enqueued on the ctx's stream, not waited for. *declined = 1: the input is
// one the kernels decline, nothing was built. build_resident_ms: the device
// time of that build, once the stream has been synchronised.
struct ResidentTree {
    const uint32_t* aos;
    const mirt_node* nodes;
    int num_nodes;
    int levels;
};
int build_resident(mirt_ctx* c, const mirt_sphere* spheres, int total, int start, int end, int depth,
                   ResidentTree* out, int* declined);
// The same from `total` spheres in device memory (read on the ctx's stream,
// not written): the build runs on a copy whose colour words hold the spheres'
// indices -- what mirt_scene_update_device builds on to learn its permutation
// -- and d_colour[total] (device) receives the spheres' own colours.
int build_resident_tagged(mirt_ctx* c, const void* d_spheres, int total, int start, int end, int depth,
                          uint32_t* d_colour, ResidentTree* out, int* declined);
int build_resident_ms(mirt_ctx* c, float* ms);
// render.hip: the scene arrays of a ctx (csrc/layout.h has the element types),
// all device allocations the ctx owns, and the scalars that go with them.
struct DeviceScene {
    void *dnodes = nullptr, *nodes32 = nullptr, *geo = nullptr, *color = nullptr, *pnodes = nullptr,
         *hnodes = nullptr, *haux = nullptr, *leaves = nullptr, *ndepth = nullptr;
    int num_nodes = 0, num_spheres = 0;
    uint32_t num_pnodes = 0, num_hnodes = 0, num_leaves = 0, wide_root = 0;
    size_t leaf_box_off = 0;
    bool encloses = false, ordered = false, leaf_big = false;
    float r_max = 0.0f, c_max = 0.0f, o_bound = 0.0f;
};
// Installs `sc` (complete on the device) in the ctx's scene slot, for every ctx
// that shares it; the slot owns the arrays from here on. The scene it held is
// freed once the frames enqueued on it have finished (mirt_ctx_share_scene).
int ctx_install_scene(mirt_ctx* c, const DeviceScene& sc);
// the two ctxs render one scene slot
bool ctx_shares_scene(const mirt_ctx* a, const mirt_ctx* b);
void ctx_set_scene_stats(mirt_ctx* c, const mirt_scene_build_stats& st);
// What a refit reads of the resident scene (refit_device.hip): the public 32-B
// tree and the node depths on the device, and the scalars. false: no scene.
struct ResidentScene {
    const mirt_node* nodes32;
    const uint8_t* ndepth;
    int num_nodes, num_spheres;
    bool ordered;
};
bool ctx_resident_scene(const mirt_ctx* c, ResidentScene* out);
void ctx_set_refit_stats(mirt_ctx* c, const mirt_refit_stats& st);
// scene_device.hip: the layouts of the `ns` 20-byte spheres at d_aos and the
// validated flat tree d_nodes[nn], both on the device, made by the layout
// kernels on `stream` (a hipStream_t) and installed in the ctx. Blocking; on
// failure the ctx keeps the scene it had.
int layout_device(mirt_ctx* c, ihipStream_t* stream, const uint32_t* d_aos, int ns, const mirt_node* d_nodes, int nn,
                  const char* fn);
// quality_device.hip: the mirt_tree_quality of the validated flat tree
// d_nodes[nn] on the device, by the kernel on `stream`, byte for byte what
// mirt_bvh_quality_flat gives for those nodes. Blocking; touches no ctx.
int quality_device(ihipStream_t* stream, const mirt_node* d_nodes, int nn, int ns, mirt_tree_quality* out,
                   const char* fn);
// render.hip: the cost of the tree the last mirt_scene_update_device installed
// in the ctx's scene slot (false: none -- every install drops it, only that
// call sets it again).
bool ctx_base_cost(const mirt_ctx* c, double* cost);
void ctx_set_base_cost(mirt_ctx* c, double cost);
// pscan.hip: the per-camera data of the primary scan (pscan.h),
// built on `stream` into arrays the ctx owns: nl records sorted by key in
// `rec`, and in `grid` ((ntx + 1) x (nty + 1) ints, row-major) the records
// holding each tile. rec_in / key_in / key_out / planes (ntx + nty) / sort_tmp
// (pscan_sort_bytes(nl) bytes) are scratch. Returns the hipError_t.
struct PscanCam;
struct PscanRec;
struct PscanPlanes;
struct PscanBuild {
    PscanRec *rec_in, *rec;
    float *key_in, *key_out;
    PscanPlanes* planes;
    int* grid;
    void* sort_tmp;
    size_t sort_bytes;
};
size_t pscan_sort_bytes(uint32_t nl);
int pscan_build(const PscanCam& cam, const void* leaf_geo, uint32_t nl, const PscanBuild& b, ihipStream_t* stream);
// denoise_host.cpp: what every form of mirt_denoise checks of its arguments
// (pointers are only compared with null).
bool denoise_args_valid(int width, int height, const void* rgba, const void* accum, int frames, const void* sphere,
                        const mirt_denoise_params* params, const void* out, const void* out_rgb);
// denoise.hip: the filter's scratch, kept on the ctx (created by the first
// call, released by mirt_destroy), and the filter of VALID arguments, all in
// device memory, enqueued on `stream` under the name `fn` of the entry point
// it serves. MIRT_OPT_DENOISE_TILE as stored: ctx_denoise_tile.
struct DenoiseState;
DenoiseState** ctx_denoise_state(mirt_ctx* c);
void denoise_state_free(DenoiseState* st);
int ctx_denoise_tile(const mirt_ctx* c);
int denoise_enqueue(mirt_ctx* c, int width, int height, const uint32_t* d_rgba, const float* d_accum, int frames,
                    const int32_t* d_sphere, const float* d_normal, const mirt_denoise_params* params,
                    uint32_t* d_out, float* d_out_rgb, ihipStream_t* stream, const char* fn);
// reproject_host.cpp: what every form of mirt_reproject checks of its
// arguments (pointers are only compared with null and with each other).
bool reproject_args_valid(int width, int height, const void* cam, const void* cam_prev, const void* rgba, const void* t,
                          const void* sphere, const void* hist, const void* t_prev, const void* sphere_prev,
                          const mirt_reproject_params* params, const void* hist_out);
// What the mirt_reproject_moments forms check beyond that: a motion, if given,
// is valid; m2_prev is null exactly when hist is; m2_out is given and is not
// m2_prev.
bool reproject_moments_valid(const void* hist, const mirt_sphere_motion* motion, bool has_prev, const void* m2_prev,
                             const void* m2_out);
// vfilter_host.cpp: what every form of mirt_denoise_var checks of its
// arguments (pointers are only compared with null).
bool vfilter_args_valid(int width, int height, const void* hist, const void* m2, const void* sphere,
                        const mirt_denoise_var_params* params, const void* out, const void* out_rgb);
// vfilter.hip: the variance-guided filter's scratch, kept on the ctx (created
// by the first call, released by mirt_destroy).
struct VfilterState;
VfilterState** ctx_vfilter_state(mirt_ctx* c);
void vfilter_state_free(VfilterState* st);
// The filter of VALID arguments, all in device memory, enqueued on `stream`
// under the name `fn` of the entry point it serves; vfilter_params_ok: the
// parameters are valid (vfilter_host.cpp).
int vfilter_enqueue(mirt_ctx* c, int width, int height, const mirt_history_px* d_hist, const float* d_m2,
                    const int32_t* d_sphere, const float* d_normal, const mirt_denoise_var_params* params,
                    uint32_t* d_out, float* d_out_rgb, float* d_var_out, ihipStream_t* stream, const char* fn);
bool vfilter_params_ok(const mirt_denoise_var_params* params);
// reproject.hip: the history of mirt_render_frame_reprojected, kept on the ctx
// (created by the first call, released by mirt_destroy). begin: the history is
// emptied if the image or the scene is not the one it was made of, and
// *d_t / *d_sphere are where the frame about to be enqueued stores its planes;
// end: the frame's display d_rgba is reprojected from the history on `stream`
// into the pair's other half, which becomes the history; *d_shown = the
// display of the new records.
struct ReprojectState;
ReprojectState** ctx_reproject_state(mirt_ctx* c);
void reproject_state_free(ReprojectState* st);
// link_from / link_motion (MIRT_OPT_HISTORY_MOTION 1): the scene id the slot's
// link to `scene_id` starts at (0: no link the ctx may use) and that link's
// motion, device pointers. A history of exactly the scene link_from is kept
// by begin, and end reprojects it with the motion; reproject_last_carried:
// the last frame did.
// moments (mirt_render_frame_reprojected_denoised): the records carry m2 in a
// pair of planes allocated beside the history by the first such call; begin
// empties a history without moments and gives *d_normal, where the frame
// stores its normal plane; end carries m2 with the records. filter: the
// variance-guided filter of the new records on `stream`, *d_filtered = its
// display. Without moments begin and end proceed as they did and drop the flag.
int reproject_frame_begin(mirt_ctx* c, int width, int height, uint64_t scene_id, uint64_t link_from, float** d_t,
                          int32_t** d_sphere, const char* fn, bool moments = false, float** d_normal = nullptr);
int reproject_frame_end(mirt_ctx* c, const mirt_camera* cam, const uint32_t* d_rgba,
                        const mirt_reproject_params* params, const mirt_sphere_motion* link_motion,
                        const uint32_t** d_shown, ihipStream_t* stream, bool moments = false);
int reproject_frame_filter(mirt_ctx* c, const mirt_denoise_var_params* vp, const uint32_t** d_filtered,
                           ihipStream_t* stream, const char* fn);
bool reproject_last_carried(mirt_ctx* c);
// render.hip: what the install a refit or an update is about to make records
// on the scene slot when the ctx has MIRT_OPT_HISTORY_MOTION 1:
// active, whether it is a rebuild, and the rebuild's permutation (perm[i] = the
// previous index of the sphere now at i) in device memory, written on the
// ctx's stream, or in host memory. Holds until ctx_link_intent_clear; an
// install outside such a bracket clears the slot's link.
void ctx_link_intent(mirt_ctx* c, bool rebuilt, const int32_t* d_perm, const int32_t* h_perm);
void ctx_link_intent_clear(mirt_ctx* c);
// render.hip: a launch on `stream` that uses scratch the ctx keeps, outside a
// frame. begin: the stream waits for the ctx's previous launch if that ran on
// another stream (host_wait: the host does, whichever stream it ran on --
// before scratch is reallocated); end: this launch is the ctx's previous one.
int ctx_launch_begin(mirt_ctx* c, ihipStream_t* stream, bool host_wait);
int ctx_launch_end(mirt_ctx* c, ihipStream_t* stream);
// [p, p + bytes) is ONE page-locked host range (mirt_host_alloc /
// mirt_host_register): copies into it are DMA, asynchronous to the host.
bool host_page_locked(const void* p, size_t bytes);
uint32_t* host_device_ptr(const void* p, size_t bytes);
int accum_settle(mirt_ctx* c);
void pinned_add(const void* p, size_t bytes);   // mirt_host_alloc / mirt_host_register ranges
void pinned_remove(const void* p);

}  // namespace mirt

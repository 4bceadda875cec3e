"""numpy/ctypes mirror of include/mirt.h (the C-ABI of the render path).

Every dtype here is byte-compatible with the struct of the same name in
include/mirt.h, which in turn is layout-compatible with the reference's own
types (vec3.h:3-7, sphere.h:7-11, ray.h:5-8, camera.h:5-14, bvh.h:7-18,
hit.h:8-14).
"""
import ctypes as C

import numpy as np

VEC3 = ("<f4", (3,))

SPHERE = np.dtype([("center", *VEC3), ("radius", "<f4"), ("color", "u1", (4,))])   # 20 B
RAY = np.dtype([("origin", *VEC3), ("direction", *VEC3)])                           # 24 B
AABB = np.dtype([("min", *VEC3), ("max", *VEC3)])                                    # 24 B
HIT = np.dtype([("t", "<f4"), ("point", *VEC3), ("normal", *VEC3),
                ("hit", "<i4"), ("sphere", "<i4"), ("pad", "<i4")])                   # 40 B
NODE = np.dtype([("bmin", *VEC3), ("bmax", *VEC3), ("sphere", "<i4"), ("skip", "<u4")])  # 32 B
CAMERA = np.dtype([("position", *VEC3), ("forward", *VEC3), ("right", *VEC3), ("up", *VEC3),
                   ("yaw", "<f4"), ("pitch", "<f4"), ("fov", "<f4"), ("move", "<i4")])   # 64 B

NODE_EMPTY = 0x80000000
SKIP_MASK = 0x7FFFFFFF

# The device layouts of csrc/layout.h (mirt_scene_layout returns them).
GEO = np.dtype(("<f4", (4,)))                                                        # 16 B: centre.xyz, radius
DNODE = np.dtype([("bmin", *VEC3), ("bmax", *VEC3), ("sphere", "<i4"), ("skip", "<u4"),
                  ("geo", "<f4", (4,)), ("pad", "<u4", (4,))])                        # 64 B
PNODE = np.dtype([("c0", "<f4", (6,)), ("c1", "<f4", (6,)), ("ref0", "<u4"), ("ref1", "<u4"),
                  ("flat", "<u4"), ("end", "<u4")])                                   # 64 B
HSLOT = np.dtype([("box", "<u4", (3,)), ("ref", "<u4")])       # box: fp16 lo | fp16 hi << 16 per axis
HNODE = np.dtype([("slot", HSLOT, (4,))])                                             # 64 B
HAUX = np.dtype([("flat", "<u4"), ("end", "<u4")])                                    # 8 B
LEAFBOX = np.dtype([("lo", *VEC3), ("hi", *VEC3), ("sphere", "<i4"), ("pad", "<u4")])  # 32 B
P_LEAF, P_NONE, P_INDEX = 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF
# MIRT_LAYOUT_* part ids, in order, with the dtype of each part's elements
LAYOUT_PARTS = [("dnodes", DNODE), ("geo", GEO), ("color", np.dtype("<u4")), ("pnodes", PNODE), ("hnodes", HNODE),
                ("haux", HAUX), ("leaf_geo", GEO), ("leaf_box", LEAFBOX), ("ndepth", np.dtype("u1"))]

assert SPHERE.itemsize == 20 and RAY.itemsize == 24 and AABB.itemsize == 24
assert HIT.itemsize == 40 and NODE.itemsize == 32 and CAMERA.itemsize == 64
assert DNODE.itemsize == 64 and PNODE.itemsize == 64 and HNODE.itemsize == 64 and HAUX.itemsize == 8
assert LEAFBOX.itemsize == 32 and GEO.itemsize == 16


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Camera(C.Structure):
    """camera.h:5-14"""
    _fields_ = [("position", Vec3), ("forward", Vec3), ("right", Vec3), ("up", Vec3),
                ("yaw", C.c_float), ("pitch", C.c_float), ("fov", C.c_float), ("move", C.c_int)]

    def to_numpy(self):
        return np.frombuffer(bytes(self), dtype=CAMERA)[0]

    @classmethod
    def from_numpy(cls, rec):
        return cls.from_buffer_copy(np.asarray(rec, dtype=CAMERA).tobytes())


class Ray(C.Structure):
    """ray.h:5-8 (by value in the per-ray drop-in calls)"""
    _fields_ = [("origin", Vec3), ("direction", Vec3)]


class Aabb(C.Structure):
    """bvh.h:7-10"""
    _fields_ = [("min", Vec3), ("max", Vec3)]


class Rgba8(C.Structure):
    """SDL_Color"""
    _fields_ = [("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("a", C.c_uint8)]


class HitRecord(C.Structure):
    """hit.h:8-14 (object: pointer into the caller's sphere array)"""
    _fields_ = [("t", C.c_float), ("point", Vec3), ("normal", Vec3), ("hit_something", C.c_int),
                ("object", C.c_void_p)]


class RandState(C.Structure):
    """glibc TYPE_3 rand() state (mirt_rand_state)."""
    _fields_ = [("r", C.c_int32 * 34), ("f", C.c_int32), ("b", C.c_int32)]


class FrameDesc(C.Structure):
    """mirt_frame_desc"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_depth", C.c_int32),
                ("use_bvh", C.c_int32), ("seed", C.c_uint64), ("sample", C.c_uint32),
                ("accumulate", C.c_int32), ("frames", C.c_int32), ("row_block", C.c_int32),
                ("shard", C.c_int32), ("num_shards", C.c_int32), ("samples", C.c_int32),
                ("jitter", C.c_int32), ("lead_skip", C.c_int32)]


class PrimaryPlanes(C.Structure):
    """mirt_primary_planes (a NULL member is not written)"""
    _fields_ = [("t", C.c_void_p), ("sphere", C.c_void_p), ("normal", C.c_void_p)]


class Lens(C.Structure):
    """mirt_lens: a thin lens (aperture 0 = the pinhole)"""
    _fields_ = [("aperture", C.c_float), ("focus", C.c_float)]


class DenoiseParams(C.Structure):
    """mirt_denoise_params (mirt_denoise_params_default: 3, 3, 0)"""
    _fields_ = [("passes", C.c_int32), ("normal_sharpness", C.c_int32), ("sigma_colour", C.c_float)]


class DenoiseVarParams(C.Structure):
    """mirt_denoise_var_params (mirt_denoise_var_params_default: 3, 3, 8, 4)"""
    _fields_ = [("passes", C.c_int32), ("normal_sharpness", C.c_int32), ("sigma_lum", C.c_float),
                ("min_history", C.c_int32)]


class ReprojectParams(C.Structure):
    """mirt_reproject_params (mirt_reproject_params_default: 64, 4, 1/64)"""
    _fields_ = [("max_history", C.c_int32), ("taps", C.c_int32), ("t_tolerance", C.c_float)]


class HistoryStats(C.Structure):
    """mirt_history_stats"""
    _fields_ = [("frames", C.c_uint64), ("scene_id", C.c_uint64), ("bytes", C.c_uint64), ("reused", C.c_uint64),
                ("fresh", C.c_uint64), ("sky", C.c_uint64), ("width", C.c_int32), ("height", C.c_int32)]


class SphereMotion(C.Structure):
    """mirt_sphere_motion: geo[num_spheres] and geo_prev[num_prev] float4 (centre, radius), prev_index (or NULL)"""
    _fields_ = [("geo", C.c_void_p), ("geo_prev", C.c_void_p), ("prev_index", C.c_void_p),
                ("num_spheres", C.c_int32), ("num_prev", C.c_int32)]


class HistoryMotion(C.Structure):
    """mirt_history_motion"""
    _fields_ = [("from_scene_id", C.c_uint64), ("to_scene_id", C.c_uint64), ("bytes", C.c_uint64),
                ("rebuilt", C.c_int32), ("carried", C.c_int32)]


# mirt_history_px: the mean of n samples (n == 0: no history)
HISTORY = np.dtype([("r", np.float32), ("g", np.float32), ("b", np.float32), ("n", np.int32)])
assert HISTORY.itemsize == 16


class PrimaryScanStats(C.Structure):
    """mirt_primary_scan_stats"""
    _fields_ = [("scanned", C.c_uint64), ("bypassed", C.c_uint64), ("rebuilds", C.c_uint64), ("bytes", C.c_uint64),
                ("tiles_scan", C.c_uint64), ("tiles_walk", C.c_uint64), ("tiles_empty", C.c_uint64),
                ("chunks", C.c_uint64), ("leaves_tested", C.c_uint64), ("candidates", C.c_uint64), ("last", C.c_int32), ("reason", C.c_int32),
                ("budget", C.c_int32), ("leaves", C.c_int32)]


class PrimaryCacheStats(C.Structure):
    """mirt_primary_cache_stats"""
    _fields_ = [("hits", C.c_uint64), ("fills", C.c_uint64), ("bypassed", C.c_uint64), ("scene_id", C.c_uint64),
                ("bytes", C.c_uint64), ("valid", C.c_int32), ("last", C.c_int32), ("reason", C.c_int32),
                ("width", C.c_int32), ("rows", C.c_int32)]


class Counts(C.Structure):
    """mirt_counts"""
    _fields_ = [("rays", C.c_uint64), ("nodes", C.c_uint64), ("spheres", C.c_uint64), ("hits", C.c_uint64),
                ("lane_steps", C.c_uint64), ("nodes_primary", C.c_uint64), ("spheres_primary", C.c_uint64),
                ("hits_primary", C.c_uint64)]


class BuildStats(C.Structure):
    """mirt_build_stats"""
    _fields_ = [("on_device", C.c_int32), ("levels", C.c_int32), ("nodes", C.c_int32),
                ("device_ms", C.c_float), ("total_ms", C.c_float)]


class BuildFinishStats(C.Structure):
    """mirt_build_finish_stats"""
    _fields_ = [("range", C.c_int32), ("round", C.c_int32), ("subtrees", C.c_int32), ("nodes", C.c_int32),
                ("moved", C.c_int32), ("finish_ms", C.c_float)]


class SceneBuildStats(C.Structure):
    """mirt_scene_build_stats"""
    _fields_ = [("on_device", C.c_int32), ("levels", C.c_int32), ("nodes", C.c_int32),
                ("build_ms", C.c_float), ("layout_ms", C.c_float), ("total_ms", C.c_float)]


class RefitStats(C.Structure):
    """mirt_refit_stats"""
    _fields_ = [("on_device", C.c_int32), ("nodes", C.c_int32),
                ("refit_ms", C.c_float), ("layout_ms", C.c_float), ("total_ms", C.c_float)]


class TreeQuality(C.Structure):
    """mirt_tree_quality"""
    _fields_ = [("inner_area", C.c_double), ("leaf_area", C.c_double), ("overhead", C.c_double), ("cost", C.c_double),
                ("root_area", C.c_float), ("inner_nodes", C.c_int32), ("leaves", C.c_int32),
                ("dead_leaves", C.c_int32), ("clamped", C.c_int32), ("degenerate", C.c_int32)]


class UpdateResult(C.Structure):
    """mirt_update_result"""
    _fields_ = [("rebuilt", C.c_int32), ("on_device", C.c_int32), ("base_cost", C.c_double), ("cost", C.c_double),
                ("decay", C.c_double), ("installed", TreeQuality), ("total_ms", C.c_float)]


class SceneLayoutInfo(C.Structure):
    """mirt_scene_layout_info"""
    _fields_ = [("encloses", C.c_int32), ("ordered", C.c_int32), ("leaf_big", C.c_int32),
                ("r_max", C.c_float), ("c_max", C.c_float), ("o_bound", C.c_float),
                ("num_pnodes", C.c_uint32), ("num_hnodes", C.c_uint32), ("num_leaves", C.c_uint32),
                ("wide_root", C.c_uint32), ("leaf_box_off", C.c_uint64)]


class MultiStats(C.Structure):
    """mirt_multi_stats (include/mirt_multi.h)"""
    _fields_ = [("launches", C.c_uint64), ("comm_inits", C.c_uint64), ("rccl_groups", C.c_uint64),
                ("rccl_sends", C.c_uint64), ("rccl_recvs", C.c_uint64), ("rccl_bytes", C.c_uint64),
                ("device_copies", C.c_uint64)]


def default_camera():
    """main.c:203-211: position (0,4,50), looking down -z, fov 45, yaw -pi."""
    cam = Camera()
    cam.position = Vec3(0.0, 4.0, 50.0)
    cam.forward = Vec3(0.0, 0.0, -1.0)
    cam.right = Vec3(1.0, 0.0, 0.0)
    cam.up = Vec3(0.0, 1.0, 0.0)
    cam.yaw = np.float32(-np.pi)
    cam.pitch = 0.0
    cam.fov = 45.0
    cam.move = 0
    return cam


def ptr(a):
    """ctypes void* of a contiguous numpy array (None passes through)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


# (name, restype, argtypes) of every symbol include/mirt.h declares.
P = C.c_void_p
I = C.c_int
SIGNATURES = [
    ("mirt_version", C.c_char_p, []),
    ("mirt_last_error", C.c_char_p, []),
    ("mirt_srand", None, [P, C.c_uint]),
    ("mirt_rand", I, [P]),
    ("mirt_scene_random", I, [P, P, I]),
    ("mirt_scene_benchmark", I, [P, P, I, C.c_float]),
    ("mirt_bench_rays", I, [P, P, I]),
    ("mirt_camera_default", None, [P]),
    ("mirt_camera_update", None, [P]),
    ("mirt_build_bvh_node", P, [P, I, I, I]),
    ("mirt_free_bvh", None, [P]),
    ("mirt_bvh_count", I, [P]),
    ("mirt_bvh_flatten", I, [P, P, P, I]),
    ("mirt_bvh_build_flat", I, [P, I, I, I, C.POINTER(P), C.POINTER(I)]),
    ("mirt_bvh_free_flat", None, [P]),
    ("mirt_bvh_validate_flat", I, [P, I, I]),
    ("mirt_bvh_build_flat_cached", I, [C.c_char_p, P, I, I, I, C.POINTER(P), C.POINTER(I), C.POINTER(I)]),
    ("mirt_create", I, [I, C.POINTER(P)]),
    ("mirt_destroy", None, [P]),
    ("mirt_scene_upload", I, [P, P, I, P]),
    ("mirt_scene_upload_flat", I, [P, P, I, P, I]),
    ("mirt_bvh_build_flat_device", I, [P, P, I, I, I, C.POINTER(P), C.POINTER(I)]),
    ("mirt_last_build_stats", I, [P, P]),
    ("mirt_last_build_finish", I, [P, P]),
    ("mirt_build_partition_probe", I, [P, P, I, P, I, P, P]),
    ("mirt_scene_layout", C.c_int64, [P, I, P, I, I, P, C.c_size_t, P]),
    ("mirt_scene_build_device", I, [P, P, I, I, I, I, P]),
    ("mirt_scene_upload_flat_device", I, [P, P, I, P, I]),
    ("mirt_last_scene_build_stats", I, [P, P]),
    ("mirt_scene_resident_layout", C.c_int64, [P, I, P, C.c_size_t, P]),
    ("mirt_bvh_refit_flat", I, [P, I, P, I, I]),
    ("mirt_scene_refit_device", I, [P, P, I, I, P]),
    ("mirt_scene_refit_device_ptr", I, [P, P, I, I, P]),
    ("mirt_last_refit_stats", I, [P, P]),
    ("mirt_bvh_quality_flat", I, [P, I, I, P]),
    ("mirt_scene_quality", I, [P, P]),
    ("mirt_scene_update_device", I, [P, P, I, I, I, C.c_double, P, P, P]),
    ("mirt_scene_update_device_ptr", I, [P, P, I, I, I, C.c_double, P, P, P]),
    ("mirt_shard_rows", I, [P, P]),
    ("mirt_render_frame", I, [P, P, P, P]),
    ("mirt_render_frame_device", I, [P, P, P, P, P, P]),
    ("mirt_render_frame_async", I, [P, P, P, P]),
    ("mirt_render_frame_planes", I, [P, P, P, P, P]),
    ("mirt_render_frame_planes_device", I, [P, P, P, P, P, P, P]),
    ("mirt_render_frame_planes_async", I, [P, P, P, P, P]),
    ("mirt_render_rays_device", I, [P, P, P, P, P, P, P]),
    ("mirt_render_rays", I, [P, P, P, P, P]),
    ("mirt_lens_rays", I, [P, P, P, P, P]),
    ("mirt_render_lens_frame", I, [P, P, P, P, P, P]),
    ("mirt_render_lens_frame_device", I, [P, P, P, P, P, P, P, P]),
    ("mirt_render_lens_frame_async", I, [P, P, P, P, P, P]),
    ("mirt_denoise_params_default", None, [P]),
    ("mirt_denoise_host", I, [I, I, P, P, I, P, P, P, P, P]),
    ("mirt_denoise_device", I, [P, I, I, P, P, I, P, P, P, P, P, P]),
    ("mirt_denoise", I, [P, I, I, P, P, I, P, P, P, P, P]),
    ("mirt_render_frame_denoised", I, [P, P, P, P, P, P, P]),
    ("mirt_reproject_params_default", None, [P]),
    ("mirt_reproject_host", I, [I, I, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_reproject_device", I, [P, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_reproject", I, [P, I, I, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_render_frame_reprojected", I, [P, P, P, P, P, P]),
    ("mirt_history_reset", I, [P]),
    ("mirt_history_stats_get", I, [P, P]),
    ("mirt_history_read", I, [P, P, C.c_size_t]),
    ("mirt_reproject_motion_host", I, [I, I, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_reproject_motion_device", I, [P, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_reproject_motion", I, [P, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_history_motion_get", I, [P, P]),
    ("mirt_denoise_var_params_default", None, [P]),
    ("mirt_reproject_moments_host", I, [I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_reproject_moments_device", I, [P, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_reproject_moments", I, [P, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    ("mirt_denoise_var_host", I, [I, I, P, P, P, P, P, P, P, P]),
    ("mirt_denoise_var_device", I, [P, I, I, P, P, P, P, P, P, P, P, P]),
    ("mirt_denoise_var", I, [P, I, I, P, P, P, P, P, P, P, P]),
    ("mirt_render_frame_reprojected_denoised", I, [P, P, P, P, P, P, P, P]),
    ("mirt_history_moments_read", I, [P, P, C.c_size_t]),
    ("mirt_ctx_wait", I, [P]),
    ("mirt_host_alloc", I, [C.c_size_t, C.POINTER(P)]),
    ("mirt_host_free", None, [P]),
    ("mirt_host_register", I, [P, C.c_size_t]),
    ("mirt_host_unregister", I, [P]),
    ("mirt_accum_download", I, [P, P, C.c_size_t]),
    ("mirt_ctx_share_accum", I, [P, P]),
    ("mirt_ctx_share_scene", I, [P, P]),
    ("mirt_ctx_scene_id", C.c_uint64, [P]),
    ("mirt_trace_rays", I, [P, P, I, I, I, C.c_uint64, C.c_uint32, P]),
    ("mirt_trace_rays_at", I, [P, P, I, I, I, C.c_uint64, C.c_uint32, C.c_uint32, P]),
    ("mirt_camera_rays_uv", I, [P, P, I, I, P, I, P]),
    ("mirt_bvh_overlay", I, [P, P, I, I, I, P]),
    ("mirt_intersect_rays", I, [P, P, I, I, P]),
    ("mirt_any_hit_rays", I, [P, P, I, I, P]),
    ("mirt_sphere_pairs", I, [P, P, P, I, P]),
    ("mirt_aabb_pairs", I, [P, P, P, I, P]),
    ("mirt_hemisphere_probe", I, [P, P, P, P, P, I, P, P]),
    ("mirt_coop_geometry", I, [I, C.c_uint64, P, P, P, P]),
    ("mirt_pixel_rows", I, [I, I, I, I, I, I, P, C.c_int64, P]),
    ("mirt_exact_t_pairs", I, [C.c_int64, P, P, P, P, P, P, P, P]),
    ("mirt_sqrt_form_sweep", I, [P, P, P]),
    ("mirt_box_form_pairs", I, [P, P, P, P, I, I, P]),
    ("mirt_sphere_form_pairs", I, [P, P, P, P, I, I, P]),
    ("mirt_camera_rays", I, [P, P, P, P]),
    ("mirt_count_frame", I, [P, P, P, P]),
    ("mirt_wave_stats", I, [P, P, P, P, I]),
    ("mirt_ctx_stream", P, [P]),
    ("mirt_last_kernel_ms", C.c_float, [P]),
    ("mirt_last_phase_ms", I, [P, C.POINTER(C.c_float)]),
    ("mirt_phase_log", I, [P, C.POINTER(C.c_float), I]),
    ("mirt_bounce_stats", I, [P, P, P, P, I]),
    ("mirt_set_option", I, [P, I, I]),
    ("mirt_get_option", I, [P, I]),
    ("mirt_primary_cache_stats_get", I, [P, P]),
    ("mirt_primary_cache_read", I, [P, P, P, C.c_size_t]),
    ("mirt_primary_cache_write", I, [P, P, P, C.c_size_t]),
    ("mirt_primary_scan_stats_get", I, [P, P]),
    ("mirt_pscan_camera", I, [P, I, I, P, P]),
    ("mirt_pscan_records", I, [P, I, I, P, C.c_int64, P, P, P]),
    # include/mirt_dropin.h: the per-ray surface
    ("mirt_dropin_init", I, [I, I, I]),
    ("mirt_dropin_release", None, []),
    ("mirt_dropin_rng", None, [C.c_uint64, C.c_uint32]),
    ("mirt_dropin_scene", I, [P, I]),
    ("mirt_dropin_invalidate", None, []),
    ("mirt_dropin_status", I, []),
    ("mirt_get_camera_ray", Ray, [P, C.c_float, C.c_float]),
    ("mirt_trace_ray", Rgba8, [Ray, P, I, I, P]),
    ("mirt_ray_sphere_intersect", HitRecord, [Ray, P]),
    ("mirt_ray_aabb_intersect", I, [Ray, Aabb]),
    ("mirt_ray_bvh_intersect", HitRecord, [Ray, P]),
    # include/mirt_multi.h: one frame loop over several GPUs (RCCL gather)
    ("mirt_multi_create", I, [P, I, I, I, C.POINTER(P)]),
    ("mirt_multi_destroy", None, [P]),
    ("mirt_multi_size", I, [P]),
    ("mirt_multi_lanes", I, [P]),
    ("mirt_multi_backend", C.c_char_p, [P]),
    ("mirt_multi_delivery", C.c_char_p, [P]),
    ("mirt_multi_failed", I, [P]),
    ("mirt_multi_ctx", P, [P, I, I]),
    ("mirt_multi_set_option", I, [P, I, I]),
    ("mirt_multi_get_option", I, [P, I]),
    ("mirt_multi_scene_upload", I, [P, P, I, P]),
    ("mirt_multi_scene_upload_flat", I, [P, P, I, P, I]),
    ("mirt_multi_scene_build_device", I, [P, P, I, I, I, I, P]),
    ("mirt_multi_scene_refit_device", I, [P, P, I, I]),
    ("mirt_multi_scene_update_device", I, [P, P, I, I, I, C.c_double, P, P, P]),
    ("mirt_multi_render_frame", I, [P, P, P, P]),
    ("mirt_multi_render_frame_async", I, [P, P, P, P]),
    ("mirt_multi_render_frames_async", I, [P, P, P, I, I, C.POINTER(P)]),
    ("mirt_multi_render_lens_frames_async", I, [P, P, P, P, I, I, C.POINTER(P)]),
    ("mirt_multi_wait", I, [P]),
    ("mirt_multi_get_stats", I, [P, P]),
    ("mirt_multi_read_gathered", I, [P, I, I, I, P, C.c_size_t]),
]

OPT_TRAVERSAL, OPT_FAST_SLAB, OPT_BLOCK_WAVES, OPT_DEFER, OPT_BOUNCE_THRESHOLD, OPT_PRUNE, OPT_ORDERED = (
    1, 2, 3, 4, 5, 6, 7)
OPT_BOUNCE_BLOCKS, OPT_QUAD_DRAIN, OPT_LEAF_BATCH, OPT_QUAD_BATCH, OPT_ZERO_COPY = 9, 11, 14, 15, 17
OPT_QUEUE_ORDER, OPT_DEBUG_STALL_MS = 18, 19
OPT_CONFIRM_ONCE, OPT_DEBUG_FAIL_CONFIRM = 21, 22
OPT_BUILD_FINISH = 23     # the device build's finish: 0 never, 1 automatic (default), 2..64 = F
OPT_PRIMARY_CACHE = 24    # a still camera's frames start from the stored primary hits: 0 off (default), 1 on
OPT_DENOISE_TILE = 26     # mirt_denoise*: passes of spacing 1 and 2 from an LDS tile with halo (1) or by direct loads (0)
OPT_HISTORY_MOTION = 27   # refits / updates record a link, reprojected frames carry their history over it: 0 off (default), 1 on
# mirt_primary_cache_stats: `last` (how the last frame met the cache) and `reason` (why it was no hit)
PCACHE_BYPASS, PCACHE_FILL, PCACHE_HIT = 0, 1, 2
PCACHE_KIND = {PCACHE_BYPASS: "bypass", PCACHE_FILL: "fill", PCACHE_HIT: "hit"}
PCACHE_REASON = {0: "", 1: "EMPTY", 2: "SCENE", 3: "CAMERA", 4: "GEOMETRY", 5: "OFF", 6: "SCHEDULE", 7: "JITTER",
                 8: "PLANES", 9: "RAYS"}
# MIRT_PCACHE_LENS, which mirt.h writes as MIRT_PCACHE_RAYS + 1 (PCACHE_REASON holds the reasons written as literals)
PCACHE_LENS = 10
PCACHE_REASON_NAME = {**PCACHE_REASON, PCACHE_LENS: "LENS"}
OPT_PRIMARY_SCAN = 28     # the camera pass by a depth-sorted tile scan: 0 off, 1 on, 2 automatic (default)
OPT_PRIMARY_SCAN_BUDGET = 29   # chunks of 64 records a tile with a pixel still without a hit reads before it takes the packet walk (default 256)
OPT_PRIMARY_SCAN_REBUILD = 30  # not a supported setting, a measurement hook: 1 = the scan's per-camera data rebuilt by every frame
# mirt_primary_scan_stats: `last` (how the last frame met the scan) and `reason` (why it was a bypass)
PSCAN_BYPASS, PSCAN_SCAN = 0, 1
PSCAN_KIND = {PSCAN_BYPASS: "bypass", PSCAN_SCAN: "scan"}
PSCAN_REASON = {0: "", 1: "OFF", 2: "CACHE", 3: "SCHEDULE", 4: "JITTER", 5: "PLANES", 6: "RAYS", 7: "LENS", 8: "TREE",
                9: "SHARD", 10: "SIZE", 11: "CAMERA", 12: "SPARSE"}
PSCAN_CAM = {0: "ok", 1: "nonfinite", 2: "degenerate", 3: "wide"}   # mirt_pscan_camera / mirt_pscan_records
BOUNCE_STATS_WORDS = 23   # mirt.h MIRT_BOUNCE_STATS_WORDS
TRAV_TILE, TRAV_WAVEFRONT = 0, 5
BOX_FORM_SLAB, BOX_FORM_SLAB_BOX, BOX_FORM_CONS, BOX_FORM_CONS_BOUNCE, BOX_FORM_CONS_CAMERA = 0, 1, 2, 3, 4
MULTI_COPY, MULTI_HOST_DIRECT, MULTI_QUEUE_AHEAD = 1, 2, 4
MULTI_FULL_GRID = 1
MULTI_OPT_TIMEOUT_MS, MULTI_OPT_EMULATE_WORLD, MULTI_OPT_EMULATE_RANK, MULTI_OPT_DIRECT_COPY = 256, 257, 258, 259
MULTI_OPT_COPY_STREAM = 260
MULTI_OPT_GATHER_SELF, MULTI_OPT_LEAD_SKIP = 261, 262

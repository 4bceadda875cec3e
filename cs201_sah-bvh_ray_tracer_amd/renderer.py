"""Python host side of the render path, mirroring the reference's interface.

Reference call surface -> here (all compute goes through libmirt.so):

  srand / rand (glibc, main.c:90)             RandState
  create_random_sphere x N (sphere.c:52-59,   create_random_spheres(n, seed)
    main.c:218-221)
  create_benchmark_sphere (sphere.c:34-41,    create_benchmark_spheres(n, seed)
    benchmark.c:307-314)
  camera init (main.c:203-211) / camera_update default_camera() / camera_update(cam)
    (camera.c:10-18)
  build_bvh_node (bvh.c:117-209)               build_bvh(spheres, start, end, depth) -> Bvh
                                               build_bvh_cached(path, spheres, ...) (tree cache file)
                                               build_bvh_node(...) -> pointer tree (drop-in)
  get_camera_ray (ray.c:17-32) per pixel       Renderer.get_camera_rays(cam, W, H)
  trace_ray (renderer.c:21-77) per ray         Renderer.trace_ray(rays, depth, ...)
  pixel loop main.c:356-374 / 379-408          Renderer.render_frame(cam, W, H, ...)
  ray_bvh_intersect (hit.c:91-109)             Renderer.ray_bvh_intersect(rays)
  ray_sphere_intersect (hit.c:19-39)           Renderer.ray_sphere_intersect(rays, spheres)
  ray_aabb_intersect (hit.c:49-82)             Renderer.ray_aabb_intersect(rays, boxes)

Errors raise MirtError (the reference only printf's); there is no CPU path.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .lib import MirtError, check, load

ptr = abi.ptr


class RandState:
    """glibc srand()/rand() (TYPE_3), restated in libmirt."""

    def __init__(self, seed=1):
        self.st = abi.RandState()
        load().mirt_srand(C.byref(self.st), seed)

    def rand(self):
        return load().mirt_rand(C.byref(self.st))


def create_random_spheres(n, seed=1, state=None):
    """srand(seed) then n x create_random_sphere() (main.c:218-221)."""
    st = state or RandState(seed)
    out = np.zeros(n, abi.SPHERE)
    check(load().mirt_scene_random(C.byref(st.st), ptr(out), n), "mirt_scene_random")
    return out


def create_benchmark_spheres(n, seed=1, world_size=1000.0, state=None):
    """srand(seed) then the benchmark.c:307-314 sphere loop."""
    st = state or RandState(seed)
    out = np.zeros(n, abi.SPHERE)
    check(load().mirt_scene_benchmark(C.byref(st.st), ptr(out), n, world_size), "mirt_scene_benchmark")
    return out


def create_bench_rays(n, state):
    """n rays of benchmark.c:176-185 (origin 0, normalised random direction)
    drawn from `state` (a RandState continuing the scene's glibc stream)."""
    out = np.zeros(n, abi.RAY)
    check(load().mirt_bench_rays(C.byref(state.st), ptr(out), n), "mirt_bench_rays")
    return out


def default_camera():
    cam = abi.Camera()
    load().mirt_camera_default(C.byref(cam))
    return cam


def camera_update(cam):
    load().mirt_camera_update(C.byref(cam))
    return cam


class Bvh:
    """A flattened tree (abi.NODE array) plus the leaf sphere counts it came from."""

    def __init__(self, nodes):
        self.nodes = nodes

    def __len__(self):
        return len(self.nodes)


def build_bvh(spheres, start=0, end=None, depth=0):
    """build_bvh_node (bvh.c:117) straight into the flat layout; reorders
    `spheres` in place exactly like the reference."""
    assert spheres.dtype == abi.SPHERE and spheres.flags["C_CONTIGUOUS"]
    end = len(spheres) if end is None else end
    out = C.c_void_p()
    cnt = C.c_int()
    L = load()
    check(L.mirt_bvh_build_flat(ptr(spheres), start, end, depth, C.byref(out), C.byref(cnt)), "mirt_bvh_build_flat")
    try:
        buf = (C.c_char * (cnt.value * abi.NODE.itemsize)).from_address(out.value)
        nodes = np.frombuffer(bytes(buf), dtype=abi.NODE).copy()
    finally:
        L.mirt_bvh_free_flat(out)
    return Bvh(nodes)


def validate_bvh(nodes, num_spheres):
    """mirt_bvh_validate_flat: raises MirtError unless `nodes` (abi.NODE) is a
    well-formed flat pre-order tree over num_spheres spheres."""
    nodes = np.ascontiguousarray(nodes, dtype=abi.NODE)
    check(load().mirt_bvh_validate_flat(ptr(nodes) if len(nodes) else None, len(nodes), num_spheres),
          "mirt_bvh_validate_flat")


def refit_bvh(tree, spheres, end=None):
    """mirt_bvh_refit_flat on a copy: the Bvh of `tree` (a Bvh or an abi.NODE
    array) with every box recomputed bottom-up from `spheres`, which are in the
    scene's order; sphere and skip of every node stay. `end` is one past the
    last sphere the tree was built over (default: all of them). Host only.
    Raises MirtError if the leaves' spheres do not increase in pre-order or
    `end` does not lie behind the last of them."""
    spheres = np.ascontiguousarray(spheres, abi.SPHERE)
    nodes = np.array(tree.nodes if isinstance(tree, Bvh) else tree, dtype=abi.NODE, order="C", copy=True)
    end = len(spheres) if end is None else end
    check(load().mirt_bvh_refit_flat(ptr(nodes) if len(nodes) else None, len(nodes),
                                     ptr(spheres) if len(spheres) else None, len(spheres), end),
          "mirt_bvh_refit_flat")
    return Bvh(nodes)


def _fields(st):
    """A ctypes struct as a dict (nested structs as dicts)."""
    return {k: _fields(getattr(st, k)) if issubclass(t, C.Structure) else getattr(st, k) for k, t in st._fields_}


def bvh_quality(tree, num_spheres):
    """mirt_bvh_quality_flat: the SAH quality of `tree` (a Bvh or an abi.NODE
    array) over num_spheres spheres, as a dict of the mirt_tree_quality fields:
    inner_area / leaf_area (the two sums), overhead (their ratio), cost
    (0.125 * overhead + 1), root_area, inner_nodes, leaves, dead_leaves,
    clamped, degenerate. cost over the cost at build time says how far a refit
    tree has decayed. Host only; raises MirtError for a malformed tree."""
    nodes = np.ascontiguousarray(tree.nodes if isinstance(tree, Bvh) else tree, dtype=abi.NODE)
    q = abi.TreeQuality()
    check(load().mirt_bvh_quality_flat(ptr(nodes) if len(nodes) else None, len(nodes), num_spheres, C.byref(q)),
          "mirt_bvh_quality_flat")
    return _fields(q)


def scene_layout(spheres, tree=None):
    """mirt_scene_layout: the device layouts an upload of `spheres` with `tree`
    (a Bvh, an abi.NODE array or None) would send, computed on the host -- no
    Renderer, no GPU. Returns (info, parts): info the mirt_scene_layout_info
    fields as a dict, parts one numpy array per abi.LAYOUT_PARTS name."""
    spheres = np.ascontiguousarray(spheres, abi.SPHERE)
    nodes = np.zeros(0, abi.NODE) if tree is None else tree.nodes if isinstance(tree, Bvh) else tree
    nodes = np.ascontiguousarray(nodes, abi.NODE)
    L = load()
    raw = abi.SceneLayoutInfo()
    args = (ptr(spheres) if len(spheres) else None, len(spheres), ptr(nodes) if len(nodes) else None, len(nodes))
    check(L.mirt_scene_layout(*args, 0, None, 0, C.byref(raw)), "mirt_scene_layout")
    count = dict(dnodes=len(nodes), geo=len(spheres) + 1, color=len(spheres) + 1, pnodes=raw.num_pnodes,
                 hnodes=raw.num_hnodes, haux=raw.num_hnodes, leaf_geo=raw.num_leaves, leaf_box=raw.num_leaves,
                 ndepth=max(len(nodes), 1))
    parts = {}
    for part, (name, dtype) in enumerate(abi.LAYOUT_PARTS):
        out = np.zeros(count[name], dtype)
        size = check(L.mirt_scene_layout(*args, part, ptr(out), out.nbytes, None), "mirt_scene_layout")
        if size != out.nbytes:
            raise MirtError(f"mirt_scene_layout: part {name} is {size} bytes, expected {out.nbytes}")
        parts[name] = out
    return {name: getattr(raw, name) for name, _ in raw._fields_}, parts


def build_bvh_cached(path, spheres, start=0, end=None, depth=0):
    """build_bvh through a flattened-tree cache file (mirt_bvh_build_flat_cached):
    returns (Bvh, cached) with cached 1 = loaded from `path`, 0 = built and
    written, -1 = built, file not written. `spheres` ends up reordered exactly
    as build_bvh leaves it either way."""
    assert spheres.dtype == abi.SPHERE and spheres.flags["C_CONTIGUOUS"]
    end = len(spheres) if end is None else end
    out = C.c_void_p()
    cnt = C.c_int()
    cached = C.c_int()
    L = load()
    check(L.mirt_bvh_build_flat_cached(os.fsencode(path), ptr(spheres), start, end, depth, C.byref(out),
                                       C.byref(cnt), C.byref(cached)), "mirt_bvh_build_flat_cached")
    try:
        buf = (C.c_char * (cnt.value * abi.NODE.itemsize)).from_address(out.value)
        nodes = np.frombuffer(bytes(buf), dtype=abi.NODE).copy()
    finally:
        L.mirt_bvh_free_flat(out)
    return Bvh(nodes), cached.value


def build_bvh_node(spheres, start=0, end=None, depth=0):
    """Drop-in build_bvh_node: returns the reference-layout pointer tree
    (free with free_bvh)."""
    end = len(spheres) if end is None else end
    root = load().mirt_build_bvh_node(ptr(spheres), start, end, depth)
    if not root:
        raise MirtError(load().mirt_last_error().decode())
    return root


def free_bvh(root):
    load().mirt_free_bvh(root)


def flatten_bvh(root, spheres):
    """Flatten a pointer tree (ours or the reference's) into a Bvh."""
    L = load()
    n = L.mirt_bvh_count(root)
    nodes = np.zeros(n, abi.NODE)
    check(L.mirt_bvh_flatten(root, ptr(spheres), ptr(nodes), n), "mirt_bvh_flatten")
    return Bvh(nodes)


def frame_desc(width, height, depth=5, use_bvh=True, seed=1, sample=0, accumulate=False, frames=1,
               row_block=8, shard=0, num_shards=1, samples=1, jitter=False, lead_skip=0):
    fd = abi.FrameDesc()
    fd.width, fd.height, fd.max_depth, fd.use_bvh = width, height, depth, int(use_bvh)
    fd.seed, fd.sample, fd.accumulate, fd.frames = seed, sample, int(accumulate), frames
    fd.row_block, fd.shard, fd.num_shards = row_block, shard, num_shards
    fd.samples = samples
    fd.jitter = int(jitter)
    fd.lead_skip = lead_skip
    return fd


def shard_rows(fd):
    """Image rows a shard renders, in its compacted order."""
    L = load()
    n = check(L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
    rows = np.zeros(n, np.int32)
    L.mirt_shard_rows(C.byref(fd), ptr(rows))
    return rows


def host_register(arr):
    """Page-lock a C-contiguous numpy array in place (mirt_host_register):
    blocking frames copied into it become one DMA. host_unregister before the
    array is released."""
    assert arr.flags["C_CONTIGUOUS"]
    check(load().mirt_host_register(ptr(arr), arr.nbytes), "mirt_host_register")


def host_unregister(arr):
    check(load().mirt_host_unregister(ptr(arr)), "mirt_host_unregister")


class HostBuffer:
    """Page-locked host memory (mirt_host_alloc) viewed as a numpy array."""

    def __init__(self, shape, dtype=np.uint8):
        self.L = load()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(self.L.mirt_host_alloc(nbytes, C.byref(p)), "mirt_host_alloc")
        self.p = p
        buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self.p:
            self.array = None
            self.L.mirt_host_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def primary_scan_stats(handle):
    """mirt_primary_scan_stats of a mirt_ctx handle, as a dict with "last"
    ("scan" / "bypass") and "reason" named. Waits for the ctx's frames when the
    last one was scanned (the device counters are copied here only)."""
    st = abi.PrimaryScanStats()
    check(load().mirt_primary_scan_stats_get(handle, C.byref(st)), "mirt_primary_scan_stats_get")
    out = _fields(st)
    out["last"] = abi.PSCAN_KIND[st.last]
    out["reason"] = abi.PSCAN_REASON[st.reason]
    return out


def primary_cache_stats(handle):
    """mirt_primary_cache_stats of a mirt_ctx handle (a Renderer's .h, or
    MultiRenderer.ctx(lane, rank)), as a dict with "last" and "reason" named."""
    st = abi.PrimaryCacheStats()
    check(load().mirt_primary_cache_stats_get(handle, C.byref(st)), "mirt_primary_cache_stats_get")
    out = _fields(st)
    out["last"] = abi.PCACHE_KIND[st.last]
    out["reason"] = abi.PCACHE_REASON_NAME[st.reason]
    return out


class Renderer:
    """One device context (mirt_ctx) with a resident scene."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        check(self.L.mirt_create(device, C.byref(h)), "mirt_create")
        self.h = h
        self.device = device
        self.num_spheres = -1

    def close(self):
        if self.h:
            self.L.mirt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- scene
    def upload(self, spheres, bvh=None):
        """Upload the (post-build) spheres and a Bvh, a pointer tree, or None."""
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        if bvh is None:
            check(self.L.mirt_scene_upload_flat(self.h, ptr(spheres), len(spheres), None, 0), "upload")
        elif isinstance(bvh, Bvh):
            check(self.L.mirt_scene_upload_flat(self.h, ptr(spheres), len(spheres), ptr(bvh.nodes), len(bvh.nodes)),
                  "mirt_scene_upload_flat")
        else:
            check(self.L.mirt_scene_upload(self.h, ptr(spheres), len(spheres), bvh), "mirt_scene_upload")
        self.num_spheres = len(spheres)

    def build_bvh(self, spheres, start=0, end=None, depth=0):
        """build_bvh on this context's device (mirt_bvh_build_flat_device): the
        same Bvh and the same in-place reordering of `spheres`, bit for bit.
        Needs no uploaded scene; last_build_stats() says how it went."""
        assert spheres.dtype == abi.SPHERE and spheres.flags["C_CONTIGUOUS"]
        end = len(spheres) if end is None else end
        out = C.c_void_p()
        cnt = C.c_int()
        check(self.L.mirt_bvh_build_flat_device(self.h, ptr(spheres), start, end, depth, C.byref(out), C.byref(cnt)),
              "mirt_bvh_build_flat_device")
        try:
            buf = (C.c_char * (cnt.value * abi.NODE.itemsize)).from_address(out.value)
            nodes = np.frombuffer(bytes(buf), dtype=abi.NODE).copy()
        finally:
            self.L.mirt_bvh_free_flat(out)
        return Bvh(nodes)

    def last_build_stats(self):
        """mirt_build_stats of the last build_bvh on this context, as a dict:
        on_device (0: the input was declined and the host builder ran), levels,
        nodes, device_ms (the kernels), total_ms (call to return)."""
        st = abi.BuildStats()
        check(self.L.mirt_last_build_stats(self.h, C.byref(st)), "mirt_last_build_stats")
        return {k: getattr(st, k) for k, _ in abi.BuildStats._fields_}

    def last_build_finish(self):
        """mirt_build_finish_stats of this context's last device build
        (build_bvh, build_scene or a rebuilding update_scene), as a dict: range
        (F in effect, 0: off), round (the level round at which one wave per
        open node took over, -1: it did not), subtrees, nodes, moved (always
        0), finish_ms."""
        st = abi.BuildFinishStats()
        check(self.L.mirt_last_build_finish(self.h, C.byref(st)), "mirt_last_build_finish")
        return {k: getattr(st, k) for k, _ in abi.BuildFinishStats._fields_}

    def build_scene(self, spheres, start=0, end=None, depth=0):
        """Spheres in, scene resident (mirt_scene_build_device): the tree of
        spheres[start:end] is built and laid out on this context's device and
        installed, as build_bvh + upload would leave it, without the tree
        leaving the device. `spheres` is not written; returns the spheres as
        reordered (what hit records index). last_scene_build_stats() says how
        it went."""
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        end = len(spheres) if end is None else end
        out = np.zeros(len(spheres), abi.SPHERE)
        check(self.L.mirt_scene_build_device(self.h, ptr(spheres), len(spheres), start, end, depth, ptr(out)),
              "mirt_scene_build_device")
        self.num_spheres = len(spheres)
        return out

    def upload_device(self, spheres, bvh=None):
        """upload() of a Bvh (or an abi.NODE array, or None) with the layouts
        derived on the device (mirt_scene_upload_flat_device): only the raw
        spheres and nodes cross the link."""
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        nodes = np.zeros(0, abi.NODE) if bvh is None else bvh.nodes if isinstance(bvh, Bvh) else bvh
        nodes = np.ascontiguousarray(nodes, abi.NODE)
        check(self.L.mirt_scene_upload_flat_device(self.h, ptr(spheres) if len(spheres) else None, len(spheres),
                                                   ptr(nodes) if len(nodes) else None, len(nodes)),
              "mirt_scene_upload_flat_device")
        self.num_spheres = len(spheres)

    def resident_layout(self):
        """mirt_scene_resident_layout: the layouts of the scene this context
        holds, read back from the device; (info, parts) shaped like
        scene_layout()'s."""
        raw = abi.SceneLayoutInfo()
        size = {}
        for part, (name, dtype) in enumerate(abi.LAYOUT_PARTS):
            size[name] = check(self.L.mirt_scene_resident_layout(self.h, part, None, 0, C.byref(raw)),
                               "mirt_scene_resident_layout")
        parts = {}
        for part, (name, dtype) in enumerate(abi.LAYOUT_PARTS):
            if size[name] % dtype.itemsize:
                raise MirtError(f"mirt_scene_resident_layout: part {name} is {size[name]} bytes")
            out = np.zeros(size[name] // dtype.itemsize, dtype)
            got = check(self.L.mirt_scene_resident_layout(self.h, part, ptr(out), out.nbytes, None),
                        "mirt_scene_resident_layout")
            if got != out.nbytes:
                raise MirtError(f"mirt_scene_resident_layout: part {name} is {got} bytes, expected {out.nbytes}")
            parts[name] = out
        return {name: getattr(raw, name) for name, _ in raw._fields_}, parts

    def last_scene_build_stats(self):
        """mirt_scene_build_stats of the last build_scene on this context, as a
        dict: on_device (0: input declined, host build and host upload ran),
        levels, nodes, build_ms, layout_ms, total_ms."""
        st = abi.SceneBuildStats()
        check(self.L.mirt_last_scene_build_stats(self.h, C.byref(st)), "mirt_last_scene_build_stats")
        return {k: getattr(st, k) for k, _ in abi.SceneBuildStats._fields_}

    def refit_scene(self, spheres, end=None, return_nodes=False):
        """Refit the resident scene to `spheres` on the device
        (mirt_scene_refit_device): the tree's topology stays, its boxes and the
        device layouts are recomputed, as refit_bvh + upload would leave them.
        `spheres` holds as many spheres as the resident scene, in its order: a
        numpy abi.SPHERE array, or a torch tensor on this context's device
        (uint8, 20 bytes per sphere, contiguous), which is read in place on the
        context's stream (mirt_scene_refit_device_ptr). `end` is one past the
        last sphere the tree was built over (default: all). Returns the refit
        Bvh if return_nodes. last_refit_stats() says how it went."""
        nodes = None
        if return_nodes:
            info = abi.SceneLayoutInfo()
            size = check(self.L.mirt_scene_resident_layout(self.h, 0, None, 0, C.byref(info)),
                         "mirt_scene_resident_layout")
            nodes = np.zeros(size // abi.DNODE.itemsize, abi.NODE)
        out = ptr(nodes) if nodes is not None and len(nodes) else None
        if isinstance(spheres, np.ndarray) or not hasattr(spheres, "data_ptr"):
            spheres = np.ascontiguousarray(spheres, abi.SPHERE)
            n = len(spheres)
            end = n if end is None else end
            check(self.L.mirt_scene_refit_device(self.h, ptr(spheres) if n else None, n, end, out),
                  "mirt_scene_refit_device")
        else:
            nbytes = spheres.numel() * spheres.element_size()
            if not spheres.is_cuda or spheres.device.index != self.device or not spheres.is_contiguous() \
                    or nbytes % abi.SPHERE.itemsize:
                raise MirtError("refit_scene: the tensor must be contiguous, on this context's device and hold "
                                "20-byte spheres")
            n = nbytes // abi.SPHERE.itemsize
            end = n if end is None else end
            import torch
            torch.cuda.current_stream(spheres.device).synchronize()  # the tensor's producer: another stream
            check(self.L.mirt_scene_refit_device_ptr(self.h, C.c_void_p(spheres.data_ptr()) if n else None, n, end,
                                                     out), "mirt_scene_refit_device_ptr")
        return Bvh(nodes) if return_nodes else None

    def last_refit_stats(self):
        """mirt_refit_stats of the last refit_scene on this context, as a dict:
        on_device (0: input declined, host refit and host upload ran), nodes,
        refit_ms, layout_ms, total_ms."""
        st = abi.RefitStats()
        check(self.L.mirt_last_refit_stats(self.h, C.byref(st)), "mirt_last_refit_stats")
        return {k: getattr(st, k) for k, _ in abi.RefitStats._fields_}

    def scene_quality(self):
        """mirt_scene_quality: bvh_quality() of the resident tree, measured by
        a kernel on this context's device; the same dict, bit for bit."""
        q = abi.TreeQuality()
        check(self.L.mirt_scene_quality(self.h, C.byref(q)), "mirt_scene_quality")
        return _fields(q)

    def update_scene(self, spheres, start=0, end=None, max_decay=0.0):
        """Refit the resident scene to `spheres` (a numpy abi.SPHERE array in
        the scene's order, or a torch tensor on this context's device as for
        refit_scene: then mirt_scene_update_device_ptr reads it in place, and
        reordered (uint8, n x 20) and perm (int32) come back as tensors on
        that device) and rebuild it instead when the refit tree's cost
        has grown past max_decay times the cost of the tree the last
        update_scene installed (mirt_scene_update_device; max_decay <= 0 never
        rebuilds). Returns (reordered, perm, result): the spheres in the order
        the scene now holds them, reordered[i] == spheres[perm[i]] (the
        identity unless rebuilt), and the mirt_update_result fields as a dict
        (rebuilt, on_device, base_cost, cost, decay, installed, total_ms)."""
        if not isinstance(spheres, np.ndarray) and hasattr(spheres, "data_ptr"):
            import torch
            nbytes = spheres.numel() * spheres.element_size()
            if not spheres.is_cuda or spheres.device.index != self.device or not spheres.is_contiguous() \
                    or nbytes % abi.SPHERE.itemsize:
                raise MirtError("update_scene: the tensor must be contiguous, on this context's device and hold "
                                "20-byte spheres")
            n = nbytes // abi.SPHERE.itemsize
            end = n if end is None else end
            reordered = torch.zeros((n, abi.SPHERE.itemsize), dtype=torch.uint8, device=spheres.device)
            perm = torch.zeros(n, dtype=torch.int32, device=spheres.device)
            res = abi.UpdateResult()
            torch.cuda.current_stream(spheres.device).synchronize()  # the tensors' producers: another stream
            check(self.L.mirt_scene_update_device_ptr(
                self.h, C.c_void_p(spheres.data_ptr()) if n else None, n, start, end, max_decay,
                C.c_void_p(reordered.data_ptr()) if n else None, C.c_void_p(perm.data_ptr()) if n else None,
                C.byref(res)), "mirt_scene_update_device_ptr")
            return reordered, perm, _fields(res)
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        n = len(spheres)
        end = n if end is None else end
        reordered = np.zeros(n, abi.SPHERE)
        perm = np.zeros(n, np.int32)
        res = abi.UpdateResult()
        check(self.L.mirt_scene_update_device(self.h, ptr(spheres) if n else None, n, start, end, max_decay,
                                              ptr(reordered) if n else None, ptr(perm) if n else None, C.byref(res)),
              "mirt_scene_update_device")
        return reordered, perm, _fields(res)

    # ---- frames
    def render_frame(self, cam, width, height, depth=5, use_bvh=True, seed=1, sample=0, accumulate=False,
                     frames=1, row_block=8, shard=0, num_shards=1, samples=1, jitter=False):
        """main.c:356-374 (fresh) or main.c:379-408 (accumulate) for one shard;
        returns (rows, width, 4) uint8 in the shard's row order. samples > 1:
        that many successive frames (RNG samples sample, sample + 1, ...) in
        one launch, accumulated; returns the display after the last."""
        fd = frame_desc(width, height, depth, use_bvh, seed, sample, accumulate, frames, row_block, shard,
                        num_shards, samples, jitter)
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        out = np.zeros((n, width, 4), np.uint8)
        check(self.L.mirt_render_frame(self.h, C.byref(cam), C.byref(fd), ptr(out)), "mirt_render_frame")
        return out

    def render_frame_into(self, cam, width, height, out, depth=5, use_bvh=True, seed=1, sample=0, accumulate=False,
                          frames=1, samples=1, jitter=False):
        """render_frame into a caller-given C-contiguous uint8 array (pageable,
        registered or page-locked) of height x width x 4."""
        fd = frame_desc(width, height, depth, use_bvh, seed, sample, accumulate, frames, 8, 0, 1, samples, jitter)
        assert out.flags["C_CONTIGUOUS"] and out.nbytes >= width * height * 4
        check(self.L.mirt_render_frame(self.h, C.byref(cam), C.byref(fd), ptr(out)), "mirt_render_frame")
        return out

    def render_frame_async(self, cam, fd, out):
        """Enqueue the frame and its D2H copy into `out` (a HostBuffer, or any
        C-contiguous uint8 array of the shard's rows x width x 4) on the ctx's
        own stream; `out` is complete after wait()."""
        arr = out.array if isinstance(out, HostBuffer) else out
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        if arr.nbytes < n * fd.width * 4 or not arr.flags["C_CONTIGUOUS"]:
            raise MirtError(f"render_frame_async: output holds {arr.nbytes} bytes, the shard needs {n * fd.width * 4}")
        check(self.L.mirt_render_frame_async(self.h, C.byref(cam), C.byref(fd), ptr(arr)), "mirt_render_frame_async")

    def wait(self):
        """Block until the ctx's stream is idle (mirt_ctx_wait)."""
        check(self.L.mirt_ctx_wait(self.h), "mirt_ctx_wait")

    def render_frame_device(self, cam, fd, d_out, d_acc=None, stream=None):
        """Enqueue a frame into device memory (integer device pointers)."""
        check(self.L.mirt_render_frame_device(self.h, C.byref(cam), C.byref(fd), C.c_void_p(d_out),
                                              C.c_void_p(d_acc) if d_acc else None,
                                              C.c_void_p(stream or 0)), "mirt_render_frame_device")

    # ---- frames with primary-hit planes (mirt_primary_planes)
    PLANES = {"t": (np.float32, ()), "sphere": (np.int32, ()), "normal": (np.float32, (3,))}

    @classmethod
    def _planes_struct(cls, ptrs, fn):
        """abi.PrimaryPlanes from {name: integer pointer}; unknown names are refused."""
        bad = [k for k in ptrs if k not in cls.PLANES]
        if bad:
            raise MirtError(f"{fn}: no such plane {bad[0]!r} (have {', '.join(cls.PLANES)})")
        return abi.PrimaryPlanes(**{k: int(v) for k, v in ptrs.items() if v})

    def render_frame_planes(self, cam, width, height, planes=("t", "sphere", "normal"), **frame_desc_args):
        """render_frame (frame_desc's keyword arguments) that also returns each
        pixel's primary hit, stored by the frame's own camera walk: (rgba, dict)
        with the asked-for planes "t" (float32; 0 on a miss), "sphere" (int32
        index into the resident spheres; -1 on a miss) and "normal" (float32 x 3;
        0 on a miss), each (rows, width[, 3]) in the shard's row order -- with
        samples > 1 (samples, rows, width[, 3]), frame j's own hits in slab j,
        while rgba is the display after the last frame."""
        fd = frame_desc(width, height, **frame_desc_args)
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        out = np.zeros((n, width, 4), np.uint8)
        lead = (fd.samples, n, width) if fd.samples > 1 else (n, width)
        self._planes_struct(dict.fromkeys(planes, 0), "render_frame_planes")   # the names
        bufs = {k: np.zeros(lead + self.PLANES[k][1], self.PLANES[k][0]) for k in planes}
        pl = self._planes_struct({k: b.ctypes.data for k, b in bufs.items()}, "render_frame_planes")
        check(self.L.mirt_render_frame_planes(self.h, C.byref(cam), C.byref(fd), ptr(out), C.byref(pl)),
              "mirt_render_frame_planes")
        return out, bufs

    def render_frame_planes_device(self, cam, fd, d_out, d_planes, d_acc=None, stream=None):
        """render_frame_device that also stores the planes: d_planes maps "t" /
        "sphere" / "normal" to integer device pointers (samples * rows * width
        elements each, three floats per element for "normal")."""
        pl = self._planes_struct(d_planes, "render_frame_planes_device")
        check(self.L.mirt_render_frame_planes_device(self.h, C.byref(cam), C.byref(fd), C.c_void_p(d_out),
                                                     C.c_void_p(d_acc) if d_acc else None, C.byref(pl),
                                                     C.c_void_p(stream or 0)), "mirt_render_frame_planes_device")

    def render_frame_planes_async(self, cam, fd, out, planes):
        """render_frame_async that also copies the planes, behind the frame on
        the ctx's stream: `planes` maps "t" / "sphere" / "normal" to HostBuffers
        or C-contiguous arrays of samples * rows * width elements (float32,
        int32, float32 x 3); all are complete after wait()."""
        arr = out.array if isinstance(out, HostBuffer) else out
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        if arr.nbytes < n * fd.width * 4 or not arr.flags["C_CONTIGUOUS"]:
            raise MirtError(f"render_frame_planes_async: output holds {arr.nbytes} bytes, the shard needs "
                            f"{n * fd.width * 4}")
        ptrs = {}
        for k, buf in planes.items():
            a = buf.array if isinstance(buf, HostBuffer) else buf
            need = max(fd.samples, 1) * n * fd.width * (12 if k == "normal" else 4)
            if a.nbytes < need or not a.flags["C_CONTIGUOUS"]:
                raise MirtError(f"render_frame_planes_async: plane {k!r} holds {a.nbytes} bytes, the frame needs {need}")
            ptrs[k] = a.ctypes.data
        pl = self._planes_struct(ptrs, "render_frame_planes_async")
        check(self.L.mirt_render_frame_planes_async(self.h, C.byref(cam), C.byref(fd), ptr(arr), C.byref(pl)),
              "mirt_render_frame_planes_async")

    # ---- ray frames (the caller's camera rays)
    def render_rays(self, rays, width, height, planes=None, **frame_desc_args):
        """render_frame (frame_desc's keyword arguments) of caller-given camera
        rays (mirt_render_rays): `rays` is an abi.RAY array of samples * rows *
        width elements, indexed as the colour output and the planes are (slab j
        = frame j's rays, rows in the shard's order), used as given. Returns
        the (rows, width, 4) uint8 display after the last frame, or, with
        `planes` (names as for render_frame_planes), (rgba, dict)."""
        fd = frame_desc(width, height, **frame_desc_args)
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        rays = np.ascontiguousarray(rays, abi.RAY)
        if rays.size != max(fd.samples, 1) * n * width:
            raise MirtError(f"render_rays: {rays.size} rays, the frame needs {max(fd.samples, 1) * n * width}")
        out = np.zeros((n, width, 4), np.uint8)
        bufs, pl = None, None
        if planes is not None:
            lead = (fd.samples, n, width) if fd.samples > 1 else (n, width)
            self._planes_struct(dict.fromkeys(planes, 0), "render_rays")   # the names
            bufs = {k: np.zeros(lead + self.PLANES[k][1], self.PLANES[k][0]) for k in planes}
            pl = C.byref(self._planes_struct({k: b.ctypes.data for k, b in bufs.items()}, "render_rays"))
        # (an empty array has no address worth passing, but NULL rays are an error: its own, unread, will do)
        check(self.L.mirt_render_rays(self.h, C.c_void_p(rays.ctypes.data), C.byref(fd), ptr(out), pl),
              "mirt_render_rays")
        return out if planes is None else (out, bufs)

    def render_rays_device(self, d_rays, fd, d_out, d_acc=None, d_planes=None, stream=None):
        """Enqueue a ray frame on device memory (integer device pointers):
        d_rays holds samples * rows * width 24-byte rays, read on `stream`;
        d_planes maps "t" / "sphere" / "normal" to device pointers, or None."""
        pl = C.byref(self._planes_struct(d_planes, "render_rays_device")) if d_planes is not None else None
        check(self.L.mirt_render_rays_device(self.h, C.c_void_p(d_rays), C.byref(fd), C.c_void_p(d_out),
                                             C.c_void_p(d_acc) if d_acc else None, pl, C.c_void_p(stream or 0)),
              "mirt_render_rays_device")

    # ---- lens frames (a thin lens computed in the frame's own camera pass)
    @staticmethod
    def _lens(lens):
        """abi.Lens from an abi.Lens or an (aperture, focus) pair."""
        return lens if isinstance(lens, abi.Lens) else abi.Lens(*lens)

    def lens_rays(self, cam, lens, width, height, **frame_desc_args):
        """The rays a lens frame of these arguments traces (mirt_lens_rays): an
        abi.RAY array (rows, width), or (samples, rows, width) with samples > 1,
        indexed as the colour output (slab j = RNG sample sample + j)."""
        fd = frame_desc(width, height, **frame_desc_args)
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        out = np.zeros((fd.samples, n, width) if fd.samples > 1 else (n, width), abi.RAY)
        check(self.L.mirt_lens_rays(self.h, C.byref(cam), C.byref(self._lens(lens)), C.byref(fd),
                                    C.c_void_p(out.ctypes.data)), "mirt_lens_rays")
        return out

    def render_lens_frame(self, cam, lens, width, height, planes=None, **frame_desc_args):
        """render_frame (frame_desc's keyword arguments: samples, accumulate,
        shard, num_shards, ...) through the thin lens `lens` (an abi.Lens or
        (aperture, focus); mirt_render_lens_frame). Returns the (rows, width, 4)
        uint8 display after the last frame, or, with `planes` (names as for
        render_frame_planes), (rgba, dict)."""
        fd = frame_desc(width, height, **frame_desc_args)
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        out = np.zeros((n, width, 4), np.uint8)
        bufs, pl = None, None
        if planes is not None:
            lead = (fd.samples, n, width) if fd.samples > 1 else (n, width)
            self._planes_struct(dict.fromkeys(planes, 0), "render_lens_frame")   # the names
            bufs = {k: np.zeros(lead + self.PLANES[k][1], self.PLANES[k][0]) for k in planes}
            pl = C.byref(self._planes_struct({k: b.ctypes.data for k, b in bufs.items()}, "render_lens_frame"))
        check(self.L.mirt_render_lens_frame(self.h, C.byref(cam), C.byref(self._lens(lens)), C.byref(fd), ptr(out), pl),
              "mirt_render_lens_frame")
        return out if planes is None else (out, bufs)

    def render_lens_frame_device(self, cam, lens, fd, d_out, d_acc=None, d_planes=None, stream=None):
        """Enqueue a lens frame into device memory (integer device pointers);
        d_planes maps "t" / "sphere" / "normal" to device pointers, or None."""
        pl = C.byref(self._planes_struct(d_planes, "render_lens_frame_device")) if d_planes is not None else None
        check(self.L.mirt_render_lens_frame_device(self.h, C.byref(cam), C.byref(self._lens(lens)), C.byref(fd),
                                                   C.c_void_p(d_out), C.c_void_p(d_acc) if d_acc else None, pl,
                                                   C.c_void_p(stream or 0)), "mirt_render_lens_frame_device")

    def render_lens_frame_async(self, cam, lens, fd, out, planes=None):
        """render_frame_async of a lens frame; `planes` as for
        render_frame_planes_async, or None. Complete after wait()."""
        arr = out.array if isinstance(out, HostBuffer) else out
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        if arr.nbytes < n * fd.width * 4 or not arr.flags["C_CONTIGUOUS"]:
            raise MirtError(f"render_lens_frame_async: output holds {arr.nbytes} bytes, the shard needs "
                            f"{n * fd.width * 4}")
        pl = None
        if planes is not None:
            ptrs = {}
            for k, buf in planes.items():
                a = buf.array if isinstance(buf, HostBuffer) else buf
                need = max(fd.samples, 1) * n * fd.width * (12 if k == "normal" else 4)
                if a.nbytes < need or not a.flags["C_CONTIGUOUS"]:
                    raise MirtError(f"render_lens_frame_async: plane {k!r} holds {a.nbytes} bytes, the frame needs "
                                    f"{need}")
                ptrs[k] = a.ctypes.data
            pl = C.byref(self._planes_struct(ptrs, "render_lens_frame_async"))
        check(self.L.mirt_render_lens_frame_async(self.h, C.byref(cam), C.byref(self._lens(lens)), C.byref(fd),
                                                  ptr(arr), pl), "mirt_render_lens_frame_async")

    # ---- denoising (an edge-avoiding a-trous filter guided by the primary-hit planes)
    @staticmethod
    def _denoise_params(params):
        """abi.DenoiseParams from one, from (passes, normal_sharpness, sigma_colour), or the defaults for None."""
        if isinstance(params, abi.DenoiseParams):
            return params
        p = abi.DenoiseParams()
        load().mirt_denoise_params_default(C.byref(p))
        if params is not None:
            p.passes, p.normal_sharpness, p.sigma_colour = params
        return p

    def denoise(self, sphere, normal=None, rgba=None, accum=None, frames=1, params=None, out=None, rgb=False,
                stream=None):
        """The filter of mirt.h's mirt_denoise_params on an image given as
        numpy arrays (mirt_denoise: blocking) or as torch tensors on the ctx's
        device (mirt_denoise_device: enqueued on `stream`, an integer
        hipStream_t, 0 / None = the default stream, not waited for). sphere:
        (H, W) int32; normal: (H, W, 3) float32 or None; the colours either
        rgba (H, W, 4) uint8 or accum (H, W, 3) float32 with its divisor
        `frames`. Returns the (H, W, 4) uint8 display, or with rgb=True
        (display, (H, W, 3) float32). `out` (device form): the uint8 tensor the
        display goes to, which may be `rgba` itself."""
        p = self._denoise_params(params)
        src = rgba if rgba is not None else accum
        if src is None or (rgba is not None and accum is not None):
            raise MirtError("denoise: give exactly one of rgba and accum")
        h, w = sphere.shape
        if not isinstance(sphere, np.ndarray):   # device tensors
            import torch
            for t, dtype in ((sphere, torch.int32), (normal, torch.float32), (rgba, torch.uint8),
                             (accum, torch.float32), (out, torch.uint8)):
                if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == dtype):
                    raise MirtError("denoise: tensors must be contiguous, on the device, int32 / float32 / uint8")
            if out is None:
                out = torch.empty((h, w, 4), dtype=torch.uint8, device=sphere.device)
            out_rgb = torch.empty((h, w, 3), dtype=torch.float32, device=sphere.device) if rgb else None
            dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            check(self.L.mirt_denoise_device(self.h, w, h, dp(rgba), dp(accum), frames, dp(sphere), dp(normal),
                                             C.byref(p), dp(out), dp(out_rgb), C.c_void_p(stream or 0)),
                  "mirt_denoise_device")
            return (out, out_rgb) if rgb else out
        sphere = np.ascontiguousarray(sphere, np.int32)
        normal = None if normal is None else np.ascontiguousarray(normal, np.float32)
        rgba = None if rgba is None else np.ascontiguousarray(rgba, np.uint8)
        accum = None if accum is None else np.ascontiguousarray(accum, np.float32)
        res = np.zeros((h, w, 4), np.uint8)
        out_rgb = np.zeros((h, w, 3), np.float32) if rgb else None
        check(self.L.mirt_denoise(self.h, w, h, ptr(rgba), ptr(accum), frames, ptr(sphere), ptr(normal), C.byref(p),
                                  ptr(res), ptr(out_rgb)), "mirt_denoise")
        return (res, out_rgb) if rgb else res

    def render_frame_denoised(self, cam, width, height, lens=None, params=None, raw=False, **frame_desc_args):
        """render_frame (frame_desc's keyword arguments; one shard), through
        `lens` if given, and its filtered display (mirt_render_frame_denoised):
        the filter's source is the accumulation buffer with accumulate=True,
        else the frame's display; the accumulation buffer is left as the plain
        call leaves it. Returns the filtered (height, width, 4) uint8 display,
        or with raw=True (filtered, the display render_frame returns)."""
        fd = frame_desc(width, height, **frame_desc_args)
        out = np.zeros((height, width, 4), np.uint8)
        plain = np.zeros((height, width, 4), np.uint8) if raw else None
        check(self.L.mirt_render_frame_denoised(self.h, C.byref(cam), C.byref(self._lens(lens)) if lens is not None
                                                else None, C.byref(fd), C.byref(self._denoise_params(params)),
                                                ptr(out), ptr(plain)), "mirt_render_frame_denoised")
        return (out, plain) if raw else out

    # ---- reprojection (a per-pixel history carried from the previous camera to the current one)
    @staticmethod
    def _reproject_params(params):
        """abi.ReprojectParams from one, from (max_history, taps, t_tolerance), or the defaults for None."""
        if isinstance(params, abi.ReprojectParams):
            return params
        p = abi.ReprojectParams()
        load().mirt_reproject_params_default(C.byref(p))
        if params is not None:
            p.max_history, p.taps, p.t_tolerance = params
        return p

    def reproject(self, cam, rgba, t, sphere, prev=None, params=None, rgb=False, out=None, stream=None, motion=None):
        """The reprojection of mirt.h's mirt_reproject_params on a frame given
        as numpy arrays (mirt_reproject: blocking) or as torch tensors on the
        ctx's device (mirt_reproject_device: enqueued on `stream`, an integer
        hipStream_t, 0 / None = the default stream, not waited for). rgba:
        (H, W, 4) uint8; t: (H, W) float32; sphere: (H, W) int32; prev: None on
        the first frame, else (cam_prev, hist, t_prev, sphere_prev) with hist
        (H, W) abi.HISTORY records (tensors: (H, W, 4) float32 holding the same
        16 bytes). Returns (hist_out, display), or with rgb=True (hist_out,
        display, (H, W, 3) float32). `out` (device form): the uint8 tensor the
        display goes to, which may be `rgba` itself. motion: None, or
        (geo, geo_prev, prev_index) -- the spheres moved between the two frames
        (mirt_sphere_motion, mirt_reproject_motion[_device]): geo (n, 4) and
        geo_prev (m, 4) float32 {centre, radius}, prev_index (n,) int32 or None
        for the identity; arrays or device tensors as the frame is."""
        p = self._reproject_params(params)
        h, w = sphere.shape
        geo, geo_prev, prev_index = motion if motion is not None else (None, None, None)
        cam_prev, hist, t_prev, sphere_prev = prev if prev is not None else (None, None, None, None)
        cp = C.byref(cam_prev) if cam_prev is not None else None
        if not isinstance(sphere, np.ndarray):   # device tensors
            import torch
            for a, dtype in ((rgba, torch.uint8), (t, torch.float32), (sphere, torch.int32), (hist, torch.float32),
                             (t_prev, torch.float32), (sphere_prev, torch.int32), (out, torch.uint8),
                             (geo, torch.float32), (geo_prev, torch.float32), (prev_index, torch.int32)):
                if a is not None and not (a.is_cuda and a.is_contiguous() and a.dtype == dtype):
                    raise MirtError("reproject: tensors must be contiguous, on the device, uint8 / float32 / int32")
            hist_out = torch.empty((h, w, 4), dtype=torch.float32, device=sphere.device)
            if out is None:
                out = torch.empty((h, w, 4), dtype=torch.uint8, device=sphere.device)
            out_rgb = torch.empty((h, w, 3), dtype=torch.float32, device=sphere.device) if rgb else None
            dp = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
            if motion is not None:
                mo = abi.SphereMotion(geo.data_ptr(), geo_prev.data_ptr(),
                                      prev_index.data_ptr() if prev_index is not None else None, geo.shape[0],
                                      geo_prev.shape[0])
                check(self.L.mirt_reproject_motion_device(self.h, w, h, C.byref(cam), cp, dp(rgba), dp(t), dp(sphere),
                                                          dp(hist), dp(t_prev), dp(sphere_prev), C.byref(p),
                                                          dp(hist_out), dp(out), dp(out_rgb), C.c_void_p(stream or 0),
                                                          C.byref(mo)), "mirt_reproject_motion_device")
                return (hist_out, out, out_rgb) if rgb else (hist_out, out)
            check(self.L.mirt_reproject_device(self.h, w, h, C.byref(cam), cp, dp(rgba), dp(t), dp(sphere), dp(hist),
                                               dp(t_prev), dp(sphere_prev), C.byref(p), dp(hist_out), dp(out),
                                               dp(out_rgb), C.c_void_p(stream or 0)), "mirt_reproject_device")
            return (hist_out, out, out_rgb) if rgb else (hist_out, out)
        cont = lambda a, dtype: None if a is None else np.ascontiguousarray(a, dtype)   # noqa: E731
        rgba, t, sphere = cont(rgba, np.uint8), cont(t, np.float32), cont(sphere, np.int32)
        hist, t_prev, sphere_prev = cont(hist, abi.HISTORY), cont(t_prev, np.float32), cont(sphere_prev, np.int32)
        hist_out = np.zeros((h, w), abi.HISTORY)
        res = np.zeros((h, w, 4), np.uint8)
        out_rgb = np.zeros((h, w, 3), np.float32) if rgb else None
        if motion is not None:
            geo, geo_prev = cont(geo, np.float32), cont(geo_prev, np.float32)
            prev_index = cont(prev_index, np.int32)
            mo = abi.SphereMotion(geo.ctypes.data, geo_prev.ctypes.data,
                                  prev_index.ctypes.data if prev_index is not None else None, geo.shape[0],
                                  geo_prev.shape[0])
            check(self.L.mirt_reproject_motion(self.h, w, h, C.byref(cam), cp, ptr(rgba), ptr(t), ptr(sphere), ptr(hist),
                                               ptr(t_prev), ptr(sphere_prev), C.byref(p), ptr(hist_out), ptr(res),
                                               ptr(out_rgb), C.byref(mo)), "mirt_reproject_motion")
            return (hist_out, res, out_rgb) if rgb else (hist_out, res)
        check(self.L.mirt_reproject(self.h, w, h, C.byref(cam), cp, ptr(rgba), ptr(t), ptr(sphere), ptr(hist),
                                    ptr(t_prev), ptr(sphere_prev), C.byref(p), ptr(hist_out), ptr(res), ptr(out_rgb)),
              "mirt_reproject")
        return (hist_out, res, out_rgb) if rgb else (hist_out, res)

    # ---- variance-guided filtering (the history carries E[L^2]; its variance steers an a-trous filter)
    def reproject_moments(self, cam, rgba, t, sphere, prev=None, params=None, rgb=False, out=None, stream=None,
                          motion=None):
        """reproject with the second moment of luminance carried along
        (mirt_reproject_moments on numpy arrays, mirt_reproject_moments_device
        on tensors): the arguments of reproject, except that prev is None or
        (cam_prev, hist, t_prev, sphere_prev, m2_prev) with m2_prev (H, W)
        float32. Returns (hist_out, display, m2_out), or with rgb=True
        (hist_out, display, (H, W, 3) float32, m2_out)."""
        p = self._reproject_params(params)
        h, w = sphere.shape
        geo, geo_prev, prev_index = motion if motion is not None else (None, None, None)
        cam_prev, hist, t_prev, sphere_prev, m2_prev = prev if prev is not None else (None,) * 5
        cp = C.byref(cam_prev) if cam_prev is not None else None
        if not isinstance(sphere, np.ndarray):   # device tensors
            import torch
            for a, dtype in ((rgba, torch.uint8), (t, torch.float32), (sphere, torch.int32), (hist, torch.float32),
                             (t_prev, torch.float32), (sphere_prev, torch.int32), (out, torch.uint8),
                             (geo, torch.float32), (geo_prev, torch.float32), (prev_index, torch.int32),
                             (m2_prev, torch.float32)):
                if a is not None and not (a.is_cuda and a.is_contiguous() and a.dtype == dtype):
                    raise MirtError("reproject_moments: tensors must be contiguous, on the device, uint8 / float32 / "
                                    "int32")
            hist_out = torch.empty((h, w, 4), dtype=torch.float32, device=sphere.device)
            m2_out = torch.empty((h, w), dtype=torch.float32, device=sphere.device)
            if out is None:
                out = torch.empty((h, w, 4), dtype=torch.uint8, device=sphere.device)
            out_rgb = torch.empty((h, w, 3), dtype=torch.float32, device=sphere.device) if rgb else None
            dp = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
            mo = None
            if motion is not None:
                mo = abi.SphereMotion(geo.data_ptr(), geo_prev.data_ptr(),
                                      prev_index.data_ptr() if prev_index is not None else None, geo.shape[0],
                                      geo_prev.shape[0])
            check(self.L.mirt_reproject_moments_device(self.h, w, h, C.byref(cam), cp, dp(rgba), dp(t), dp(sphere),
                                                       dp(hist), dp(t_prev), dp(sphere_prev), C.byref(p), dp(hist_out),
                                                       dp(out), dp(out_rgb), C.c_void_p(stream or 0),
                                                       C.byref(mo) if mo is not None else None, dp(m2_prev),
                                                       dp(m2_out)), "mirt_reproject_moments_device")
            return (hist_out, out, out_rgb, m2_out) if rgb else (hist_out, out, m2_out)
        cont = lambda a, dtype: None if a is None else np.ascontiguousarray(a, dtype)   # noqa: E731
        rgba, t, sphere = cont(rgba, np.uint8), cont(t, np.float32), cont(sphere, np.int32)
        hist, t_prev, sphere_prev = cont(hist, abi.HISTORY), cont(t_prev, np.float32), cont(sphere_prev, np.int32)
        m2_prev = cont(m2_prev, np.float32)
        hist_out = np.zeros((h, w), abi.HISTORY)
        m2_out = np.zeros((h, w), np.float32)
        res = np.zeros((h, w, 4), np.uint8)
        out_rgb = np.zeros((h, w, 3), np.float32) if rgb else None
        mo = None
        if motion is not None:
            geo, geo_prev = cont(geo, np.float32), cont(geo_prev, np.float32)
            prev_index = cont(prev_index, np.int32)
            mo = abi.SphereMotion(geo.ctypes.data, geo_prev.ctypes.data,
                                  prev_index.ctypes.data if prev_index is not None else None, geo.shape[0],
                                  geo_prev.shape[0])
        check(self.L.mirt_reproject_moments(self.h, w, h, C.byref(cam), cp, ptr(rgba), ptr(t), ptr(sphere), ptr(hist),
                                            ptr(t_prev), ptr(sphere_prev), C.byref(p), ptr(hist_out), ptr(res),
                                            ptr(out_rgb), C.byref(mo) if mo is not None else None, ptr(m2_prev),
                                            ptr(m2_out)), "mirt_reproject_moments")
        return (hist_out, res, out_rgb, m2_out) if rgb else (hist_out, res, m2_out)

    @staticmethod
    def _denoise_var_params(params):
        """abi.DenoiseVarParams from one, from (passes, normal_sharpness, sigma_lum, min_history), or the defaults."""
        if isinstance(params, abi.DenoiseVarParams):
            return params
        p = abi.DenoiseVarParams()
        load().mirt_denoise_var_params_default(C.byref(p))
        if params is not None:
            p.passes, p.normal_sharpness, p.sigma_lum, p.min_history = params
        return p

    def denoise_var(self, hist, m2, sphere, normal=None, params=None, out=None, rgb=False, var=False, stream=None):
        """The variance-guided filter of mirt.h's mirt_denoise_var_params on
        records given as numpy arrays (mirt_denoise_var: blocking) or as torch
        tensors on the ctx's device (mirt_denoise_var_device: enqueued on
        `stream`, not waited for). hist: (H, W) abi.HISTORY (tensors:
        (H, W, 4) float32 holding the same 16 bytes); m2: (H, W) float32;
        sphere: (H, W) int32; normal: (H, W, 3) float32 or None. Returns the
        (H, W, 4) uint8 display; with rgb=True and / or var=True a tuple
        (display[, (H, W, 3) float32][, (H, W) float32 variances])."""
        p = self._denoise_var_params(params)
        h, w = sphere.shape
        if not isinstance(sphere, np.ndarray):   # device tensors
            import torch
            for a, dtype in ((hist, torch.float32), (m2, torch.float32), (sphere, torch.int32),
                             (normal, torch.float32), (out, torch.uint8)):
                if a is not None and not (a.is_cuda and a.is_contiguous() and a.dtype == dtype):
                    raise MirtError("denoise_var: tensors must be contiguous, on the device, float32 / int32 / uint8")
            if out is None:
                out = torch.empty((h, w, 4), dtype=torch.uint8, device=sphere.device)
            out_rgb = torch.empty((h, w, 3), dtype=torch.float32, device=sphere.device) if rgb else None
            var_out = torch.empty((h, w), dtype=torch.float32, device=sphere.device) if var else None
            dp = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
            check(self.L.mirt_denoise_var_device(self.h, w, h, dp(hist), dp(m2), dp(sphere), dp(normal), C.byref(p),
                                                 dp(out), dp(out_rgb), dp(var_out), C.c_void_p(stream or 0)),
                  "mirt_denoise_var_device")
            res = out
        else:
            hist, m2 = np.ascontiguousarray(hist, abi.HISTORY), np.ascontiguousarray(m2, np.float32)
            sphere = np.ascontiguousarray(sphere, np.int32)
            normal = None if normal is None else np.ascontiguousarray(normal, np.float32)
            res = np.zeros((h, w, 4), np.uint8)
            out_rgb = np.zeros((h, w, 3), np.float32) if rgb else None
            var_out = np.zeros((h, w), np.float32) if var else None
            check(self.L.mirt_denoise_var(self.h, w, h, ptr(hist), ptr(m2), ptr(sphere), ptr(normal), C.byref(p),
                                          ptr(res), ptr(out_rgb), ptr(var_out)), "mirt_denoise_var")
        got = (res,) + ((out_rgb,) if rgb else ()) + ((var_out,) if var else ())
        return got if len(got) > 1 else res

    def render_frame_reprojected_denoised(self, cam, width, height, params=None, var_params=None, reprojected=False,
                                          raw=False, **frame_desc_args):
        """render_frame_reprojected with the second moment carried along, and
        the variance-guided filter of the new records
        (mirt_render_frame_reprojected_denoised). Returns the filtered
        (height, width, 4) uint8 display; with reprojected=True and / or
        raw=True a tuple (filtered[, the history's display][, the one-sample
        display])."""
        fd = frame_desc(width, height, **frame_desc_args)
        out = np.zeros((height, width, 4), np.uint8)
        rep = np.zeros((height, width, 4), np.uint8) if reprojected else None
        plain = np.zeros((height, width, 4), np.uint8) if raw else None
        check(self.L.mirt_render_frame_reprojected_denoised(self.h, C.byref(cam), C.byref(fd),
                                                            C.byref(self._reproject_params(params)),
                                                            C.byref(self._denoise_var_params(var_params)), ptr(out),
                                                            ptr(rep), ptr(plain)),
              "mirt_render_frame_reprojected_denoised")
        got = (out,) + ((rep,) if reprojected else ()) + ((plain,) if raw else ())
        return got if len(got) > 1 else out

    def history_moments_read(self):
        """The current m2 plane, (height, width) float32 (mirt_history_moments_read)."""
        st = self.history_stats()
        out = np.zeros((st["height"], st["width"]), np.float32)
        check(self.L.mirt_history_moments_read(self.h, ptr(out), out.size), "mirt_history_moments_read")
        return out

    def render_frame_reprojected(self, cam, width, height, params=None, raw=False, **frame_desc_args):
        """render_frame (frame_desc's keyword arguments; one sample, one shard,
        no jitter, not accumulating) and the display of its history
        (mirt_render_frame_reprojected): each pixel's record is carried from
        where the previous call's camera saw the same surface. Returns the
        (height, width, 4) uint8 display, or with raw=True (display, the
        one-sample display render_frame returns)."""
        fd = frame_desc(width, height, **frame_desc_args)
        out = np.zeros((height, width, 4), np.uint8)
        plain = np.zeros((height, width, 4), np.uint8) if raw else None
        check(self.L.mirt_render_frame_reprojected(self.h, C.byref(cam), C.byref(fd),
                                                   C.byref(self._reproject_params(params)), ptr(out), ptr(plain)),
              "mirt_render_frame_reprojected")
        return (out, plain) if raw else out

    def history_reset(self):
        """Empty the history of render_frame_reprojected (mirt_history_reset)."""
        check(self.L.mirt_history_reset(self.h), "mirt_history_reset")

    def history_stats(self):
        """mirt_history_stats as a dict (waits for the ctx's stream)."""
        st = abi.HistoryStats()
        check(self.L.mirt_history_stats_get(self.h, C.byref(st)), "mirt_history_stats_get")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def history_motion(self):
        """mirt_history_motion as a dict: the scene slot's link (abi.OPT_HISTORY_MOTION) and whether this ctx's last
        reprojected frame was carried over one. No device call."""
        st = abi.HistoryMotion()
        check(self.L.mirt_history_motion_get(self.h, C.byref(st)), "mirt_history_motion_get")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def history_read(self):
        """The current records, (height, width) abi.HISTORY (mirt_history_read)."""
        st = self.history_stats()
        out = np.zeros((st["height"], st["width"]), abi.HISTORY)
        check(self.L.mirt_history_read(self.h, ptr(out), out.size), "mirt_history_read")
        return out

    def share_accum(self, owner):
        """Use `owner`'s accumulation buffer (mirt_ctx_share_accum): the ctxs
        of one accumulating display loop with frames in flight; None: a
        private buffer again."""
        check(self.L.mirt_ctx_share_accum(self.h, owner.h if owner is not None else None), "mirt_ctx_share_accum")

    def share_scene(self, owner):
        """Render `owner`'s resident scene (mirt_ctx_share_scene): installs and
        reads through either context then concern one scene, and frames in
        flight finish on the scene they were enqueued on. None: a private slot
        again, still holding the scene the group has now."""
        check(self.L.mirt_ctx_share_scene(self.h, owner.h if owner is not None else None), "mirt_ctx_share_scene")

    def scene_id(self):
        """mirt_ctx_scene_id: the stamp of the resident scene (0: none); equal
        across the contexts that share it, new with every install."""
        return int(self.L.mirt_ctx_scene_id(self.h))

    def accum(self, count):
        out = np.zeros(count, np.float32)
        check(self.L.mirt_accum_download(self.h, ptr(out), count), "mirt_accum_download")
        return out

    def count_frame(self, cam, width, height, depth=5, use_bvh=True, seed=1, sample=0, row_block=8, shard=0,
                    num_shards=1, samples=1, jitter=False):
        """Work of one launch (samples frames): rays, node tests, sphere tests, hits."""
        fd = frame_desc(width, height, depth, use_bvh, seed, sample, False, 1, row_block, shard, num_shards,
                        samples, jitter)
        c = abi.Counts()
        check(self.L.mirt_count_frame(self.h, C.byref(cam), C.byref(fd), C.byref(c)), "mirt_count_frame")
        return {k: getattr(c, k) for k, _ in abi.Counts._fields_}

    def set_option(self, option, value):
        """abi.OPT_TRAVERSAL (abi.TRAV_*) / abi.OPT_FAST_SLAB (0/1): speed only."""
        check(self.L.mirt_set_option(self.h, option, value), "mirt_set_option")

    def get_option(self, option):
        return check(self.L.mirt_get_option(self.h, option), "mirt_get_option")

    def primary_cache_stats(self):
        """mirt_primary_cache_stats of this context (abi.OPT_PRIMARY_CACHE), as
        a dict; "last" is "hit" / "fill" / "bypass" and "reason" the name of
        why the last frame was no hit ("" on a hit)."""
        return primary_cache_stats(self.h)

    def primary_scan_stats(self):
        """mirt_primary_scan_stats of this context (abi.OPT_PRIMARY_SCAN), as a dict."""
        return primary_scan_stats(self.h)

    def primary_cache_read(self):
        """The cache's slab (mirt_primary_cache_read): (t float32, sphere int32),
        each of shape (rows, width)."""
        st = self.primary_cache_stats()
        t = np.zeros((st["rows"], st["width"]), np.float32)
        sphere = np.zeros((st["rows"], st["width"]), np.int32)
        check(self.L.mirt_primary_cache_read(self.h, ptr(t), ptr(sphere), t.size), "mirt_primary_cache_read")
        return t, sphere

    def primary_cache_write(self, t, sphere):
        """Replace the cache's slab (mirt_primary_cache_write; a test hook: a
        hit frame then starts from these hits)."""
        t = np.ascontiguousarray(t, np.float32)
        sphere = np.ascontiguousarray(sphere, np.int32)
        if t.size != sphere.size:
            raise MirtError(f"primary_cache_write: {t.size} t values for {sphere.size} sphere indices")
        check(self.L.mirt_primary_cache_write(self.h, ptr(t), ptr(sphere), t.size), "mirt_primary_cache_write")

    def bounce_stats(self, cam, width, height, depth=5, seed=1, sample=0, shard=0, num_shards=1):
        """Per-wave diagnostic of the bounce kernel: uint64 array of (iterations,
        walking lanes summed, iterations after the queue ran dry, their lanes,
        t_start, t_dry, t_end [10 ns ticks], longest chain << 32 | longest walk,
        quad-drain iterations, t_quad_start, DFS-segment fallback lane-steps,
        fallbacks entered, gate executions, those with an f64 t, its lanes, those
        with a LeafBox load, its lanes, iterations with a gate / f64 t / LeafBox,
        closest hits confirmed, confirmations failed, fallback restarts)."""
        fd = frame_desc(width, height, depth, True, seed, sample, False, 1, 8, shard, num_shards)
        n = -self.L.mirt_bounce_stats(self.h, C.byref(cam), C.byref(fd), None, 0)
        if n <= 0:
            check(-n, "mirt_bounce_stats")
        out = np.zeros((n, abi.BOUNCE_STATS_WORDS), np.uint64)
        check(self.L.mirt_bounce_stats(self.h, C.byref(cam), C.byref(fd), ptr(out), n), "mirt_bounce_stats")
        return out

    def wave_stats(self, cam, width, height, depth=5, use_bvh=True, seed=1, sample=0, row_block=8, shard=0,
                   num_shards=1):
        """Per-wave (8x8 tile) diagnostic: array of (tile, steps, start, end),
        start/end in 10 ns ticks of the device's constant clock."""
        fd = frame_desc(width, height, depth, use_bvh, seed, sample, False, 1, row_block, shard, num_shards)
        n = -self.L.mirt_wave_stats(self.h, C.byref(cam), C.byref(fd), None, 0)
        out = np.zeros((n, 4), np.uint32)
        check(self.L.mirt_wave_stats(self.h, C.byref(cam), C.byref(fd), ptr(out), n), "mirt_wave_stats")
        return out

    @property
    def stream_handle(self):
        """The ctx's own hipStream_t (int)."""
        return self.L.mirt_ctx_stream(self.h) or 0

    @property
    def last_kernel_ms(self):
        return self.L.mirt_last_kernel_ms(self.h)

    def last_phase_ms(self):
        """(primary ms, bounce ms) of the last wavefront-schedule frame; waits for it."""
        out = (C.c_float * 2)()
        check(self.L.mirt_last_phase_ms(self.h, out), "mirt_last_phase_ms")
        return float(out[0]), float(out[1])

    def phase_log(self, n=64):
        """(primary ms, bounce ms) of each of the ctx's last <= n wavefront
        frames, oldest first, from HIP events on each frame's own stream
        (durations under whatever overlap the frames ran with); waits."""
        out = (C.c_float * (2 * n))()
        k = check(self.L.mirt_phase_log(self.h, out, n), "mirt_phase_log")
        return [(float(out[2 * j]), float(out[2 * j + 1])) for j in range(k)]

    def bvh_overlay(self, cam, width, height, max_levels=-1):
        """The BVH debug view (bvh_visualiser.c:16-126) of the uploaded tree:
        (height, width, 4) uint8."""
        out = np.zeros((height, width, 4), np.uint8)
        check(self.L.mirt_bvh_overlay(self.h, C.byref(cam), width, height, max_levels, ptr(out)), "mirt_bvh_overlay")
        return out

    # ---- per-ray surface (batched)
    def get_camera_rays(self, cam, width, height, row_block=8, shard=0, num_shards=1):
        fd = frame_desc(width, height, 1, True, 1, 0, False, 1, row_block, shard, num_shards)
        n = check(self.L.mirt_shard_rows(C.byref(fd), None), "mirt_shard_rows")
        out = np.zeros((n, width), abi.RAY)
        check(self.L.mirt_camera_rays(self.h, C.byref(cam), C.byref(fd), ptr(out)), "mirt_camera_rays")
        return out

    def camera_rays_uv(self, cam, width, height, uv):
        """get_camera_ray (ray.c:17-32) at caller-given (u, v): `uv` is (n, 2)
        float32, the result n abi.RAY."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros(len(uv), abi.RAY)
        check(self.L.mirt_camera_rays_uv(self.h, C.byref(cam), width, height, ptr(uv), len(uv), ptr(out)),
              "mirt_camera_rays_uv")
        return out

    def trace_ray(self, rays, depth=5, use_bvh=True, seed=1, sample=0):
        rays = np.ascontiguousarray(rays, abi.RAY)
        out = np.zeros((len(rays), 4), np.uint8)
        check(self.L.mirt_trace_rays(self.h, ptr(rays), len(rays), depth, int(use_bvh), seed, sample, ptr(out)),
              "mirt_trace_rays")
        return out

    def closest_hit(self, rays, use_bvh=True):
        rays = np.ascontiguousarray(rays, abi.RAY)
        out = np.zeros(len(rays), abi.HIT)
        check(self.L.mirt_intersect_rays(self.h, ptr(rays), len(rays), int(use_bvh), ptr(out)),
              "mirt_intersect_rays")
        return out

    def any_hit(self, rays, use_bvh=False):
        """int32 per ray: 1 if it hits some sphere (benchmark.c:190-199
        brute force; with use_bvh, ray_bvh_intersect's hit_something)."""
        rays = np.ascontiguousarray(rays, abi.RAY)
        out = np.zeros(len(rays), np.int32)
        check(self.L.mirt_any_hit_rays(self.h, ptr(rays), len(rays), int(use_bvh), ptr(out)), "mirt_any_hit_rays")
        return out

    def ray_bvh_intersect(self, rays):
        return self.closest_hit(rays, True)

    def ray_sphere_intersect(self, rays, spheres):
        rays = np.ascontiguousarray(rays, abi.RAY)
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        out = np.zeros(len(rays), abi.HIT)
        check(self.L.mirt_sphere_pairs(self.h, ptr(rays), ptr(spheres), len(rays), ptr(out)), "mirt_sphere_pairs")
        return out

    def ray_aabb_intersect(self, rays, boxes):
        rays = np.ascontiguousarray(rays, abi.RAY)
        boxes = np.ascontiguousarray(boxes, abi.AABB)
        out = np.zeros(len(rays), np.int32)
        check(self.L.mirt_aabb_pairs(self.h, ptr(rays), ptr(boxes), len(rays), ptr(out)), "mirt_aabb_pairs")
        return out

    # ---- diagnostics: the walks' filtered tests on pairs
    def box_form_pairs(self, rays, boxes, best, form):
        """int32 per pair: 1 if the walks' box test `form` (abi.BOX_FORM_*)
        passes box i for ray i with a best hit so far of best[i] (+inf: none),
        under the uploaded scene's pruning state and origin bound."""
        rays = np.ascontiguousarray(rays, abi.RAY)
        boxes = np.ascontiguousarray(boxes, abi.AABB)
        best = np.ascontiguousarray(best, np.float32)
        assert len(boxes) == len(rays) and len(best) == len(rays)
        out = np.zeros(len(rays), np.int32)
        check(self.L.mirt_box_form_pairs(self.h, ptr(rays), ptr(boxes), ptr(best), len(rays), form, ptr(out)),
              "mirt_box_form_pairs")
        return out

    def sphere_form_pairs(self, rays, spheres, best, fast=True):
        """float32 per pair: what the walks' sphere test returns for a best hit
        so far of best[i] (t if sphere i would become the closest hit, else
        -1), from the filtered test (fast = 1 / True) or the exact one (0).
        fast = 2: the filtered test with the float-pair certification off;
        fast = 3: 1.4e-45 (the bits of 1) where fast = 1 ran the binary64
        branch, 0 elsewhere -- view the result as uint32 (include/mirt.h)."""
        rays = np.ascontiguousarray(rays, abi.RAY)
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        best = np.ascontiguousarray(best, np.float32)
        assert len(spheres) == len(rays) and len(best) == len(rays)
        out = np.zeros(len(rays), np.uint32)
        check(self.L.mirt_sphere_form_pairs(self.h, ptr(rays), ptr(spheres), ptr(best), len(rays), int(fast),
                                            ptr(out)), "mirt_sphere_form_pairs")
        return out.view(np.float32)

    def sqrt_form_sweep(self):
        """mirt_sqrt_form_sweep: (mismatches, least mismatching bit pattern) of
        normalize3's binary32 root against the binary64 form over every
        non-negative finite float."""
        bad, first = C.c_uint64(), C.c_uint32()
        check(self.L.mirt_sqrt_form_sweep(self.h, C.byref(bad), C.byref(first)), "mirt_sqrt_form_sweep")
        return bad.value, first.value

    def hemisphere_probe(self, keys, k0, normals, need, out_dir):
        """mirt_hemisphere_probe: the kernels' wave-cooperative bounce sampling
        on len(keys) lanes (64, or a multiple of 256). Returns (dir, k):
        float32 (n, 3) directions, starting from `out_dir` (lanes with need ==
        0 keep theirs), and uint32 draws consumed."""
        keys = np.ascontiguousarray(keys, np.uint64)
        k0 = np.ascontiguousarray(k0, np.uint32)
        normals = np.ascontiguousarray(normals, np.float32)
        need = np.ascontiguousarray(need, np.int32)
        d = np.array(out_dir, np.float32, order="C")
        n = len(keys)
        assert k0.shape == (n,) and need.shape == (n,) and normals.shape == (n, 3) and d.shape == (n, 3)
        k = np.zeros(n, np.uint32)
        check(self.L.mirt_hemisphere_probe(self.h, ptr(keys), ptr(k0), ptr(normals), ptr(need), n, ptr(d), ptr(k)),
              "mirt_hemisphere_probe")
        return d, k

    def partition_probe(self, centre, seg, split):
        """The device build's partition on caller-given keys: segments
        [seg[k], seg[k+1]) of `centre`, each partitioned by centre < split[k];
        returns int32 perm, perm[j] = source index of the element that ends at
        position j (bvh.c:172-201's swap loop)."""
        centre = np.ascontiguousarray(centre, np.float32)
        seg = np.ascontiguousarray(seg, np.int32)
        split = np.ascontiguousarray(split, np.float32)
        assert len(seg) == len(split) + 1
        perm = np.zeros(len(centre), np.int32)
        check(self.L.mirt_build_partition_probe(self.h, ptr(centre), len(centre), ptr(seg), len(split), ptr(split),
                                                ptr(perm)), "mirt_build_partition_probe")
        return perm


class MultiRenderer:
    """One frame loop over several GPUs from this process (include/mirt_multi.h,
    SURVEY §8(b) mirt_init(num_gpus)): interleaved row blocks per rank, the
    slabs gathered to rank 0 over RCCL (distinct devices) or by device copies
    ("copy": forced, or a device listed twice -- n shards on one GPU), or with
    host_direct every rank's blocks copied straight into the host frame;
    `lanes` launches in flight, each of one or more frames. Frames equal
    Renderer.render_frame's on one GPU."""

    def __init__(self, devices, lanes=1, copy=False, host_direct=False, queue_ahead=False):
        self.L = load()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        flags = ((abi.MULTI_COPY if copy else 0) | (abi.MULTI_HOST_DIRECT if host_direct else 0)
                 | (abi.MULTI_QUEUE_AHEAD if queue_ahead else 0))
        check(self.L.mirt_multi_create(devs, len(devices), lanes, flags, C.byref(h)), "mirt_multi_create")
        self.h = h
        self.devices = list(devices)
        self.queue_ahead = bool(queue_ahead)
        self.lanes = self.L.mirt_multi_lanes(h)   # launch slots (2 x lanes with queue_ahead)
        self.launches = 0   # launch k runs on lane k % lanes (mirt_multi's rotation)

    def close(self):
        if self.h:
            self.L.mirt_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def backend(self):
        return self.L.mirt_multi_backend(self.h).decode()

    @property
    def delivery(self):
        return self.L.mirt_multi_delivery(self.h).decode()

    @property
    def size(self):
        return self.L.mirt_multi_size(self.h)

    @property
    def failed(self):
        return self.L.mirt_multi_failed(self.h) == 1

    def ctx(self, lane, rank):
        """(lane, rank)'s mirt_ctx handle (owned by the multi renderer)."""
        return self.L.mirt_multi_ctx(self.h, lane, rank)

    def primary_cache_stats(self, lane, rank):
        """mirt_primary_cache_stats of (lane, rank)'s context."""
        return primary_cache_stats(self.ctx(lane, rank))

    def primary_scan_stats(self, lane, rank):
        """mirt_primary_scan_stats of (lane, rank)'s context."""
        return primary_scan_stats(self.ctx(lane, rank))

    def phase_log(self, lane, rank, n):
        """mirt_phase_log of (lane, rank)'s context: [primary_ms, bounce_ms] of its last n frames."""
        buf = (C.c_float * (2 * n))()
        got = check(self.L.mirt_phase_log(self.ctx(lane, rank), buf, n), "mirt_phase_log")
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(got)]

    def upload(self, spheres, bvh):
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        if isinstance(bvh, Bvh):
            check(self.L.mirt_multi_scene_upload_flat(self.h, ptr(spheres), len(spheres), ptr(bvh.nodes),
                                                      len(bvh.nodes)), "mirt_multi_scene_upload_flat")
        else:
            check(self.L.mirt_multi_scene_upload(self.h, ptr(spheres), len(spheres), bvh), "mirt_multi_scene_upload")

    def build_scene(self, spheres, start=0, end=None, depth=0):
        """Renderer.build_scene once per device (mirt_multi_scene_build_device):
        the contexts of a device share the one scene. Launches in flight are
        not waited for; they deliver the old scene's frames. Returns the
        spheres as reordered."""
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        end = len(spheres) if end is None else end
        out = np.zeros(len(spheres), abi.SPHERE)
        check(self.L.mirt_multi_scene_build_device(self.h, ptr(spheres), len(spheres), start, end, depth, ptr(out)),
              "mirt_multi_scene_build_device")
        return out

    def refit_scene(self, spheres, end=None):
        """Renderer.refit_scene once per device (mirt_multi_scene_refit_device),
        under launches in flight."""
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        n = len(spheres)
        end = n if end is None else end
        check(self.L.mirt_multi_scene_refit_device(self.h, ptr(spheres) if n else None, n, end),
              "mirt_multi_scene_refit_device")

    def update_scene(self, spheres, start=0, end=None, max_decay=0.0):
        """Renderer.update_scene once per device (mirt_multi_scene_update_device),
        under launches in flight; (reordered, perm, result) of the first
        device."""
        spheres = np.ascontiguousarray(spheres, abi.SPHERE)
        n = len(spheres)
        end = n if end is None else end
        reordered = np.zeros(n, abi.SPHERE)
        perm = np.zeros(n, np.int32)
        res = abi.UpdateResult()
        check(self.L.mirt_multi_scene_update_device(self.h, ptr(spheres) if n else None, n, start, end, max_decay,
                                                    ptr(reordered) if n else None, ptr(perm) if n else None,
                                                    C.byref(res)), "mirt_multi_scene_update_device")
        return reordered, perm, _fields(res)

    def scene_ids(self):
        """The distinct mirt_ctx_scene_id values of the object's contexts: one
        per device once they share, one per context after upload()."""
        contexts = self.lanes // 2 if self.queue_ahead else self.lanes
        return sorted({int(self.L.mirt_ctx_scene_id(self.ctx(l, r))) for l in range(contexts)
                       for r in range(self.size)})

    def resident_layout(self, lane, rank):
        """Renderer.resident_layout of the scene (lane, rank)'s context renders."""
        view = Renderer.__new__(Renderer)   # a view: the handle stays the object's
        view.L, view.h = self.L, None
        try:
            view.h = self.ctx(lane, rank)
            return view.resident_layout()
        finally:
            view.h = None

    def set_option(self, option, value):
        """MULTI_OPT_* (timeout, emulation) or a MIRT_OPT_* for every context."""
        check(self.L.mirt_multi_set_option(self.h, option, value), "mirt_multi_set_option")

    def get_option(self, option):
        return check(self.L.mirt_multi_get_option(self.h, option), "mirt_multi_get_option")

    def emulate(self, world, rank):
        """Measurement only (one rank): play shard `rank` of a frame split
        `world` ways (MIRT_MULTI_OPT_EMULATE_*); frames are then incomplete."""
        self.set_option(abi.MULTI_OPT_EMULATE_WORLD, world)
        self.set_option(abi.MULTI_OPT_EMULATE_RANK, rank)

    def render_frame(self, cam, width, height, depth=5, use_bvh=True, seed=1, sample=0, accumulate=False, frames=1,
                     row_block=8, samples=1, jitter=False):
        """The whole frame (height, width, 4) uint8, blocking."""
        fd = frame_desc(width, height, depth, use_bvh, seed, sample, accumulate, frames, row_block, 0, 1, samples,
                        jitter)
        out = np.zeros((height, width, 4), np.uint8)
        check(self.L.mirt_multi_render_frame(self.h, C.byref(cam), C.byref(fd), ptr(out)), "mirt_multi_render_frame")
        self.launches += 1
        return out

    @staticmethod
    def _host(out, fd):
        arr = out.array if isinstance(out, HostBuffer) else out
        if arr.nbytes < fd.width * fd.height * 4 or not arr.flags["C_CONTIGUOUS"]:
            raise MirtError("mirt_multi: output too small or not contiguous")
        return arr

    def render_frame_async(self, cam, fd, out):
        """Enqueue a whole frame into `out` (HostBuffer or uint8 array of
        height x width x 4) on the next lane; complete after wait()."""
        arr = self._host(out, fd)
        check(self.L.mirt_multi_render_frame_async(self.h, C.byref(cam), C.byref(fd), ptr(arr)),
              "mirt_multi_render_frame_async")
        self.launches += 1

    def render_frames_async(self, cam, fd, outs, nframes=None, full_grid=False):
        """One launch of len(outs) successive frames (RNG samples fd.sample + j)
        on the next lane, frame j into outs[j]; outs None: `nframes` frames
        left on the devices. Complete after wait() (or the lane's next launch)."""
        n = len(outs) if outs is not None else int(nframes or 1)
        if outs is not None:
            arrs = [self._host(o, fd) for o in outs]
            cp = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        else:
            cp = None
        check(self.L.mirt_multi_render_frames_async(self.h, C.byref(cam), C.byref(fd), n,
                                                    abi.MULTI_FULL_GRID if full_grid else 0, cp),
              "mirt_multi_render_frames_async")
        self.launches += 1

    def render_lens_frames_async(self, cam, lens, fd, outs, nframes=None, full_grid=False):
        """render_frames_async of lens frames (mirt_multi_render_lens_frames_async):
        `lens` is an abi.Lens or (aperture, focus); only it travels to the ranks."""
        n = len(outs) if outs is not None else int(nframes or 1)
        if outs is not None:
            arrs = [self._host(o, fd) for o in outs]
            cp = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        else:
            cp = None
        check(self.L.mirt_multi_render_lens_frames_async(self.h, C.byref(cam), C.byref(Renderer._lens(lens)),
                                                         C.byref(fd), n, abi.MULTI_FULL_GRID if full_grid else 0, cp),
              "mirt_multi_render_lens_frames_async")
        self.launches += 1

    def wait(self):
        check(self.L.mirt_multi_wait(self.h), "mirt_multi_wait")

    def stats(self):
        """mirt_multi_get_stats as a dict (RCCL calls issued, copies, launches)."""
        st = abi.MultiStats()
        check(self.L.mirt_multi_get_stats(self.h, C.byref(st)), "mirt_multi_get_stats")
        return {k: int(getattr(st, k)) for k, _ in abi.MultiStats._fields_}

    def read_gathered(self, shard, rows, width, frame=0, lane=-1):
        """Test hook: shard `shard`'s compact rows (rows x width RGBA8) of
        frame `frame` as they arrived in device 0's gather buffer in the last
        launch (lane -1) or lane `lane`'s."""
        out = np.zeros((rows, width, 4), np.uint8)
        check(self.L.mirt_multi_read_gathered(self.h, lane, shard, frame, ptr(out), out.nbytes),
              "mirt_multi_read_gathered")
        return out

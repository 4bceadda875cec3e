"""ctypes front of the oracle libraries -- TEST INFRASTRUCTURE ONLY.

`Oracle` wraps liboracle.so (the C restatement, oracle.c); `Reference` wraps
_ref/libref_<W>x<H>.so (the unmodified reference sources + ref_harness.c).
Struct layouts come from include/mirt.h via the product's abi module (types
only; no product code runs here).
"""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

abi = importlib.import_module("cs201_sah-bvh_ray_tracer_amd.abi")

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "_ref")
P = C.c_void_p
I = C.c_int


def build(ref=False):
    """Compile liboracle.so (and, if asked and possible, the _ref libraries)."""
    subprocess.run(["make", "-s", "-C", HERE, "all"], check=True)
    if ref and os.path.isdir("/root/reference/src"):
        subprocess.run(["make", "-s", "-C", HERE, "ref"], check=True)


def _p(a):
    return abi.ptr(a)


class Oracle:
    """The C restatement (oracle.c)."""

    def __init__(self, path=None):
        path = path or os.path.join(HERE, "liboracle.so")
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        self.L = L
        sig = {
            "o_srand": (None, [C.c_uint]), "o_libc_rand": (I, []),
            "o_contract_draw": (I, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
            "o_gen_render_scene": (None, [C.c_uint, I, P]),
            "o_gen_bench_scene": (None, [C.c_uint, I, C.c_float, P]),
            "o_build": (P, [P, I, I, I]), "o_free": (None, [P]),
            "o_node_count": (I, [P]), "o_flatten": (I, [P, P, I]), "o_tree_from_flat": (P, [P, I]),
            "o_intersect": (None, [P, P, I, P, I, I, P]),
            "o_intersect_flat": (None, [P, I, P, I, P, I, P]),
            "o_sphere_pairs": (None, [P, P, I, P]), "o_aabb_pairs": (None, [P, P, I, P]),
            "o_camera_ray_px": (None, [P, I, I, I, I, P]),
            "o_render_rows": (None, [P, I, I, P, I, P, I, I, I, C.c_uint64, C.c_uint32, P, I, P, I, P, I]),
            "o_trace_rays": (None, [P, I, P, I, P, I, I, I, C.c_uint64, C.c_uint32, P]),
            "o_accumulate": (None, [P, I, P, I, I, P]),
            "o_bvh_overlay": (None, [P, P, I, I, I, P]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args

    # ---- inputs
    def render_scene(self, seed, n):
        out = np.zeros(n, abi.SPHERE)
        self.L.o_gen_render_scene(seed, n, _p(out))
        return out

    def bench_scene(self, seed, n, world=1000.0):
        out = np.zeros(n, abi.SPHERE)
        self.L.o_gen_bench_scene(seed, n, world, _p(out))
        return out

    def contract_draw(self, seed, pixel, sample, k):
        return self.L.o_contract_draw(seed, pixel, sample, k)

    # ---- BVH (pointer tree handle + flattened copy)
    def build(self, spheres, start=0, end=None, depth=0):
        """Builds in place (reorders `spheres`), returns an opaque tree."""
        end = len(spheres) if end is None else end
        return self.L.o_build(_p(spheres), start, end, depth)

    def flatten(self, tree):
        n = self.L.o_node_count(tree)
        out = np.zeros(n, abi.NODE)
        assert self.L.o_flatten(tree, _p(out), n) == n
        return out

    def tree_from_flat(self, nodes):
        """The pointer tree of a flat tree (abi.NODE array), boxes as they
        stand: what render / trace_rays / intersect take, for a tree that no
        builder made. flatten() of it gives `nodes` back. Release with free."""
        nodes = np.ascontiguousarray(nodes, abi.NODE)
        return self.L.o_tree_from_flat(_p(nodes), len(nodes))

    def free(self, tree):
        self.L.o_free(tree)

    # ---- intersect
    def intersect(self, tree, spheres, rays, use_bvh=True):
        out = np.zeros(len(rays), abi.HIT)
        self.L.o_intersect(tree, _p(spheres), len(spheres), _p(rays), len(rays), int(use_bvh), _p(out))
        return out

    def intersect_flat(self, nodes, spheres, rays):
        """hit.c:91-109 over a flat tree (abi.NODE array)."""
        out = np.zeros(len(rays), abi.HIT)
        nodes = np.ascontiguousarray(nodes, abi.NODE)
        self.L.o_intersect_flat(_p(nodes), len(nodes), _p(spheres), len(spheres), _p(rays), len(rays), _p(out))
        return out

    def sphere_pairs(self, rays, spheres):
        out = np.zeros(len(rays), abi.HIT)
        self.L.o_sphere_pairs(_p(rays), _p(spheres), len(rays), _p(out))
        return out

    def aabb_pairs(self, rays, boxes):
        out = np.zeros(len(rays), np.int32)
        self.L.o_aabb_pairs(_p(rays), _p(boxes), len(rays), _p(out))
        return out

    def camera_rays(self, cam, W, H, rows=None):
        rows = range(H) if rows is None else rows
        out = np.zeros((len(rows), W), abi.RAY)
        r1 = np.zeros(1, abi.RAY)
        for i, y in enumerate(rows):
            for x in range(W):
                self.L.o_camera_ray_px(C.byref(cam), W, H, x, y, _p(r1))
                out[i, x] = r1[0]
        return out

    # ---- shading
    def render(self, cam, W, H, spheres, tree, depth=5, use_bvh=True, mode=1, seed=1, sample=0,
               rows=None, threads=None, counts=False, jitter=False):
        """Fresh frame (main.c:358-374) of the given rows -> (nrows, W, 4) u8."""
        rows = np.arange(H, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, np.int32)
        out = np.zeros((len(rows), W, 4), np.uint8)
        cnt = np.zeros(3, np.int64)
        threads = threads or os.cpu_count() or 1
        if mode == 0:
            self.L.o_srand(seed)
        self.L.o_render_rows(C.byref(cam), W, H, _p(spheres), len(spheres), tree, depth, int(use_bvh),
                             mode, seed, sample, _p(rows), len(rows), _p(out), threads, _p(cnt), int(jitter))
        return (out, cnt) if counts else out

    def trace_rays(self, rays, spheres, tree, depth=5, use_bvh=True, mode=1, seed=1, sample=0):
        out = np.zeros((len(rays), 4), np.uint8)
        if mode == 0:
            self.L.o_srand(seed)
        self.L.o_trace_rays(_p(rays), len(rays), _p(spheres), len(spheres), tree, depth, int(use_bvh),
                            mode, seed, sample, _p(out))
        return out

    def bvh_overlay(self, tree, cam, W, H, max_levels=-1):
        """bvh_visualiser.c:16-126 on an RGBA8 canvas -> (H, W, 4) u8."""
        out = np.zeros((H, W, 4), np.uint8)
        self.L.o_bvh_overlay(tree, C.byref(cam), W, H, max_levels, _p(out))
        return out

    def accumulate(self, colors, acc, fresh, frames):
        colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        shown = np.zeros_like(colors)
        self.L.o_accumulate(_p(colors), len(colors), _p(acc), int(fresh), frames, _p(shown))
        return shown


class Reference:
    """The unmodified reference sources (oracle/_ref/libref_<W>x<H>.so)."""

    def __init__(self, W, H, opt="O2"):
        """opt "O2": -O2 build; "O0": the reference's own flags (no -O, -g)."""
        path = os.path.join(REF_DIR, f"libref_{W}x{H}.so" if opt == "O2" else f"libref_{opt}_{W}x{H}.so")
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        L = C.CDLL(path)
        self.L, self.W, self.H = L, W, H
        sig = {
            "h_width": (I, []), "h_height": (I, []), "h_srand": (None, [C.c_uint]), "h_rand": (I, []),
            "h_sizeof_sphere": (I, []), "h_sizeof_node": (I, []), "h_sizeof_hit": (I, []),
            "h_sizeof_camera": (I, []),
            "h_gen_render_scene": (None, [C.c_uint, I, P]),
            "h_gen_bench_scene": (None, [C.c_uint, I, C.c_float, P]),
            "h_build": (P, [P, I, I, I]), "h_free": (None, [P]), "h_node_count": (I, [P]),
            "h_flatten": (I, [P, P, P, I]), "h_leaf_counts": (I, [P, P]),
            "h_intersect_bvh": (None, [P, P, P, I, P]),
            "h_sphere_pairs": (None, [P, P, I, P]), "h_aabb_pairs": (None, [P, P, I, P]),
            "h_camera_ray": (None, [P, I, I, P]),
            "h_render": (None, [P, P, I, P, I, I, I, C.c_uint64, C.c_uint32, I, I, I, P, I, I]),
            "h_trace_rays": (None, [P, I, P, I, P, I, I, I, C.c_uint64, C.c_uint32, P]),
            "h_camera_update": (None, [P]),
            "h_bench_point": (None, [I, I, C.c_float, P, P, P, P, P, P]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        assert (L.h_width(), L.h_height()) == (W, H)

    def bench_point(self, n, num_rays, world=1000.0):
        """One sweep point of benchmark.c's run_benchmark_with_plotting on the
        current rand() stream (srand first): spheres, rays and hit flags of
        both loops, and their clock() seconds."""
        s = np.zeros(n, abi.SPHERE)
        ra, rb = np.zeros(num_rays, abi.RAY), np.zeros(num_rays, abi.RAY)
        ha, hb = np.zeros(num_rays, np.int32), np.zeros(num_rays, np.int32)
        secs = np.zeros(2, np.float64)
        self.L.h_bench_point(n, num_rays, world, _p(s), _p(ra), _p(rb), _p(ha), _p(hb), _p(secs))
        return {"spheres": s, "rays_no_bvh": ra, "rays_bvh": rb, "hit_no_bvh": ha, "hit_bvh": hb,
                "secs": (float(secs[0]), float(secs[1]))}

    def srand(self, seed):
        self.L.h_srand(seed)

    def render_scene(self, seed, n):
        out = np.zeros(n, abi.SPHERE)
        self.L.h_gen_render_scene(seed, n, _p(out))
        return out

    def bench_scene(self, seed, n, world=1000.0):
        out = np.zeros(n, abi.SPHERE)
        self.L.h_gen_bench_scene(seed, n, world, _p(out))
        return out

    def build(self, spheres, start=0, end=None, depth=0):
        end = len(spheres) if end is None else end
        return self.L.h_build(_p(spheres), start, end, depth)

    def flatten(self, tree, spheres):
        n = self.L.h_node_count(tree)
        out = np.zeros(n, abi.NODE)
        assert self.L.h_flatten(tree, _p(spheres), _p(out), n) == n
        return out

    def leaf_counts(self, tree):
        n = self.L.h_node_count(tree)
        out = np.zeros(n, np.int32)
        k = self.L.h_leaf_counts(tree, _p(out))
        return out[:k]

    def free(self, tree):
        self.L.h_free(tree)

    def intersect(self, tree, spheres, rays):
        out = np.zeros(len(rays), abi.HIT)
        self.L.h_intersect_bvh(tree, _p(spheres), _p(rays), len(rays), _p(out))
        return out

    def sphere_pairs(self, rays, spheres):
        out = np.zeros(len(rays), abi.HIT)
        self.L.h_sphere_pairs(_p(rays), _p(spheres), len(rays), _p(out))
        return out

    def aabb_pairs(self, rays, boxes):
        out = np.zeros(len(rays), np.int32)
        self.L.h_aabb_pairs(_p(rays), _p(boxes), len(rays), _p(out))
        return out

    def camera_rays(self, cam, rows=None):
        rows = range(self.H) if rows is None else rows
        out = np.zeros((len(rows), self.W), abi.RAY)
        r1 = np.zeros(1, abi.RAY)
        c = abi.Camera.from_buffer_copy(bytes(cam))
        for i, y in enumerate(rows):
            for x in range(self.W):
                self.L.h_camera_ray(C.byref(c), x, y, _p(r1))
                out[i, x] = r1[0]
        return out

    def render(self, cam, spheres, tree, depth=5, use_bvh=True, mode=1, seed=1, sample=0,
               row0=0, step=1, nrows=None, threads=1, jitter=False):
        """mode 0: call srand(seed) then render with the glibc stream (the
        unmodified reference); mode 1: the per-pixel contract."""
        nrows = (self.H - row0 + step - 1) // step if nrows is None else nrows
        out = np.zeros((nrows, self.W, 4), np.uint8)
        if mode == 0:
            self.L.h_srand(seed)
        self.L.h_render(C.byref(cam), _p(spheres), len(spheres), tree, depth, int(use_bvh), mode, seed, sample,
                        row0, step, nrows, _p(out), threads, int(jitter))
        return out

    def trace_rays(self, rays, spheres, tree, depth=5, use_bvh=True, mode=1, seed=1, sample=0):
        out = np.zeros((len(rays), 4), np.uint8)
        if mode == 0:
            self.L.h_srand(seed)
        self.L.h_trace_rays(_p(rays), len(rays), _p(spheres), len(spheres), tree, depth, int(use_bvh),
                            mode, seed, sample, _p(out))
        return out

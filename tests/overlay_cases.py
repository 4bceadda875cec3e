"""The BVH overlay (mirt_bvh_overlay) at its edges: the inputs of
tests/test_overlay_edges_host.py (the oracle alone, no GPU) and
tests/test_overlay_edges_gpu.py. A case is (scene, camera, (W, H), max_levels);
its expected image is oracle.bvh_overlay of the scene's tree, computed once,
cached and read-only.

Scenes, by name (`scene(name)` -> spheres, the oracle's tree handle, flat nodes):

  r1000, r2, r1, r0   render_scene(1, n) built by the oracle (2181, 3, 1 and 1 nodes)
  no_tree             five spheres uploaded without a tree: 0 nodes, the cleared canvas
  coincident          the 50 coincident spheres of test_device_build.test_degenerate:
                      chains of empty leaves that carry the inverted (empty) box
  cluster             make_golden_layouts' cluster scene (3240 spheres, 40 x 6 coincident)
  hand_falling, hand_chain70, hand_chain300, hand_sticks_out
                      make_golden_layouts.hand_trees: trees of no builder, through
                      oracle.tree_from_flat; hand_chain300's nodes reach depth 300,
                      past the one-byte depth (MIRT_LAYOUT_NDEPTH, clamped to 255)
  nan_c_16th, inf_c_4th
                      hostile_sphere_cases scenes: 181 of 2115 and all 159 node boxes hold
                      +-inf (no builder writes a NaN into a box: fminf / fmaxf drop it)
  nan_boxes           r1000's flat tree with a NaN written into every 5th node's bmin.y
                      and every 7th node's bmax.z, through oracle.tree_from_flat

Cameras, by name: fields are set directly (no camera_update), so the basis may
be skewed, zero or huge and the position non-finite. `face` and `chain` depend
on the scene: 0.1 in front of the root box's largest z, and (60, 0, 120) with
fov 60 looking down -z at the hand trees' row of spheres along x.

CASES is the pruned list the GPU file runs; the host file shows which cases
draw, which give the cleared canvas, and that the corner classes occur.
"""
import functools
import importlib.util
import os

import numpy as np

import hostile_sphere_cases as sc
import test_planes_cases as cases

abi = cases.abi
F32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
CLEAR = np.array([0, 0, 0, 255], np.uint8)

_spec = importlib.util.spec_from_file_location(
    "make_golden_layouts", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

BUILT = ("r1000", "r2", "r1", "r0", "coincident", "cluster")
HAND = ("hand_falling", "hand_chain70", "hand_chain300", "hand_sticks_out")
HOSTILE = ("nan_c_16th", "inf_c_4th")
SCENES = BUILT + ("no_tree",) + HAND + HOSTILE + ("nan_boxes",)

CAMERAS = ("default", "inside", "away", "face", "skew", "fov1", "fov170", "fov180", "fov0", "fov-45", "fov_nan",
           "pos_nan", "pos_inf", "pos_1e30", "fwd_zero", "fwd_1e20")
# on r1000 at 160 x 90 these draw nothing (test_overlay_edges_host asserts the cleared canvas exactly) ...
DARK = ("away", "fov0", "fov_nan", "pos_nan", "pos_inf", "fwd_zero")
# ... and every other one lights pixels

SIZES = ((1, 1), (1, 7), (7, 1), (5, 3), (257, 3), (3, 257), (130, 9), (64, 64), (160, 90))
LEVELS = (0, 1, 2, 5, 20, 21, 22, 40, 41, INT_MAX, -1, -2, INT_MIN)    # r1000's deepest node has depth 40
CHAIN_LEVELS = (-1, 254, 255, 256, 257, 300, 301)              # hand_chain300's has depth 300


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _mirt():
    return importlib.import_module("cs201_sah-bvh_ray_tracer_amd")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(spheres as uploaded, the oracle's tree handle or None, the flat nodes)."""
    o = cases._oracle()
    if name == "r1000":
        return cases.scene(1000)
    if name in HOSTILE:
        return sc.scene(name)
    if name == "no_tree":
        return _frozen(o.render_scene(1, 5)), None, _frozen(np.zeros(0, abi.NODE))
    if name in BUILT:
        if name == "coincident":
            s = np.zeros(50, abi.SPHERE)
            s["center"] = [1.0, 2.0, 3.0]
            s["radius"] = 0.5
        elif name == "cluster":
            mirt = _mirt()
            base = mirt.create_random_spheres(3000, 7)
            cl = np.repeat(base[:40], 6)
            cl["color"][:, 2] ^= (np.arange(len(cl)) % 6 * 37).astype(np.uint8)
            s = np.concatenate([base, cl])
        else:
            s = o.render_scene(1, int(name[1:]))
        tree = o.build(s)
        return _frozen(s), tree, _frozen(o.flatten(tree))
    if name == "nan_boxes":
        s, _, nodes = cases.scene(1000)
        nodes = nodes.copy()
        nodes["bmin"][::5, 1] = np.nan
        nodes["bmax"][::7, 2] = np.nan
        return s, o.tree_from_flat(nodes), _frozen(nodes)
    if name in HAND:
        s, nodes = gen.hand_trees(_mirt())[name]
        nodes = np.ascontiguousarray(nodes, abi.NODE)
        return _frozen(s), o.tree_from_flat(nodes), _frozen(nodes)
    raise KeyError(name)


def depths(nodes):
    """Every node's true depth (int32): the children of inner node i are i + 1
    and the left child's skip."""
    d = np.zeros(max(len(nodes), 1), np.int32)
    skip = (nodes["skip"] & abi.SKIP_MASK).astype(np.int64)
    for i in range(len(nodes)):
        if nodes["sphere"][i] < 0:
            d[i + 1] = d[skip[i + 1]] = d[i] + 1
    return d[:len(nodes)]


def camera(name, scene_name="r1000"):
    cam = abi.default_camera()
    V = abi.Vec3
    if name == "default":
        pass
    elif name == "inside":
        cam.position = V(0.0, 0.0, 0.0)
    elif name == "away":
        cam.position = V(0.0, 4.0, -200.0)
    elif name == "face":
        nodes = scene(scene_name)[2]
        z = (F32(nodes["bmax"][0][2]) if len(nodes) else F32(0.0)) + F32(0.1)
        cam.position = V(0.0, 4.0, float(z))
    elif name == "chain":
        cam.position = V(60.0, 0.0, 120.0)
        cam.fov = 60.0
    elif name == "skew":
        cam.forward = V(0.1, 0.0, -1.0)
        cam.right = V(1.0, 0.3, 0.0)
        cam.up = V(0.2, 1.5, 0.1)
    elif name.startswith("fov"):
        cam.fov = float("nan") if name == "fov_nan" else float(name[3:])
    elif name == "pos_nan":
        cam.position = V(float("nan"), 4.0, 50.0)
    elif name == "pos_inf":
        cam.position = V(0.0, 4.0, float("inf"))
    elif name == "pos_1e30":
        cam.position = V(0.0, 4.0, 1e30)
    elif name == "fwd_zero":
        cam.forward = V(0.0, 0.0, 0.0)
    elif name == "fwd_1e20":
        cam.forward = V(0.0, 0.0, -1e20)
    else:
        raise KeyError(name)
    return cam


def _cases():
    out = []
    big = (160, 90)
    out += [("r1000", c, big, -1) for c in CAMERAS]
    out += [("r1000", c, size, -1) for c in ("inside", "default") for size in SIZES[:-1]]
    out += [("r1000", "default", big, lv) for lv in LEVELS if lv != -1]
    out += [("r1000", "inside", (64, 64), lv) for lv in (5, 20, 21, 22, 40, 41, INT_MAX, -2, INT_MIN)]
    out += [("r1000", "skew", (130, 9), 5), ("r1000", "fov-45", (257, 3), 21)]
    for name in ("r2", "r1", "r0", "no_tree", "coincident", "cluster") + HOSTILE + ("nan_boxes",):
        out += [(name, "default", big, -1), (name, "inside", (64, 64), -1), (name, "face", (130, 9), 2),
                (name, "default", (5, 3), 1)]
    out += [("coincident", "default", big, lv) for lv in (39, 40, 41)]
    for name in HAND:
        out += [(name, "chain", big, -1), (name, "default", (64, 64), -1), (name, "chain", (130, 9), 2),
                (name, "inside", (257, 3), -1)]
    out += [("hand_chain300", "chain", big, lv) for lv in CHAIN_LEVELS if lv != -1]
    out += [("hand_chain300", "chain", (130, 9), lv) for lv in (255, 256, 300)]
    out += [("hand_chain70", "chain", big, lv) for lv in (69, 70, 71)]
    assert len(set(out)) == len(out)
    return tuple(out)


CASES = _cases()


def cases_of(scene_name):
    return [c for c in CASES if c[0] == scene_name]


@functools.lru_cache(maxsize=None)
def expected(scene_name, cam_name, size, levels):
    """oracle.bvh_overlay of the case: (H, W, 4) uint8."""
    return overlay_of(scene(scene_name)[1], camera(cam_name, scene_name), size, levels)


def overlay_of(tree, cam, size, levels=-1):
    """oracle.bvh_overlay of a tree handle (None: no tree, the cleared canvas)."""
    w, h = size
    if tree is None:
        out = np.zeros((h, w, 4), np.uint8)
        out[:] = CLEAR
        return _frozen(out)
    return _frozen(cases._oracle().bvh_overlay(tree, cam, w, h, levels))


def lit(img):
    return int((img != CLEAR).any(-1).sum())


def depth_colour(d):
    return (255 - (d * 40) % 200, (d * 80) % 200, (d * 120) % 200, 180)


def corners(nodes):
    """(n, 8, 3) float32: every node's corners in draw_aabb's order."""
    lo, hi = nodes["bmin"], nodes["bmax"]
    k = np.arange(8)
    hx, hy, hz = np.isin(k, (1, 2, 5, 6)), np.isin(k, (2, 3, 6, 7)), k >= 4
    return np.stack([np.where(hx, hi[:, None, 0], lo[:, None, 0]), np.where(hy, hi[:, None, 1], lo[:, None, 1]),
                     np.where(hz, hi[:, None, 2], lo[:, None, 2])], -1).astype(F32)


def project(cam, p, w, h):
    """world_to_screen (bvh_visualiser.c:16-41) in float32 over an array of
    points (..., 3): a dict of the float z, sx, sy, the classes `behind` (z <=
    0.1), `outside` (the float range test, of those not behind), `nan_z`, and
    of the points that pass both tests the integer x and y as x86's
    conversion gives them (INT_MIN for a NaN or a value out of range)."""
    v = lambda a: np.array([a.x, a.y, a.z], F32)
    with np.errstate(all="ignore"):
        t = np.asarray(p, F32) - v(cam.position)
        dot = lambda b: (t[..., 0] * b[0] + t[..., 1] * b[1]) + t[..., 2] * b[2]
        z, x, y = dot(v(cam.forward)), dot(v(cam.right)), dot(v(cam.up))
        fov = F32(np.float64(cam.fov) * (np.pi / 180.0))
        hh = F32(np.tan(fov / F32(2)))
        hw = F32(F32(w) / F32(h)) * hh
        sx = (x / (z * hw * F32(2)) + F32(0.5)) * F32(w)
        sy = (-y / (z * hh * F32(2)) + F32(0.5)) * F32(h)
        behind = z <= F32(0.1)
        outside = ~behind & ((sx < -w) | (sx > 2 * w) | (sy < -h) | (sy > 2 * h))
        ok = ~behind & ~outside

        def trunc(s):
            fits = (s > F32(-2147483648.0)) & (s < F32(2147483648.0))
            return np.where(fits, np.trunc(np.where(fits, s, 0)), INT_MIN).astype(np.int64)
    return dict(z=z, sx=sx, sy=sy, behind=behind, outside=outside, ok=ok, nan_z=np.isnan(z), ix=trunc(sx), iy=trunc(sy))


# ---------------------------------------------------------------- mirt_camera_rays_uv

UV_SIZES = ((160, 90), (77, 45), (1, 1))
UV_BATCHES = (1, 2, 255, 256, 257, 4097)


def uv_cameras(small):
    """The default camera, the goldens' camera 1 and one fuzz camera (seeded, through camera_update)."""
    mirt = _mirt()
    rng = np.random.default_rng(77)
    fuzz = mirt.default_camera()
    fuzz.position = abi.Vec3(*map(float, rng.uniform(-70.0, 70.0, 3)))
    fuzz.yaw = F32(rng.uniform(-np.pi, np.pi))
    fuzz.pitch = F32(rng.uniform(-1.4, 1.4))
    fuzz.fov = float(rng.uniform(20.0, 90.0))
    mirt.camera_update(fuzz)
    return {"default": mirt.default_camera(), "camera1": abi.Camera.from_numpy(small["cameras"][1]), "fuzz": fuzz}


def pixel_uv(w, h):
    """(h, w, 2) float32: the (u, v) the frame's pixel loop passes to
    get_camera_ray (main.c:356-365; oracle.c o_camera_ray_px): v negated."""
    aspect = F32(w) / F32(h)
    xf = np.broadcast_to(np.arange(w, dtype=F32)[None, :], (h, w))
    yf = np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w))
    u = (xf / F32(w) - F32(0.5)) * aspect
    v = -(yf / F32(h) - F32(0.5))
    return np.stack([u, v], -1).astype(F32)


def uv_rays(cam, w, h, uv):
    """camera_uv_kernel restated in float32: direction = normalize3(forward +
    horizontal * u + vertical * v), horizontal = right * (2 half_w), vertical
    = up * (2 half_h) (render.hip make_frame_const)."""
    import lens_frame_cases as lc
    uv = np.asarray(uv, F32)
    with np.errstate(all="ignore"):
        aspect = F32(w) / F32(h)
        fov_rad = F32(np.float64(cam.fov) * (np.pi / 180.0))
        half_h = F32(np.tan(np.float64(fov_rad / F32(2.0))))
        half_w = aspect * half_h
        hor = lc._vec(cam.right) * (F32(2.0) * half_w)
        ver = lc._vec(cam.up) * (F32(2.0) * half_h)
        d = lc._vec(cam.forward) + hor * uv[..., 0, None]
        d = (d + ver * uv[..., 1, None]).astype(F32)
        d = lc.normalize(d)
    out = np.zeros(uv.shape[:-1], abi.RAY)
    out["origin"] = lc._vec(cam.position)
    out["direction"] = d
    return out


def hostile_uv():
    """(n, 2) float32: every pair of the edge values, then seeded mixtures."""
    sub = np.float32(1e-42)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 2.5, -2.5, sub, -sub, 1e30, -1e30, np.inf, -np.inf, np.nan,
                     np.finfo(F32).max, np.finfo(F32).tiny], F32)
    pairs = np.stack(np.meshgrid(vals, vals, indexing="ij"), -1).reshape(-1, 2)
    rng = np.random.default_rng(78)
    mix = rng.uniform(-3.0, 3.0, (300, 2)).astype(F32)
    k = rng.random((300, 2)) < 0.25
    mix[k] = rng.choice(vals, int(k.sum()))
    return _frozen(np.concatenate([pairs, mix]).astype(F32))

"""The denoiser's definition (csrc/denoise.h, mirt.h mirt_denoise_params)
restated in numpy, one float32 operation per operation of the definition and in
its order, and the cases its tests run, from the oracle and a seeded generator
alone (no GPU).

For an image of W x H pixels, colours c (u8 / 255.0f of an RGBA8 display, or
a / (float)frames of float3 sums), guides sphere (< 0: a miss) and normal:
pass i = 0 .. passes - 1 has spacing s = 2^i and visits the taps
q = p + (dx s, dy s), dy = -2 .. 2 outermost, dx innermost. A tap outside the
image or on another sphere contributes nothing; else w = B[dy + 2] * B[dx + 2],
B = {1/16, 1/4, 3/8, 1/4, 1/16}; off the centre, with normals and
sphere[p] >= 0, d = nx nx' ; d = d + ny ny'; d = d + nz nz'; m = max(d, 0);
m = m * m k times; w = w * m; with sigma > 0, g = er er; g = g + eg eg;
g = g + eb eb; w = w * (1 / (1 + g * inv_i)), inv_0 = 1 / (sigma * sigma),
inv_{i+1} = inv_i * 4. sw = sw + w, sc = sc + c_q * w in visiting order from
+0; the pass's colour is sc / sw. The display is (u8)(int)min(c * 255, 255),
alpha 255.

Cases (CASES): the rendered ones are test_planes_cases' case A (44 x 26, 1000
spheres: 5.5 x 3.25 tiles of 8 x 8) -- "A0" .. "A3" the oracle's one-sample
frames of samples 0 .. 3 with the oracle's planes, "Asum" their float sum as an
accum source with frames = 4; the synthetic ones are seeded: sphere ids from
{-1, 0, 1, 2}, unit normals (zero on misses), random colours, at the sizes of
SIZES, and at 33 x 65 all-miss, one sphere everywhere, and a checkerboard of
nine ids with period 3 in x and y, where every pixel filters alone: an offset
of 2^i or 2^(i+1) is never a multiple of 3. Spacing 16 on the 26 rows of case
A, and on every synthetic image smaller than 33, puts taps off both edges.
"""
import ctypes as C
import functools
import itertools

import numpy as np

import test_planes_cases as cases

abi = cases.abi
F32 = np.float32
B = [F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625)]
W, H, N = 44, 26, 1000
SIZES = [(1, 1), (1, 37), (37, 1), (2, 2), (5, 3), (64, 1), (33, 65), (129, 70)]   # (width, height)
# (passes, normal_sharpness, sigma_colour, with the normal plane)
PARAMS = list(itertools.product((1, 2, 3, 4, 5), (0, 3, 7), (0.0, 0.5), (True, False)))
DEFAULT = (3, 3, 0.0, True)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def oracle_frame(sample):
    """The oracle's one-sample frame of case A, (H, W, 4) u8."""
    spheres, tree, _ = cases.scene(N)
    out = cases._oracle().render(cases.camera("A"), W, H, spheres, tree, depth=5, seed=1, sample=sample)
    out = np.ascontiguousarray(out.reshape(H, W, 4))
    out.setflags(write=False)
    return out


def _synthetic(width, height, seed, pattern="random", source="rgba"):
    rng = np.random.default_rng(seed)
    if pattern == "random":
        sphere = rng.integers(-1, 3, (height, width)).astype(np.int32)
    elif pattern == "miss":
        sphere = np.full((height, width), -1, np.int32)
    elif pattern == "one":
        sphere = np.full((height, width), 2, np.int32)
    else:   # a checkerboard of nine ids with period 3: no tap of any spacing 2^i meets the pixel's own id
        y, x = np.mgrid[0:height, 0:width]
        sphere = ((x % 3) + 3 * (y % 3)).astype(np.int32)
    n = rng.standard_normal((height, width, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    n[sphere < 0] = 0.0
    case = dict(width=width, height=height, sphere=sphere, normal=n, rgba=None, accum=None, frames=1)
    if source == "rgba":
        rgba = rng.integers(0, 256, (height, width, 4)).astype(np.uint8)
        rgba[..., 3] = 255
        case["rgba"] = rgba
    else:
        case["frames"] = 3
        case["accum"] = (rng.random((height, width, 3)) * 3.0).astype(F32)
    return _frozen(case)


@functools.lru_cache(maxsize=None)
def case(name):
    """{"width", "height", "rgba" | "accum", "frames", "sphere", "normal"}; read-only."""
    if name.startswith("A"):
        pl = cases.expected("A")
        out = dict(width=W, height=H, sphere=pl["sphere"], normal=pl["normal"], rgba=None, accum=None, frames=1)
        if name == "Asum":
            acc = np.zeros((H, W, 3), F32)
            for s in range(4):
                acc = acc + oracle_frame(s)[..., :3].astype(F32) / F32(255.0)
            out["accum"], out["frames"] = acc, 4
        else:
            out["rgba"] = oracle_frame(int(name[1:]))
        return _frozen(out)
    kind, w, h = name.split("_")
    return _synthetic(int(w), int(h), seed=1000 * int(w) + int(h),
                      pattern=kind if kind in ("miss", "one", "checker") else "random",
                      source="accum" if kind == "acc" else "rgba")


CASES = ["A0", "A1", "A2", "A3", "Asum"] + [f"syn_{w}_{h}" for w, h in SIZES] + \
        ["acc_5_3", "acc_33_65", "miss_33_65", "one_33_65", "checker_33_65"]


def source_colours(c):
    if c["rgba"] is not None:
        return c["rgba"][..., :3].astype(F32) / F32(255.0)
    return c["accum"] / F32(c["frames"])


def display(rgb):
    """(u8)(int)fminf(c * 255, 255) per channel, alpha 255."""
    v = np.minimum(rgb * F32(255.0), F32(255.0)).astype(np.int32)
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = (v & 0xFF).astype(np.uint8)
    return out


def restate(c, passes, k, sigma, with_normal):
    """(out (H, W, 4) u8, out_rgb (H, W, 3) f32) of the definition, in numpy."""
    w_, h_ = c["width"], c["height"]
    sphere = c["sphere"]
    normal = c["normal"] if with_normal else None
    col = source_colours(c)
    assert col.dtype == F32
    inv = F32(1.0) / (F32(sigma) * F32(sigma)) if sigma > 0 else None
    ys, xs = np.arange(h_), np.arange(w_)
    use_n = sphere >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(passes):
            s = 1 << i
            sw = np.zeros((h_, w_), F32)
            sc = np.zeros((h_, w_, 3), F32)
            for dy in range(-2, 3):
                qy = ys + dy * s
                in_y = (qy >= 0) & (qy < h_)
                qy = np.clip(qy, 0, h_ - 1)
                for dx in range(-2, 3):
                    qx = xs + dx * s
                    in_x = (qx >= 0) & (qx < w_)
                    qx = np.clip(qx, 0, w_ - 1)
                    q = np.ix_(qy, qx)
                    take = in_y[:, None] & in_x[None, :] & (sphere[q] == sphere)
                    cq = col[q]
                    wt = np.full((h_, w_), B[dy + 2] * B[dx + 2], F32)
                    if dx or dy:
                        if normal is not None:
                            nq = normal[q]
                            d = normal[..., 0] * nq[..., 0]
                            d = d + normal[..., 1] * nq[..., 1]
                            d = d + normal[..., 2] * nq[..., 2]
                            m = np.maximum(d, F32(0.0))
                            for _ in range(k):
                                m = m * m
                            wt = np.where(use_n, wt * m, wt)
                        if inv is not None:
                            e = col - cq
                            g = e[..., 0] * e[..., 0]
                            g = g + e[..., 1] * e[..., 1]
                            g = g + e[..., 2] * e[..., 2]
                            wt = wt * (F32(1.0) / (F32(1.0) + g * inv))
                    assert wt.dtype == F32
                    sw = np.where(take, sw + wt, sw)
                    sc = np.where(take[..., None], sc + cq * wt[..., None], sc)
            col = sc / sw[..., None]
            assert col.dtype == F32
            if inv is not None:
                inv = inv * F32(4.0)
    return display(col), col


@functools.lru_cache(maxsize=None)
def expected(name, params):
    out, rgb = restate(case(name), *params)
    out.setflags(write=False)
    rgb.setflags(write=False)
    return out, rgb


def params_struct(params):
    passes, k, sigma, _ = params
    return abi.DenoiseParams(passes, k, sigma)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host(lib, c, params, want_out=True, want_rgb=True):
    """mirt_denoise_host on a case: (out, out_rgb), None for an output not asked for."""
    h_, w_ = c["height"], c["width"]
    out = np.zeros((h_, w_, 4), np.uint8) if want_out else None
    rgb = np.zeros((h_, w_, 3), F32) if want_rgb else None
    p = params_struct(params)
    rc = lib.mirt_denoise_host(w_, h_, _p(c["rgba"]), _p(c["accum"]), c["frames"], _p(c["sphere"]),
                               _p(c["normal"]) if params[3] else None, C.byref(p), _p(out), _p(rgb))
    assert rc == 0, lib.mirt_last_error().decode()
    return out, rgb


def host_filter(lib, width, height, sphere, normal, params, rgba=None, accum=None, frames=1):
    """The host filter's display of any source (contiguous arrays)."""
    c = dict(width=width, height=height, sphere=np.ascontiguousarray(sphere, np.int32),
             normal=np.ascontiguousarray(normal, F32),
             rgba=None if rgba is None else np.ascontiguousarray(rgba, np.uint8),
             accum=None if accum is None else np.ascontiguousarray(accum, F32), frames=frames)
    return host(lib, c, params, want_rgb=False)[0]


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} bytes differ"

"""The cases of the primary-hit planes' tests and what the planes must hold,
from the oracle alone (no GPU): a case's expected planes are the t, sphere and
normal fields of oracle.intersect(tree, spheres, oracle.camera_rays(cam, W, H,
rows), use_bvh). The tests here assert that the cases cover their ground;
tests/test_planes_gpu.py imports the cases from here.

  A: 44 x 26, the default camera, render_scene(1, 1000): hits, misses and the
     zero-component rays of the image's centre row and column (those the
     unordered schedules hand to deferred waves), over more than one 8x8 tile
     with overhang in both directions (44 = 5.5 tiles, 26 = 3.25)
  B: the same scene from z = 600, fov 6: a camera beyond four times the
     scene's origin bound (the unbounded ordered instantiation)
  C: 256 x 144, render_scene(1, 10000)
"""
import functools
import importlib

import numpy as np

from oracle.lib import Oracle

abi = importlib.import_module("cs201_sah-bvh_ray_tracer_amd").abi

CASES = {
    "A": dict(W=44, H=26, n=1000, z=50.0, fov=45.0),
    "B": dict(W=44, H=26, n=1000, z=600.0, fov=6.0),
    "C": dict(W=256, H=144, n=10000, z=50.0, fov=45.0),
}


def camera(name):
    cam = abi.default_camera()
    cam.position.z = CASES[name]["z"]
    cam.fov = CASES[name]["fov"]
    return cam


@functools.lru_cache(maxsize=None)
def _oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def scene(n):
    """(spheres as the oracle's build reordered them, its tree handle, the flat
    tree): built once per size and never changed."""
    o = _oracle()
    spheres = o.render_scene(1, n)
    tree = o.build(spheres)
    nodes = o.flatten(tree)
    spheres.setflags(write=False)
    nodes.setflags(write=False)
    return spheres, tree, nodes


@functools.lru_cache(maxsize=None)
def rays(name):
    c = CASES[name]
    out = _oracle().camera_rays(camera(name), c["W"], c["H"])
    out.setflags(write=False)
    return out


def planes_of(hits, shape):
    """The three planes of an abi.HIT array, shaped like the frame."""
    hits = np.asarray(hits).reshape(shape)
    return {"t": np.ascontiguousarray(hits["t"]), "sphere": np.ascontiguousarray(hits["sphere"]),
            "normal": np.ascontiguousarray(hits["normal"])}


def intersect(n, some_rays, use_bvh=True):
    """The oracle's hit records of any rays against the scene of n spheres."""
    spheres, tree, _ = scene(n)
    return _oracle().intersect(tree, spheres, np.ascontiguousarray(some_rays).reshape(-1), use_bvh)


@functools.lru_cache(maxsize=None)
def expected(name, use_bvh=True):
    """{"t", "sphere", "normal"} of the case, (H, W[, 3]); read-only."""
    c = CASES[name]
    pl = planes_of(intersect(c["n"], rays(name), use_bvh), (c["H"], c["W"]))
    for a in pl.values():
        a.setflags(write=False)
    return pl


def zero_component(name):
    """Pixels whose camera ray has a direction component of exactly zero."""
    return (rays(name)["direction"] == 0.0).any(axis=-1)


def counts(name, use_bvh=True):
    pl = expected(name, use_bvh)
    hit = pl["sphere"] >= 0
    zc = zero_component(name)
    return dict(hits=int(hit.sum()), misses=int((~hit).sum()), zero=int(zc.sum()), zero_hits=int((zc & hit).sum()))


def test_a_miss_is_zero_minus_one_zero():
    for name in ("A", "B"):
        for use_bvh in (True, False):
            pl = expected(name, use_bvh)
            miss = pl["sphere"] < 0
            assert (pl["sphere"][miss] == -1).all() and not pl["t"][miss].view(np.uint32).any()
            assert not pl["normal"][miss].view(np.uint32).any()
            assert (pl["t"][~miss] > 0).all() and (pl["sphere"][~miss] < CASES[name]["n"]).all()
            assert np.allclose(np.linalg.norm(pl["normal"][~miss], axis=-1), 1.0, atol=1e-5)


def test_case_a_covers_hits_misses_and_zero_component_rays():
    for use_bvh in (True, False):
        c = counts("A", use_bvh)
        print("case A", "bvh" if use_bvh else "brute", c)
        assert c["hits"] >= 200 and c["misses"] >= 200 and c["zero_hits"] >= 20, c
    # the centre column (26 rays) and the centre row (44), one pixel shared
    assert counts("A")["zero"] == 69


def test_case_b_covers_hits_and_misses_from_far_away():
    c = counts("B")
    print("case B", c)
    assert c["hits"] >= 100 and c["misses"] >= 100, c


def test_case_c_has_hits_and_misses():
    c = counts("C")
    print("case C", c)
    assert c["hits"] > 0 and c["misses"] > 0

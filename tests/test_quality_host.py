"""mirt_bvh_quality_flat (csrc/bvh_quality.cpp): the SAH quality of a flat tree,
against a restatement of the definition in include/mirt.h written here -- the
box area in numpy float32 in the stated operation order, the terms and sums in
Python integers -- field for field and bit for bit. The sums are integers, so
there is no tolerance anywhere."""
import ctypes as C
import importlib.util
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_layouts", os.path.join(GOLDEN, "make_golden_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

E_INVALID = -1
F4 = np.float32
FLOATS = ("inner_area", "leaf_area", "overhead", "cost")
INTS = ("inner_nodes", "leaves", "dead_leaves", "clamped", "degenerate")


def dbits(x):
    return struct.pack("<d", x)


def assert_same_quality(got, want, what=""):
    for k in FLOATS:
        assert dbits(got[k]) == dbits(want[k]), f"{what}: {k} is {got[k]!r}, the restatement has {want[k]!r}"
    assert struct.pack("<f", got["root_area"]) == struct.pack("<f", want["root_area"]), (what, "root_area")
    for k in INTS:
        assert got[k] == want[k], f"{what}: {k} is {got[k]}, the restatement has {want[k]}"
    assert set(got) == set(FLOATS) | set(INTS) | {"root_area"}


def areas(nodes):
    """box_area of bvh.c:48-57 for every node: fp32, one rounding per operation."""
    with np.errstate(all="ignore"):
        d = nodes["bmax"].astype(F4) - nodes["bmin"].astype(F4)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        s = dx * dy
        s = s + dy * dz
        s = s + dz * dx
        out = F4(2.0) * s
    assert out.dtype == F4
    return out


def terms(mirt, nodes, ns):
    """Per node: (kind, term) with kind 'inner' / 'leaf' / 'dead', and the
    number of clamped terms, e, A0 -- or None for a degenerate root."""
    area = areas(nodes)
    a0 = float(area[0])
    kinds = []
    for n in nodes:
        if n["sphere"] < 0:
            kinds.append("inner")
        elif (int(n["skip"]) & mirt.abi.NODE_EMPTY) or n["sphere"] >= ns:
            kinds.append("dead")
        else:
            kinds.append("leaf")
    if not (a0 > 0.0 and math.isfinite(a0)):
        return kinds, None, 0, 0, area[0]
    e = math.frexp(a0)[1]                       # a0 = m 2^e with m in [0.5, 1): ilogb(a0) + 1
    assert 2.0 ** (e - 1) <= a0 < 2.0 ** e
    scale = Fraction(2) ** (48 - e)
    out, clamped = [], 0
    for k, a in zip(kinds, area):
        a = float(a)
        if k == "dead":
            out.append(0)
        elif not a >= 0.0:
            out.append(0)
            clamped += 1
        elif a > a0:
            out.append(1 << 48)
            clamped += 1
        else:
            out.append(math.floor(Fraction(a) * scale))
            assert out[-1] < 1 << 48
    return kinds, out, clamped, e, area[0]


def quality_restated(mirt, nodes, ns):
    zero = dict.fromkeys(FLOATS, 0.0)
    zero.update(dict.fromkeys(INTS, 0), root_area=0.0)
    if len(nodes) == 0:
        return zero
    kinds, t, clamped, e, a0 = terms(mirt, nodes, ns)
    q = dict(zero, root_area=float(a0), inner_nodes=kinds.count("inner"), leaves=kinds.count("leaf"),
             dead_leaves=kinds.count("dead"))
    if t is None:
        q["degenerate"] = 1
        return q

    def total(kind):
        hi = sum(x >> 24 for k, x in zip(kinds, t) if k == kind)
        lo = sum(x & 0xFFFFFF for k, x in zip(kinds, t) if k == kind)
        return math.ldexp(float(hi) * 2.0 ** 24 + float(lo), e - 48)

    q["clamped"] = clamped
    q["inner_area"], q["leaf_area"] = total("inner"), total("leaf")
    if q["leaf_area"] == 0.0:
        q["overhead"] = 0.0 if q["inner_area"] == 0.0 else math.inf
    else:
        q["overhead"] = q["inner_area"] / q["leaf_area"]
    q["cost"] = 0.125 * q["overhead"] + 1.0
    return q


def moved_centres(s, sigma, seed):
    """test_refit_host's `moved`, on the centres only."""
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(F4)
    return out


def duplicates(mirt):
    s = mirt.create_random_spheres(64, 5)
    s[8:40] = s[8]
    return s


@pytest.fixture(scope="module")
def built(mirt):
    """name -> (spheres in the scene's order, nodes, end)"""
    out = {}
    for n in (1000, 10000):
        s = mirt.create_random_spheres(n, 1)
        out[f"render_{n}"] = (s, mirt.build_bvh(s).nodes, n)
    s = mirt.create_benchmark_spheres(1000, 1)
    out["bench_1000"] = (s, mirt.build_bvh(s, 0, 999, 20).nodes, 999)      # benchmark.c:317
    s = duplicates(mirt)
    out["duplicates_64"] = (s, mirt.build_bvh(s).nodes, 64)
    for name, (s, nodes) in gen.hand_trees(mirt).items():
        out[name] = (s, nodes, len(s))
    return out


NAMES = ("render_1000", "render_10000", "bench_1000", "duplicates_64", "hand_falling", "hand_chain70",
         "hand_chain300", "hand_sticks_out", "hand_nan_centre")


@pytest.mark.parametrize("name", NAMES)
def test_definition_against_the_restatement(mirt, built, name):
    s, nodes, _ = built[name]
    keep = nodes.copy()
    got = mirt.bvh_quality(nodes, len(s))
    assert nodes.tobytes() == keep.tobytes()
    assert_same_quality(got, quality_restated(mirt, nodes, len(s)), name)
    assert_same_quality(mirt.bvh_quality(mirt.Bvh(nodes), len(s)), got, name)
    assert got["inner_nodes"] + got["leaves"] + got["dead_leaves"] == len(nodes)
    assert got["degenerate"] == 0 and got["cost"] > 1.0
    if name == "render_10000":
        assert (len(nodes), got["inner_nodes"], got["leaves"], got["clamped"]) == (29399, 14699, 9811, 0)
    if name.startswith(("render", "bench", "duplicates")):        # a builder's boxes nest
        assert got["clamped"] == 0


@pytest.mark.parametrize("name", ("render_1000", "render_10000", "bench_1000", "duplicates_64"))
def test_refit_to_the_same_spheres_keeps_the_quality(mirt, built, name):
    s, nodes, end = built[name]
    again = mirt.refit_bvh(nodes, s, end)
    assert_same_quality(mirt.bvh_quality(again, len(s)), mirt.bvh_quality(nodes, len(s)), name)


@pytest.mark.parametrize("factor", [2.0, 0.5])
@pytest.mark.parametrize("name", ("render_1000", "render_10000", "duplicates_64"))
def test_uniform_scaling_keeps_the_overhead(mirt, built, name, factor):
    """Centres and radii times a power of two are exact in fp32, so every area
    is exactly 4x or 1/4x and every term is the same integer."""
    s, nodes, end = built[name]
    s2 = s.copy()
    s2["center"] *= F4(factor)
    s2["radius"] *= F4(factor)
    base = mirt.bvh_quality(nodes, len(s))
    got = mirt.bvh_quality(mirt.refit_bvh(nodes, s2, end), len(s))
    assert dbits(got["overhead"]) == dbits(base["overhead"]) and dbits(got["cost"]) == dbits(base["cost"])
    assert got["root_area"] == base["root_area"] * factor * factor
    assert got["inner_area"] == base["inner_area"] * factor * factor
    assert_same_quality(got, quality_restated(mirt, mirt.refit_bvh(nodes, s2, end).nodes, len(s)), name)


def test_clamped_terms(mirt, built):
    s, nodes, _ = built["render_1000"]
    ns = len(s)
    base = mirt.bvh_quality(nodes, ns)
    live = np.nonzero((nodes["sphere"] >= 0) & ((nodes["skip"] & mirt.abi.NODE_EMPTY) == 0) & (nodes["sphere"] < ns))[0]
    leaf = int(live[len(live) // 2])
    big = nodes.copy()
    big["bmin"][leaf] = nodes["bmin"][0] - F4(1.0)
    big["bmax"][leaf] = nodes["bmax"][0] + F4(1.0)
    kinds, t, clamped, e, _ = terms(mirt, big, ns)
    assert kinds[leaf] == "leaf" and t[leaf] == 1 << 48 and clamped == 1
    got = mirt.bvh_quality(big, ns)
    assert got["clamped"] == 1 and got["leaf_area"] > base["leaf_area"]
    assert dbits(got["inner_area"]) == dbits(base["inner_area"])
    assert_same_quality(got, quality_restated(mirt, big, ns), "a leaf larger than the root")
    nan = nodes.copy()
    nan["bmax"][leaf][2] = np.nan
    kinds, t, clamped, e, _ = terms(mirt, nan, ns)
    assert t[leaf] == 0 and clamped == 1
    got = mirt.bvh_quality(nan, ns)
    assert got["clamped"] == 1 and got["leaf_area"] < base["leaf_area"]
    assert_same_quality(got, quality_restated(mirt, nan, ns), "a NaN coordinate")
    inner = nodes.copy()
    inner["bmin"][1][0] = np.nan                  # node 1 of a 1000-sphere tree is an inner node
    assert nodes["sphere"][1] < 0
    got = mirt.bvh_quality(inner, ns)
    assert got["clamped"] == 1 and got["inner_area"] < base["inner_area"]
    assert_same_quality(got, quality_restated(mirt, inner, ns), "a NaN coordinate in an inner node")


def test_other_cases(mirt):
    L, p = mirt.load(), mirt.abi.ptr
    q = mirt.abi.TreeQuality()
    C.memset(C.byref(q), 0xAB, C.sizeof(q))
    assert L.mirt_bvh_quality_flat(None, 0, 5, C.byref(q)) == 0
    assert bytes(q) == bytes(C.sizeof(q))
    assert_same_quality(mirt.bvh_quality(np.zeros(0, mirt.abi.NODE), 5), quality_restated(mirt, [], 5), "no tree")
    s = mirt.create_random_spheres(1, 1)
    leaf = mirt.build_bvh(s).nodes
    got = mirt.bvh_quality(leaf, 1)
    assert len(leaf) == 1 and got["leaves"] == 1 and got["inner_nodes"] == 0
    assert got["overhead"] == 0.0 and got["cost"] == 1.0 and got["degenerate"] == 0
    assert_same_quality(got, quality_restated(mirt, leaf, 1), "single leaf")
    s["radius"] = 0.0
    point = mirt.build_bvh(s).nodes
    got = mirt.bvh_quality(point, 1)
    assert got["degenerate"] == 1 and got["leaves"] == 1 and got["root_area"] == 0.0
    assert got["cost"] == 0.0 and got["overhead"] == 0.0 and got["leaf_area"] == 0.0 and got["clamped"] == 0
    assert_same_quality(got, quality_restated(mirt, point, 1), "zero radius")
    # a root whose area is infinite is degenerate too
    inf = leaf.copy()
    inf["bmax"][0][0] = np.inf
    got = mirt.bvh_quality(inf, 1)
    assert got["degenerate"] == 1 and math.isinf(got["root_area"])
    assert_same_quality(got, quality_restated(mirt, inf, 1), "infinite root")
    # a malformed tree is refused by the validation every upload runs
    bad = np.array([gen._node(-1, 3), gen._node(0, 2), gen._node(7, 3)], mirt.abi.NODE)
    C.memset(C.byref(q), 0xAB, C.sizeof(q))
    assert L.mirt_bvh_quality_flat(p(bad), 3, 3, C.byref(q)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_bvh_quality_flat: malformed node 2 (sphere 7, skip 3)"
    assert bytes(q) == b"\xab" * C.sizeof(q)
    with pytest.raises(mirt.MirtError, match="malformed node 2"):
        mirt.bvh_quality(bad, 3)
    assert L.mirt_bvh_quality_flat(p(bad), 3, 3, None) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_bvh_quality_flat: invalid arguments"
    assert L.mirt_bvh_quality_flat(None, 3, 3, C.byref(q)) == E_INVALID
    assert L.mirt_bvh_quality_flat(p(bad), -1, 3, C.byref(q)) == E_INVALID


@pytest.mark.parametrize("name", ("render_1000", "render_10000"))
def test_decay_follows_the_motion(mirt, built, name):
    """cost of the refit tree over cost of the built tree: diffusing spheres
    make it grow with the distance travelled, a small shake leaves it near 1."""
    s, nodes, end = built[name]
    base = mirt.bvh_quality(nodes, len(s))["cost"]
    decay = {}
    for sigma in (0.05, 3.0, 10.0):
        s2 = moved_centres(s, sigma, 7)
        decay[sigma] = mirt.bvh_quality(mirt.refit_bvh(nodes, s2, end), len(s))["cost"] / base
    print(name, decay)
    assert decay[10.0] > decay[3.0] > 1.1 > decay[0.05] > 0.9, decay

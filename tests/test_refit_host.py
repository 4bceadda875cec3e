"""mirt_bvh_refit_flat (csrc/bvh_refit.cpp): the boxes of a flat tree recomputed
bottom-up from moved spheres, topology untouched. Checked against a numpy
restatement of the definition in include/mirt.h written here, bit for bit: the
boxes are exact min / max, so there is no tolerance anywhere."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_layouts", os.path.join(GOLDEN, "make_golden_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

E_INVALID = -1
F4 = np.float32


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def classify(mirt, nodes, ns):
    """(live, dead) masks over the nodes: hit-able leaves and the other leaves."""
    leaf = nodes["sphere"] >= 0
    empty = (nodes["skip"] & mirt.abi.NODE_EMPTY) != 0
    live = leaf & ~empty & (nodes["sphere"] < ns)
    return live, leaf & ~live


def ranges(mirt, nodes, ns, end):
    """The hit-able leaves' node indices and their sphere ranges [first, last)."""
    live, _ = classify(mirt, nodes, ns)
    idx = np.nonzero(live)[0]
    first = nodes["sphere"][idx].astype(np.int64)
    assert (np.diff(first) > 0).all() and (len(first) == 0 or first[-1] < end) and 0 <= end <= ns
    return idx, first, np.append(first[1:], end)


def refit_numpy(mirt, nodes, s, end):
    """The definition, restated: leaf boxes fold fl(c - r), fl(c + r) over the
    leaf's range from the empty box, inner boxes combine their children's, a
    dead leaf counts as the empty box and keeps its bytes."""
    out = nodes.copy()
    nn, ns = len(nodes), len(s)
    idx, first, last = ranges(mirt, nodes, ns, end)
    lo = (s["center"] - s["radius"][:, None]).astype(F4)
    hi = (s["center"] + s["radius"][:, None]).astype(F4)
    bmin = np.full((nn, 3), np.inf, F4)
    bmax = np.full((nn, 3), -np.inf, F4)
    for i, a, b in zip(idx, first, last):
        for k in range(a, b):
            bmin[i] = np.fmin(bmin[i], lo[k])
            bmax[i] = np.fmax(bmax[i], hi[k])
    skip = (nodes["skip"] & mirt.abi.SKIP_MASK).astype(np.int64)
    inner = nodes["sphere"] < 0
    for i in range(nn - 1, -1, -1):
        if inner[i]:
            l, r = i + 1, skip[i + 1]
            bmin[i] = np.fmin(bmin[l], bmin[r])
            bmax[i] = np.fmax(bmax[l], bmax[r])
    _, dead = classify(mirt, nodes, ns)
    out["bmin"][~dead] = bmin[~dead]
    out["bmax"][~dead] = bmax[~dead]
    return out


def check_nesting(mirt, nodes, s, end):
    """Every inner box holds its children's boxes, every leaf box its range."""
    ns = len(s)
    _, dead = classify(mirt, nodes, ns)
    skip = (nodes["skip"] & mirt.abi.SKIP_MASK).astype(np.int64)
    inner = np.nonzero(nodes["sphere"] < 0)[0]
    for child in (inner + 1, skip[inner + 1]):
        ok = dead[child] | ((nodes["bmin"][inner] <= nodes["bmin"][child]).all(axis=1) &
                            (nodes["bmax"][inner] >= nodes["bmax"][child]).all(axis=1))
        assert ok.all()
    lo = (s["center"] - s["radius"][:, None]).astype(F4)
    hi = (s["center"] + s["radius"][:, None]).astype(F4)
    idx, first, last = ranges(mirt, nodes, ns, end)
    owner = np.repeat(idx, last - first)           # the leaf of every sphere in [s_0, end)
    k = np.arange(first[0], end) if len(first) else np.zeros(0, np.int64)
    assert (nodes["bmin"][owner] <= lo[k]).all() and (nodes["bmax"][owner] >= hi[k]).all()


def duplicates(mirt):
    s = mirt.create_random_spheres(64, 5)
    s[8:40] = s[8]
    return s


def moved(s, sigma, seed):
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(F4)
    out["radius"] *= r.uniform(0.5, 1.5, len(s)).astype(F4)
    return out


@pytest.fixture(scope="module")
def built(mirt):
    """name -> (spheres in the scene's order, the builder's nodes, end)"""
    out = {}
    s = mirt.create_random_spheres(1000, 2)
    out["render_1000_2"] = (s, mirt.build_bvh(s).nodes, 1000)
    s = mirt.create_random_spheres(10000, 1)
    out["render_10000_1"] = (s, mirt.build_bvh(s).nodes, 10000)
    for n in (1000, 100000):
        s = mirt.create_benchmark_spheres(n, 1)
        out[f"bench_{n}"] = (s, mirt.build_bvh(s, 0, n - 1, 20).nodes, n - 1)     # benchmark.c:317
    s = duplicates(mirt)
    out["duplicates_64"] = (s, mirt.build_bvh(s).nodes, 64)
    return out


NAMES = ("render_1000_2", "render_10000_1", "bench_1000", "bench_100000", "duplicates_64")


@pytest.mark.parametrize("name", NAMES)
def test_identity(mirt, built, name):
    """Unchanged spheres: the builder's tree, bit for bit."""
    s, nodes, end = built[name]
    mirt.validate_bvh(nodes, len(s))
    before_s, before_n = s.copy(), nodes.copy()
    got = mirt.refit_bvh(nodes, s, end)
    assert same(got.nodes, nodes)
    assert same(s, before_s) and same(nodes, before_n)       # refit_bvh works on a copy
    assert same(mirt.refit_bvh(mirt.Bvh(nodes), s, end).nodes, nodes)
    if name.startswith(("render", "duplicates")):            # not vacuous: stuck groups and dead leaves
        _, dead = classify(mirt, nodes, len(s))
        _, first, last = ranges(mirt, nodes, len(s), end)
        assert (last - first > 1).any() and dead.any(), name


@pytest.mark.parametrize("sigma", [0.05, 3.0])
@pytest.mark.parametrize("name", ("render_1000_2", "render_10000_1", "bench_1000", "duplicates_64"))
def test_moved(mirt, built, name, sigma):
    s, nodes, end = built[name]
    s2 = moved(s, sigma, 7)
    got = mirt.refit_bvh(nodes, s2, end).nodes
    want = refit_numpy(mirt, nodes, s2, end)
    assert same(got["sphere"], nodes["sphere"]) and same(got["skip"], nodes["skip"])
    assert same(got, want)
    assert not same(got, nodes)
    mirt.validate_bvh(got, len(s2))
    check_nesting(mirt, got, s2, end)
    info, _ = mirt.scene_layout(s2, got)
    assert info["encloses"] == 1 and info["ordered"] == 1 and info["o_bound"] > 0.0


def test_moved_100k(mirt, built):
    s, nodes, end = built["bench_100000"]
    s2 = moved(s, 0.5, 3)
    got = mirt.refit_bvh(nodes, s2, end).nodes
    idx, first, last = ranges(mirt, nodes, len(s), end)
    # the leaves, vectorised: a range of one sphere takes the sphere's own box
    one = last - first == 1
    assert one.sum() > 90000
    assert same(got["bmin"][idx[one]], (s2["center"] - s2["radius"][:, None]).astype(F4)[first[one]])
    assert same(got["bmax"][idx[one]], (s2["center"] + s2["radius"][:, None]).astype(F4)[first[one]])
    mirt.validate_bvh(got, len(s))
    check_nesting(mirt, got, s2, end)


@pytest.mark.parametrize("name", ("render_1000_2", "bench_1000", "duplicates_64"))
def test_there_and_back(mirt, built, name):
    """A -> B -> A returns A's bytes: a refit depends on nothing but topology and spheres."""
    s, nodes, end = built[name]
    b = mirt.refit_bvh(nodes, moved(s, 3.0, 11), end)
    assert not same(b.nodes, nodes)
    assert same(mirt.refit_bvh(b, s, end).nodes, nodes)


def test_errors_leave_the_nodes_untouched(mirt, built):
    L, p = mirt.load(), mirt.abi.ptr
    s, nodes = gen.hand_trees(mirt)["hand_falling"]
    work = nodes.copy()
    assert L.mirt_bvh_refit_flat(p(work), len(work), p(s), len(s), len(s)) == E_INVALID
    assert L.mirt_last_error().decode() == ("mirt_bvh_refit_flat: node 2 holds sphere 0 after sphere 1: "
                                            "the leaves' spheres do not increase")
    assert same(work, nodes)
    with pytest.raises(mirt.MirtError, match="do not increase"):
        mirt.refit_bvh(nodes, s)
    s, nodes, end = built["render_1000_2"]
    s2 = moved(s, 3.0, 1)
    _, first, _ = ranges(mirt, nodes, len(s), end)
    for bad_end in (int(first[-1]), int(first[-1]) - 5, 0, -1, len(s) + 1):
        work = nodes.copy()
        assert L.mirt_bvh_refit_flat(p(work), len(work), p(s2), len(s2), bad_end) == E_INVALID, bad_end
        assert L.mirt_last_error().decode().startswith("mirt_bvh_refit_flat: end"), bad_end
        assert same(work, nodes), bad_end
    work = nodes.copy()
    assert L.mirt_bvh_refit_flat(p(work), len(work), p(s2), len(s2), int(first[-1]) + 1) == 0
    assert L.mirt_bvh_refit_flat(None, len(work), p(s2), len(s2), len(s2)) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_bvh_refit_flat: invalid arguments"
    work = nodes.copy()
    assert L.mirt_bvh_refit_flat(p(work), len(work), None, len(s2), len(s2)) == E_INVALID
    assert same(work, nodes)
    # a malformed tree is refused by the validation every upload runs
    bad = np.array([gen._node(-1, 3), gen._node(0, 2), gen._node(7, 3)], mirt.abi.NODE)
    keep = bad.copy()
    assert L.mirt_bvh_refit_flat(p(bad), 3, p(s2), 3, 3) == E_INVALID
    assert L.mirt_last_error().decode() == "mirt_bvh_refit_flat: malformed node 2 (sphere 7, skip 3)"
    assert same(bad, keep)


def test_no_tree_is_ok(mirt):
    L, p = mirt.load(), mirt.abi.ptr
    s = mirt.create_random_spheres(5, 1)
    assert L.mirt_bvh_refit_flat(None, 0, p(s), 5, 5) == 0
    assert L.mirt_bvh_refit_flat(None, 0, p(s), 5, 0) == 0
    assert L.mirt_bvh_refit_flat(None, 0, None, 0, 0) == 0
    assert L.mirt_bvh_refit_flat(None, 0, p(s), 5, 6) == E_INVALID
    assert len(mirt.refit_bvh(np.zeros(0, mirt.abi.NODE), s)) == 0


def test_deep_monotone_chain_refits(mirt):
    """hand_chain70: too deep for the ordered walks, but its leaves' spheres
    increase: the host refits it (the device path hands it over)."""
    s, nodes = gen.hand_trees(mirt)["hand_chain70"]
    assert mirt.scene_layout(s, nodes)[0]["ordered"] == 0
    s2 = moved(s, 0.5, 2)
    got = mirt.refit_bvh(nodes, s2).nodes
    assert same(got, refit_numpy(mirt, nodes, s2, len(s2)))
    check_nesting(mirt, got, s2, len(s2))
    assert mirt.scene_layout(s2, got)[0]["encloses"] == 1


def test_dead_leaves_keep_their_bytes(mirt, built):
    s, nodes, end = built["render_1000_2"]
    got = mirt.refit_bvh(nodes, moved(s, 3.0, 5), end).nodes
    _, dead = classify(mirt, nodes, len(s))
    assert dead.any() and same(got[dead], nodes[dead])

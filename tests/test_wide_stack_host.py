"""The trees of wide_stack_cases.py do what the GPU tests need them to do,
shown on the CPU alone: the push rule's model overflows on each of them (and
not on the control), their layouts admit the ordered four-wide walk, hit.c's
result on them does not depend on the padded inner boxes, and their frames and
ray batches are not vacuous. Also records why such trees are needed: a walk
that passed every inner slot of the golden render scenes of up to 10,000
spheres would still fit the 20-entry stack.
"""
import numpy as np
import pytest

import wide_stack_cases as W

NAMES = list(W.CASES)


@pytest.fixture(scope="module")
def layouts(mirt):
    return {name: mirt.scene_layout(W.case(name).spheres, W.case(name).nodes) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_model_overflows_in_the_kernels_order(layouts, name):
    """At cap 20 a complete walk overflows at least once on every overflowing
    tree, under each visit order its walks can take (wide_stack_cases.py says
    which and why); the control overflows under none."""
    c = W.case(name)
    info, parts = layouts[name]
    for order in c.orders:
        overflows, peak = W.stack_model(parts, info, W.CAP, order)
        print(f"{name} {order}: {overflows} overflows, peak {peak}")
        if c.overflows:
            assert overflows >= 1 and peak > W.CAP, (name, order, overflows, peak)
        else:
            assert overflows == 0 and peak <= W.CAP, (name, order, overflows, peak)
    if c.overflows and not W.CASES[name].get("graft_n"):
        # the spine alone, nearest first: three pairs wait per level
        assert W.stack_model(parts, info, W.CAP, "nearest")[1] == 3 * c.K


@pytest.mark.parametrize("name", NAMES)
def test_layouts_admit_the_wide_walk(layouts, name):
    abi = W.abi
    c = W.case(name)
    info, parts = layouts[name]
    assert info["ordered"] == 1 and info["encloses"] == 1
    ref = parts["hnodes"]["slot"]["ref"]
    inner = ((ref != abi.P_NONE) & ((ref & abi.P_LEAF) == 0)).sum(axis=1)
    assert int((inner == 4).sum()) >= c.K          # every spine HNode: four inner slots
    # what a segment walks: HAux's flat node and its skip, inside the tree; every slot reference in range
    # (from wide_root on: the walks never visit HNode 0, the root box alone)
    nn = len(c.nodes)
    assert len(parts["haux"]) == len(ref) == info["num_hnodes"] and info["wide_root"] == 1
    haux = parts["haux"][1:]
    assert (haux["flat"] < nn).all() and (c.nodes["sphere"][haux["flat"]] < 0).all()
    assert (haux["end"] == (c.nodes["skip"][haux["flat"]] & abi.SKIP_MASK)).all() and (haux["end"] <= nn).all()
    live = ref != abi.P_NONE
    leaf = live & ((ref & abi.P_LEAF) != 0)
    assert (ref[live & ~leaf] < info["num_hnodes"]).all() and ((ref[leaf] & abi.P_INDEX) < info["num_leaves"]).all()
    if W.CASES[name].get("far"):
        # c_max >= 6.0e4: no origin bound (the BND = false walks), fp16 slot boxes saturated
        assert info["c_max"] >= 6.0e4 and info["o_bound"] == 0.0
        box = parts["hnodes"]["slot"]["box"][ref != abi.P_NONE]
        hi = (box >> 16).astype(np.uint16).view(np.float16)
        assert np.isinf(hi).any() or (hi == np.float16(65504)).any()
    else:
        assert info["o_bound"] > 0.0
    # the twins are there
    s = c.spheres
    geo = np.concatenate([s["center"], s["radius"][:, None]], axis=1)
    twins = len(s) - len(np.unique(geo, axis=0))
    assert twins == (1 if W.CASES[name].get("twin") else 0)


@pytest.mark.parametrize("n,lo,hi,fits", [(1000, 11, 14, True), (10000, 17, 20, True), (100000, 21, 24, False)])
def test_golden_render_scenes_and_the_stack(mirt, n, lo, hi, fits):
    """The record: a walk passing EVERY inner slot of the golden render scenes
    peaks at 11-14 (1,000 spheres) and 17-20 (10,000) entries, in slot order
    and in reverse -- within the 20-entry stack, and real walks prune. So no
    frame of those scenes enters a fallback; hand-written trees do. At
    100,000 spheres the full visit peaks at 21-24: a few pixels of the golden
    1080p frame of that scene do reach a fallback, nothing smaller
    does."""
    s = mirt.create_random_spheres(n, 1)
    info, parts = mirt.scene_layout(s, mirt.build_bvh(s))
    for order in ("slot", "reverse"):
        overflows, peak = W.stack_model(parts, info, W.CAP, order)
        print(f"render {n} {order}: {overflows} overflows, peak {peak}")
        assert lo <= peak <= hi and (overflows == 0) == fits, (n, order, overflows, peak)


@pytest.fixture(scope="module")
def camera_rays(oracle):
    return {(name, W_, H): oracle.camera_rays(W.case(name).cam, W_, H).reshape(-1)
            for name in NAMES for W_, H in W.SIZES}


@pytest.mark.parametrize("name", NAMES)
def test_padded_boxes_do_not_change_the_hits(oracle, camera_rays, name):
    """The containment argument on these inputs: hit.c over the padded tree
    equals hit.c over the same tree with exact boxes, byte for byte, for the
    frames' camera rays and the rays from inside the box."""
    c = W.case(name)
    for rays in [camera_rays[name, W_, H] for W_, H in W.SIZES] + [W.inside_rays(name)]:
        padded = oracle.intersect_flat(c.nodes, c.spheres, rays)
        exact = oracle.intersect_flat(c.exact, c.spheres, rays)
        assert padded.tobytes() == exact.tobytes(), name
    # and the pointer tree the oracle's frames are rendered from is this tree
    t = oracle.tree_from_flat(c.nodes)
    assert oracle.flatten(t).tobytes() == c.nodes.tobytes()
    got = oracle.intersect(t, c.spheres, W.inside_rays(name))
    oracle.free(t)
    assert got.tobytes() == oracle.intersect_flat(c.nodes, c.spheres, W.inside_rays(name)).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_frames_and_batches_are_not_vacuous(oracle, camera_rays, name):
    """At least 25% of every test frame's camera rays hit, and at least 20% of
    the rays from inside the box (a condition on the scenes, met by placing
    the camera: the oracle alone decides it). A twin never wins: hit.c gives
    the tie to the later sphere."""
    c = W.case(name)
    for W_, H in W.SIZES:
        hits = oracle.intersect_flat(c.nodes, c.spheres, camera_rays[name, W_, H])
        assert hits["hit"].mean() >= 0.25, (name, W_, H, hits["hit"].mean())
    hits = oracle.intersect_flat(c.nodes, c.spheres, W.inside_rays(name))
    assert hits["hit"].mean() >= 0.20, (name, hits["hit"].mean())
    if W.CASES[name].get("twin"):
        s = c.spheres
        a, b = [(a, a + 1) for a in range(len(s) - 1)
                if s["radius"][a] == s["radius"][a + 1] and (s["center"][a] == s["center"][a + 1]).all()][0]
        assert int((hits["sphere"] == a).sum()) == 0 and int((hits["sphere"] == b).sum()) > 0

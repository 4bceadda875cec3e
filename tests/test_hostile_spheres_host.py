"""The hostile sphere scenes (tests/hostile_sphere_cases.py) on the CPU: the
oracle held to the unmodified reference (tests/golden/hostile_spheres.json,
made by tests/golden/make_golden_hostile_spheres.py), the host builder and the
scene layout held to the oracle byte for byte, and what the reference does with
the scenes, so that the GPU file's comparisons are not vacuous. The counts are
the reference's, never the product's; MEASUREMENTS.md records them.

test_host_builder_gives_the_oracles_tree is the regression test of
bvh_build.cpp's inverted-box rule: before it, a node whose spheres have
negative radii (box c - r > c + r) was split by bins that assume increasing
planes, and neg_r_4th gave 3159 nodes where the reference gives 2237.
"""
import functools
import json
import os

import numpy as np
import pytest

import hostile_sphere_cases as sc
import test_planes_cases as cases
from conftest import GOLDEN, sha

with open(os.path.join(GOLDEN, "hostile_spheres.json")) as _f:
    REF = json.load(_f)["scenes"]

NON_FINITE = tuple(n for n in sc.SCENES if n[:5] in ("nan_r", "nan_c", "inf_r", "inf_c"))
NEGATIVE = ("neg_r_sparse", "neg_r_4th", "neg_r_all")
# what layout_rules.h and scene_layout.cpp state, per scene: a non-finite sphere, or a leaf box that does not
# hold fl(c -+ |r|) (an inverted one cannot), turns pruning off; C >= 6.0e4 or no pruning leaves no origin bound
ENCLOSES_0 = NON_FINITE + NEGATIVE
O_BOUND_0 = ENCLOSES_0 + ("huge_r_sparse", "huge_r_4th", "far_c_sparse", "far_c_4th", "giant_wall", "giant_dome_61000")
CHAINS = ("inf_r_4th", "inf_c_4th", "huge_r_4th", "far_c_4th")


def _hit(records):
    return records["hit"] != 0


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def test_golden_covers_the_scenes():
    assert list(REF) == list(sc.SCENES)


def test_the_scenes_are_what_the_docstring_says():
    base = sc.base()
    assert len(base) == sc.N and base.tobytes() == cases._oracle().render_scene(1, sc.N).tobytes()
    assert 0.4 < base["radius"].min() and base["radius"].max() < 5.1 and np.isfinite(base["center"]).all()
    for name in sc.SCENES:
        s, m = sc.inputs(name)
        changed = np.array([s[i].tobytes() != base[i].tobytes() for i in range(sc.N)])
        assert (changed <= m).all() and changed.sum() >= min(3, m.sum()), name
        assert name in ("dups", "neg_hidden") or s["color"].tobytes() == base["color"].tobytes()
        if name.endswith("_sparse") or name == "giant_inplace":
            assert list(np.flatnonzero(m)) == list(sc.FIXED), name
        if name.endswith("_4th"):
            assert m.sum() == 250
        if name.endswith("_16th"):
            assert m.sum() == 63
        assert sc.hostile(name).sum() == m.sum() and not sc.scene(name)[0].flags.writeable
    for name in NEGATIVE:
        s, m = sc.inputs(name)
        assert (s["radius"][m] == -base["radius"][m]).all() and (s["radius"][~m] > 0).all()
    r = sc.inputs("tiny_r")[0]["radius"][1::2]
    k = sc.exponents("tiny_r")[1::2]
    assert k.min() == 10 and k.max() == 140 and (r > 0).all()
    subnormal = r < np.float32(2.0 ** -126)
    assert subnormal.sum() >= 20 and (r * r == 0).sum() >= 200 and (r[k < 70] * r[k < 70] > 0).all()
    k = sc.exponents("scales")
    assert k.min() == -16 and k.max() == 2
    assert (sc.inputs("scales")[0]["radius"] == base["radius"] * np.float32(2.0) ** k.astype(np.float32)).all()
    for name, values in (("nan_r_16th", ()), ("inf_r_4th", (np.inf, -np.inf))):
        r = sc.inputs(name)[0]["radius"][sc.inputs(name)[1]]
        assert np.isnan(r).all() if not values else all((r == v).sum() >= 100 for v in values)
    for name in ("nan_c_16th", "inf_c_4th"):
        c = sc.inputs(name)[0]["center"][sc.inputs(name)[1]]
        bad = ~np.isfinite(c)
        assert (bad.sum(1) == 1).all() and bad.any(0).all(), name            # one component each, every component
    c = sc.inputs("inf_c_4th")[0]["center"]
    assert (c == np.inf).any() and (c == -np.inf).any()
    r = sc.inputs("huge_r_4th")[0]["radius"][::4]
    assert r.min() >= 2.0 ** 20 and r.max() >= 2.0 ** 126 and np.isfinite(r).all()
    with np.errstate(over="ignore"):
        assert np.isinf(r * r).sum() >= 100 and np.isfinite(r * r).sum() >= 50
    assert list(sc.inputs("huge_r_sparse")[0]["radius"][list(sc.FIXED)]) == [2.0 ** 20, 2.0 ** 64, 2.0 ** 127]
    c = np.abs(sc.inputs("far_c_4th")[0]["center"][::4]).max(1)
    assert np.isfinite(c).all() and c.max() > 1e30 and c.min() < 1e6
    h = sc.inputs("neg_hidden")[0]
    assert h["radius"][0] == -6.0 and h["center"][0].tobytes() == h["center"][1].tobytes() and h["radius"][1] > 0
    assert np.abs(h["radius"][1:]).max() < 6.0
    d = sc.inputs("dups")[0]
    assert d[1::2].tobytes() == d[0::2].tobytes() and d[0::2].tobytes() == base[0::2].tobytes()
    w = sc.inputs("giant_wall")[0]
    assert w["radius"][0] == 3.0e4 and (w["center"][0, 2] + 3.0e4 <= (base["center"][:, 2] - base["radius"]).min() + 0.01)
    assert [float(sc.inputs(f"giant_dome_{r}")[0]["radius"][0]) for r in (50000, 59900, 61000)] == [5.0e4, 5.99e4, 6.1e4]
    assert list(sc.inputs("giant_inplace")[0]["radius"][list(sc.FIXED)]) == [1.0e3, 3.0e4, 5.9e4]
    s = sc.inputs("dust_scene")[0]
    assert (s["center"] == base["center"] * np.float32(2.0 ** -10)).all()
    assert (s["radius"] == base["radius"] * np.float32(2.0 ** -20)).all()
    assert (sc.inputs("dust_radii")[0]["radius"] == base["radius"] * np.float32(2.0 ** -12)).all()


# ---------------------------------------------------------------- the oracle against the reference

@functools.lru_cache(maxsize=None)
def _rays_160x90():
    return cases._oracle().camera_rays(cases.camera("A"), 160, 90).reshape(-1)


@pytest.mark.parametrize("name", sc.SCENES)
def test_oracle_equals_the_reference(oracle, name):
    """oracle.c's reordered spheres, flat tree, 160 x 90 hit records and depth-5
    frames (tree and brute force) are the unmodified reference's, byte for byte."""
    s, tree, nodes = sc.scene(name)
    want = REF[name]
    assert len(nodes) == want["nodes"]
    assert sha(s) == want["spheres"] and sha(nodes) == want["tree"]
    assert sha(oracle.intersect(tree, s, _rays_160x90())) == want["hits"]
    cam = cases.camera("A")
    assert sha(oracle.render(cam, 160, 90, s, tree, depth=5, mode=1, seed=1)) == want["frame_tree"]
    assert sha(oracle.render(cam, 160, 90, s, tree, depth=5, mode=1, seed=1, use_bvh=False)) == want["frame_brute"]


# ---------------------------------------------------------------- the host side against the oracle

def restated(abi, s, nd):
    """encloses, ordered, r_max, c_max and o_bound as csrc/scene_layout.cpp and csrc/layout_rules.h state them,
    from the spheres and the flat tree alone."""
    ns, nn = len(s), len(nd)
    c, r = s["center"], np.abs(s["radius"])
    skip = (nd["skip"] & abi.SKIP_MASK).astype(np.int64)
    empty = (nd["skip"] & abi.NODE_EMPTY) != 0
    sphere = nd["sphere"].astype(np.int64)
    leaf = sphere >= 0
    live = leaf & ~empty & (sphere < ns)
    encloses = bool(np.isfinite(c).all() and np.isfinite(r).all())
    r_max = c_max = np.float32(0.0)
    if encloses:
        k = sphere[live]
        with np.errstate(over="ignore"):
            lo, hi = c - r[:, None], c + r[:, None]                      # float32, as bvh.c:26-35
        encloses = bool((nd["bmin"][live] <= lo[k]).all() and (nd["bmax"][live] >= hi[k]).all())
        inner = np.flatnonzero(~leaf)
        for child in (inner + 1, skip[inner + 1]):
            holds = empty[child] | ((nd["bmin"][inner] <= nd["bmin"][child]) & (nd["bmax"][inner] >= nd["bmax"][child])).all(1)
            encloses = encloses and bool(holds.all())
        if encloses:
            r_max = r.max()
            with np.errstate(over="ignore"):
                c_max = (np.abs(c).max(1) + r).max()
    tested = np.zeros(ns + 1, bool)
    tested[sphere[live]] = True
    orphan = bool((leaf & (sphere < ns) & empty & ~tested[np.clip(sphere, 0, ns)]).any())
    encloses = encloses and not orphan
    box = np.concatenate([nd["bmin"][~empty], nd["bmax"][~empty]]).astype(np.float64)
    box = np.abs(box[np.isfinite(box)])
    cb = max(float(c_max), float(box.max()) if box.size else 0.0) * (1.0 + 2.0 ** -10) + 2.0 ** -10
    o_bound = np.float32(cb) if encloses and cb < 6.0e4 else np.float32(0.0)
    ends, depth, last, mono = [], 0, -1, nn > 0
    for i in range(nn):
        while ends and ends[-1] <= i:
            ends.pop()
        if not leaf[i]:
            ends.append(int(skip[i]))
            depth = max(depth, len(ends))
        elif live[i]:
            mono = mono and sphere[i] > last
            last = sphere[i]
    return dict(encloses=int(encloses), ordered=int(mono and depth + 2 <= 64), r_max=r_max, c_max=c_max, o_bound=o_bound)


@pytest.mark.parametrize("name", sc.SCENES)
def test_host_builder_gives_the_oracles_tree(mirt, name):
    s, _, nodes = sc.scene(name)
    mine = sc.inputs(name)[0].copy()
    b = mirt.build_bvh(mine)
    assert len(b.nodes) == len(nodes), f"{name}: {len(b.nodes)} nodes, the reference has {len(nodes)}"
    assert mine.tobytes() == s.tobytes(), f"{name}: the sphere order differs"
    assert b.nodes.tobytes() == nodes.tobytes(), name


@pytest.mark.parametrize("name", sc.SCENES)
def test_validate_and_layout_on_the_oracles_tree(mirt, name):
    s, _, nodes = sc.scene(name)
    mirt.validate_bvh(nodes, len(s))
    info, parts = mirt.scene_layout(s, mirt.Bvh(nodes))
    want = restated(mirt.abi, s, nodes)
    print(name, {k: info[k] for k in want}, "depth", sc.tree_depth(nodes))
    for k in ("encloses", "ordered"):
        assert info[k] == want[k], (name, k, info[k], want[k])
    for k in ("r_max", "c_max", "o_bound"):
        assert fbits(info[k]) == fbits(want[k]), (name, k, info[k], want[k])
    assert info["ordered"] == 1                       # the reference's builds partition in place, depth <= 40
    assert (info["encloses"] == 0) == (name in ENCLOSES_0), name
    assert (info["o_bound"] == 0) == (name in O_BOUND_0), name
    assert info["num_pnodes"] == 1 + int((nodes["sphere"] < 0).sum())
    if name == "neg_hidden":   # the untested twin's |r| is the scene's largest
        assert info["encloses"] == 1 and info["r_max"] == 6.0


def test_which_scenes_walk_unpruned_and_which_without_an_origin_bound(mirt):
    """The record: encloses == 0 (no pruning), o_bound == 0 (every bounce ray
    takes the exact box test), and both."""
    rows = {}
    for name in sc.SCENES:
        info, _ = mirt.scene_layout(sc.scene(name)[0], mirt.Bvh(sc.scene(name)[2]))
        rows[name] = (info["encloses"] == 0, info["o_bound"] == 0)
    print("encloses == 0:", [n for n, v in rows.items() if v[0]])
    print("o_bound == 0 only:", [n for n, v in rows.items() if v[1] and not v[0]])
    print("bounded and pruned:", [n for n, v in rows.items() if not v[1]])
    assert [n for n, v in rows.items() if v[0]] == [n for n in sc.SCENES if n in ENCLOSES_0]
    assert all(v[1] for v in rows.values() if v[0])   # no pruning implies no bound
    # the dome at 5.99e4 keeps its bound, the one at 6.1e4 loses it: the threshold of layout_bound
    assert not rows["giant_dome_59900"][1] and rows["giant_dome_61000"][1]


# ---------------------------------------------------------------- not vacuous

def test_hostile_spheres_are_hit():
    """Every family whose hostile spheres can be hit has a ray set with at
    least 50 primary hits on them in the reference (the tree walk's, except
    where the tree hides the sphere: then brute force's)."""
    for family, scenes in sc.HIT_FAMILIES.items():
        rows = {(n, *rs): (int(sc.on_hostile(n, *rs).sum()), int(sc.on_hostile(n, *rs, use_bvh=False).sum()))
                for n in scenes for rs in sc.ray_sets(n)}
        print(family, "(scene, camera, w, h) -> primary hits on hostile spheres (tree, brute force):", rows)
        assert max(max(v) for v in rows.values()) >= 50, family
        if family != "huge_r sparse":   # there hit.c's walk tests only the first sphere of the leaf that holds them
            assert max(v[0] for v in rows.values()) >= 50, family
    # negative radii: hit.c squares r and normalises p - c, so the sphere itself is the positive one's, outward
    # normal included; only its box, and so the tree around it, differs
    rec = sc.hits("neg_r_4th", "A", 44, 26)
    on = sc.on_hostile("neg_r_4th", "A", 44, 26)
    s = sc.scene("neg_r_4th")[0]
    assert on.sum() >= 50 and (s["radius"][rec["sphere"][on]] < 0).all()
    out = rec["point"][_hit(rec)] - s["center"][rec["sphere"][_hit(rec)]]
    assert ((out * rec["normal"][_hit(rec)]).sum(-1) > 0).all()
    # the wall: every ray hits something, the wall at t of about 3e4 to 6e4: its discriminant is beyond 2^30
    rec, on = sc.hits("giant_wall", "A", 44, 26), sc.on_hostile("giant_wall", "A", 44, 26)
    assert _hit(rec).all() and rec["t"][on].min() > 50.0 and rec["t"][on].max() < 7.0e4
    # scales: hits on spheres scaled down and up
    rec, on = sc.hits("scales", "A", 44, 26), sc.on_hostile("scales", "A", 44, 26)
    r = sc.scene("scales")[0]["radius"][rec["sphere"][on]]
    print("scales: radii of the spheres hit from", r.min(), "to", r.max())
    assert r.min() < 2.0 and r.max() > 10.0 and len(np.unique(rec["sphere"][on])) >= 20


def test_mask_shares():
    """Where rays that hit a hostile sphere sit beside ordinary ones: per lane
    mask, the share inside and outside it (case A's 44 x 26)."""
    for name in ("neg_r_4th", "scales", "dups", "giant_wall"):
        shares = sc.mask_shares(name)
        print(name, shares)
        for m, (inside, outside) in shares.items():
            assert inside > 0 and (outside > 0 or m == "wave"), (name, m)   # `wave` leaves 17 rays outside
    assert 0.02 < sc.mask_shares("neg_r_4th")["quad"][0] < 0.5   # a mixed scene: hostile hits beside ordinary ones


@pytest.mark.parametrize("name", sc.NEVER_HIT + ("tiny_r",))
def test_zero_tiny_nan_and_inf_spheres_are_never_hit(name):
    """c = oc.oc - r r with r = 0 is a point (disc > 0 fails but for rounding:
    none here), a NaN makes disc NaN, an infinite r makes c = -inf, disc = +inf
    and t = -inf."""
    s = sc.scene(name)[0]
    for rs in sc.ray_sets(name):
        for use_bvh in (True, False):
            rec = sc.hits(name, *rs, use_bvh)
            on = sc.on_hostile(name, *rs, use_bvh)
            if name == "tiny_r":   # ordinary down to k of about 70, never once r * r == 0
                r = s["radius"][rec["sphere"][on]]
                assert (r * r > 0).all(), name
                continue
            assert not on.any(), (name, rs, use_bvh)
            assert _hit(rec).sum() >= 1


def test_dense_non_finite_and_overflowing_scenes_collapse_to_a_chain():
    """Box areas of inf or NaN leave the SAH's fallback split (everything on
    one side) at every level: 40 inner levels, each with one empty leaf, and
    two leaves that hold spheres, of which hit.c tests the first only."""
    for name in CHAINS + ("inf_r_sparse",):
        nodes = sc.scene(name)[2]
        live = (nodes["sphere"] >= 0) & ((nodes["skip"] & cases.abi.NODE_EMPTY) == 0)
        print(name, len(nodes), "nodes, depth", sc.tree_depth(nodes), "leaves with spheres", int(live.sum()))
        assert len(nodes) == 159 and sc.tree_depth(nodes) == 40 and live.sum() == 2, name
        c = sc.counts(name)
        assert c["hits"] <= 20 and c["brute_hits"] >= 800 and c["tree_vs_brute_records"] >= 800, (name, c)
    for name in ("inf_c_sparse", "huge_r_sparse", "far_c_sparse", "nan_r_sparse", "nan_c_sparse"):   # stay rich
        assert len(sc.scene(name)[2]) >= 1000 and sc.counts(name)["hits"] >= 400, name


def test_tree_and_brute_force_differ():
    rows = {name: sc.counts(name)["tree_vs_brute_records"] for name in sc.SCENES}
    print("records tree != brute force (A, 44 x 26):", rows)
    assert rows["neg_r_4th"] >= 100 and rows["neg_r_all"] >= 800 and rows["giant_dome_50000"] >= 100
    assert rows["tiny_r"] == 0 and rows["far_c_sparse"] == 0 and rows["dust_radii"] == 0


def test_counts_and_nan_elements():
    """The oracle's records hold no NaN on any scene: a NaN or infinite sphere
    is never hit, and every hit has a finite t, point and normal."""
    total = {}
    for name in sc.SCENES:
        for rs in sc.ray_sets(name):
            if rs[1:] == sc.SIZES[0]:
                print(name, rs[0], sc.counts(name, *rs))
            for use_bvh in (True, False):
                rec = sc.hits(name, *rs, use_bvh)
                total[name, rs, use_bvh] = sc.nan_elements(rec)
                assert np.isfinite(rec["t"]).all() and (rec["t"][_hit(rec)] > 0).all()
    print("oracle NaN elements:", {k: v for k, v in total.items() if v} or "none on any scene")
    assert not any(total.values())

"""The cases of tests/overlay_cases.py are not vacuous (the oracle alone, no
GPU): the cases that should draw light pixels, the ones that should not give
the cleared canvas exactly, world_to_screen's corner classes occur (a float32
restatement in numpy), and hand_chain300's images differ between the level
values on both sides of the one-byte depth's clamp. Every threshold is what
the oracle gave when this file was written, asserted as a floor
(MEASUREMENTS.md records them)."""
import numpy as np
import pytest

import overlay_cases as oc

BIG = (160, 90)
# lit pixels of r1000 at 160 x 90, every level, by camera
LIT = {"default": 14384, "inside": 13378, "face": 14394, "skew": 14398, "fov1": 58, "fov170": 92, "fov180": 8,
       "fov-45": 14376, "pos_1e30": 5, "fwd_1e20": 5}
INSIDE_BY_SIZE = {(1, 1): 1, (1, 7): 7, (7, 1): 7, (5, 3): 15, (257, 3): 749, (3, 257): 257, (130, 9): 1170,
                  (64, 64): 3915}
DEFAULT_BY_LEVEL = {1: 948, 2: 1986, 5: 9440, 20: 14384}


def dark(case):
    """The cases of oc.CASES that draw nothing, by rule."""
    name, cam, size, levels = case
    return (name in ("r0", "no_tree", "inf_c_4th") or cam in oc.DARK or levels == 0
            or (cam == "inside" and name in ("r2", "r1", "coincident"))
            or (cam == "face" and name in ("coincident", "nan_boxes")))


def test_the_scenes_are_what_their_names_say():
    abi = oc.abi
    want = {"r1000": (2181, 40), "r2": (3, 1), "r1": (1, 0), "r0": (1, 0), "no_tree": (0, None), "coincident": (81, 40),
            "cluster": (9595, 40), "hand_falling": (3, 1), "hand_chain70": (141, 70), "hand_chain300": (601, 300),
            "hand_sticks_out": (3, 1), "nan_c_16th": (2115, 40), "inf_c_4th": (159, 40), "nan_boxes": (2181, 40)}
    assert set(want) == set(oc.SCENES)
    for name, (nn, depth) in want.items():
        nodes = oc.scene(name)[2]
        assert len(nodes) == nn, name
        if nn:
            assert int(oc.depths(nodes).max()) == depth, name
    boxes = lambda n: np.concatenate([oc.scene(n)[2]["bmin"], oc.scene(n)[2]["bmax"]], 1)
    assert int(np.isinf(boxes("nan_c_16th")).any(1).sum()) == 181
    assert np.isinf(boxes("inf_c_4th")).any(1).all()
    assert int(np.isnan(boxes("nan_boxes")).any(1).sum()) >= 600
    # coincident: chains of empty leaves with the inverted box (+inf, -inf)
    n = oc.scene("coincident")[2]
    empty = (n["skip"] & abi.NODE_EMPTY) != 0
    assert empty.sum() == 40 and (n["bmin"][empty] == np.inf).all() and (n["bmax"][empty] == -np.inf).all()
    # past the one-byte depth: 90 nodes of hand_chain300 lie deeper than 255, none of hand_chain70
    d = oc.depths(oc.scene("hand_chain300")[2])
    assert int((d > 255).sum()) == 90 and int((d >= 255).sum()) == 92
    # a flat tree through tree_from_flat flattens to itself
    o = oc.cases._oracle()
    for name in oc.HAND + ("nan_boxes",):
        _, tree, nodes = oc.scene(name)
        assert o.flatten(tree).tobytes() == nodes.tobytes(), name


def test_every_case_draws_or_gives_the_cleared_canvas():
    assert len(oc.CASES) >= 120
    for scene in oc.SCENES:
        assert oc.cases_of(scene), scene
    for case in oc.CASES:
        img = oc.expected(*case)
        assert img.shape == (case[2][1], case[2][0], 4)
        if dark(case):
            assert (img == oc.CLEAR).all(), case
        else:
            assert oc.lit(img) > 0, case
            assert (img[(img != oc.CLEAR).any(-1)][:, 3] == 180).all(), case


def test_the_cameras_on_the_built_scene():
    assert set(LIT) | set(oc.DARK) == set(oc.CAMERAS)
    for cam, floor in LIT.items():
        assert oc.lit(oc.expected("r1000", cam, BIG, -1)) >= floor, cam
    for cam in oc.DARK:
        assert (oc.expected("r1000", cam, BIG, -1) == oc.CLEAR).all(), cam
    # heavy overdraw: the last-line-wins rule decides nearly every pixel of the default view
    img = oc.expected("r1000", "default", BIG, -1)
    # (the depth colours have period 5: 40 d mod 200)
    assert len({tuple(int(v) for v in c) for c in img.reshape(-1, 4)}) == 6
    shallow = oc.expected("r1000", "default", BIG, 5)
    both = (img != oc.CLEAR).any(-1) & (shallow != oc.CLEAR).any(-1)
    assert int((img[both] != shallow[both]).any(-1).sum()) >= 5000   # pixels a deeper node's line took over


def test_the_sizes_and_levels():
    for size, floor in INSIDE_BY_SIZE.items():
        assert oc.lit(oc.expected("r1000", "inside", size, -1)) >= floor, size
    for size in oc.SIZES:
        assert oc.lit(oc.expected("r1000", "default", size, -1)) > 0, size
    assert (oc.expected("r1000", "default", BIG, 0) == oc.CLEAR).all()
    for lv, floor in DEFAULT_BY_LEVEL.items():
        assert oc.lit(oc.expected("r1000", "default", BIG, lv)) >= floor, lv
    # one level alone is the root box in the root's colour
    img = oc.expected("r1000", "default", BIG, 1)
    assert (img[(img != oc.CLEAR).any(-1)] == np.array(oc.depth_colour(0), np.uint8)).all()
    # from inside, the first levels light nothing (their corners are behind the camera or out of range)
    o = oc.cases._oracle()
    tree = oc.scene("r1000")[1]
    for lv in (0, 1, 2):
        assert (oc.overlay_of(tree, oc.camera("inside"), BIG, lv) == oc.CLEAR).all(), lv
    # r1000's deepest nodes have depth 40: 41 and every negative or huge value draw every node, 40 does not
    full = oc.expected("r1000", "default", BIG, -1)
    for lv in (41, oc.INT_MAX, -2, oc.INT_MIN):
        assert (oc.expected("r1000", "default", BIG, lv) == full).all(), lv
    # (21 happens to equal the full image: the colours have period 5, and a chain of coincident spheres
    # draws the same box at every depth from 16 to 40; 20, 22 and 40 differ from it in 212 pixels)
    for lv, floor in ((5, 11968), (20, 212), (22, 212), (40, 212)):
        assert int((oc.expected("r1000", "default", BIG, lv) != full).any(-1).sum()) >= floor, lv


@pytest.mark.parametrize("cam,floors", [
    ("default", dict(behind=0, outside=0, nan_z=752, minus_one=46, toward_zero=34, int_min=752)),
    ("inside", dict(behind=5912, outside=9032, nan_z=752, minus_one=1, toward_zero=12, int_min=752))])
def test_world_to_screen_corner_classes(cam, floors):
    """Of r1000's 17448 corners at 160 x 90: behind z <= 0.1; outside [-W, 2W]
    x [-H, 2H]; a NaN z (an infinite box coordinate times a zero basis
    component), which passes both float tests and converts to INT_MIN; x
    truncating to -1, the `x == -1` sentinel that drops a visible corner's
    edges; a negative x truncating toward zero to 0."""
    p = oc.project(oc.camera(cam), oc.corners(oc.scene("r1000")[2]), *BIG)
    ok = p["ok"]
    got = dict(behind=int(p["behind"].sum()), outside=int(p["outside"].sum()), nan_z=int(p["nan_z"].sum()),
               minus_one=int((ok & (p["ix"] == -1)).sum()), toward_zero=int((ok & (p["sx"] < 0) & (p["ix"] == 0)).sum()),
               int_min=int((ok & (p["ix"] == oc.INT_MIN)).sum()))
    assert ok.size == 17448
    for k, floor in floors.items():
        assert got[k] >= floor, (k, got)


def test_the_restated_projection_is_the_oracles():
    """The root box alone (max_levels 1): every corner the restatement keeps on screen is lit."""
    for name, cam in (("r1000", "default"), ("r2", "default"), ("hand_chain300", "chain")):
        nodes = oc.scene(name)[2]
        img = oc.expected(name, cam, BIG, 1) if (name, cam, BIG, 1) in oc.CASES else \
            oc.overlay_of(oc.scene(name)[1], oc.camera(cam, name), BIG, 1)
        p = oc.project(oc.camera(cam, name), oc.corners(nodes[:1]), *BIG)
        seen = 0
        for k in range(8):
            x, y = int(p["ix"][0, k]), int(p["iy"][0, k])
            if p["ok"][0, k] and 0 <= x < BIG[0] and 0 <= y < BIG[1]:
                seen += 1
                assert (img[y, x] != oc.CLEAR).any(), (name, k)
        assert seen >= 2, name


def test_hand_chain300_across_the_clamp():
    """The camera at (60, 0, 120), fov 60, looking down -z at 160 x 90."""
    img = {lv: oc.expected("hand_chain300", "chain", BIG, lv) for lv in oc.CHAIN_LEVELS}
    diff = lambda a, b: (img[a] != img[b]).any(-1)
    assert oc.lit(img[-1]) >= 482
    # what a depth clamped to 255 cannot show: leaving out the nodes deeper than 255 changes 280 pixels ...
    changed = diff(256, -1)
    assert int(changed.sum()) >= 280
    # ... none of which has depth 255's colour, which the clamp would give them
    assert not (img[-1][changed] == np.array(oc.depth_colour(255), np.uint8)).all(-1).any()
    assert int(diff(254, 255).sum()) >= 372 and int(diff(255, 256).sum()) >= 364
    assert int(diff(256, 257).sum()) >= 356
    assert int(diff(300, 301).sum()) >= 12
    assert not diff(301, -1).any()
    # the chain of 70 stays below the clamp: its levels are the byte's own
    a, b, c = (oc.expected("hand_chain70", "chain", BIG, lv) for lv in (69, 70, 71))
    assert (a != b).any() and (b != c).any() and (c == oc.expected("hand_chain70", "chain", BIG, -1)).all()


# ---------------------------------------------------------------- mirt_camera_rays_uv

def test_the_uv_restatement_is_the_oracles_on_the_pixel_grid(small):
    o = oc.cases._oracle()
    for name, cam in oc.uv_cameras(small).items():
        for w, h in oc.UV_SIZES[1:]:
            want = o.camera_rays(cam, w, h)
            got = oc.uv_rays(cam, w, h, oc.pixel_uv(w, h))
            assert got.tobytes() == want.tobytes(), (name, w, h)


def test_the_hostile_uv_reach_the_edges(small):
    uv = oc.hostile_uv()
    assert len(uv) >= 500 and np.isnan(uv).any() and np.isinf(uv).any()
    d = oc.uv_rays(oc.uv_cameras(small)["default"], 160, 90, uv)["direction"]
    nan = np.isnan(d).any(1)
    zero = (d == 0).all(1)
    finite = np.isfinite(d).all(1) & ~zero
    # a NaN or infinite sum gives NaN (inf / inf), a sum whose square overflows a zero vector (x / inf)
    assert nan.sum() >= 50 and zero.sum() >= 20 and finite.sum() >= 200
    n = np.sqrt((d[finite].astype(np.float64) ** 2).sum(1))
    assert np.abs(n - 1).max() < 1e-6

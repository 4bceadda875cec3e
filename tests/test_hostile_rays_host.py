"""The hostile ray sets (tests/hostile_ray_cases.py) are not vacuous: from the
oracle alone (no GPU), what hit.c and renderer.c do with them. The counts are
the reference's, never the product's; MEASUREMENTS.md records them."""
import numpy as np
import pytest

import hostile_ray_cases as hc
import test_planes_cases as cases

W, H = hc.W, hc.H


def _hit(records):
    return records["hit"] != 0


def _same_records(a, b):
    return (np.ascontiguousarray(a).view(np.uint8).reshape(a.size, -1) ==
            np.ascontiguousarray(b).view(np.uint8).reshape(b.size, -1)).all(-1).reshape(a.shape)


def test_the_sets_are_what_the_docstring_says():
    base = hc.base()
    for name in ("nf_origin", "nf_dir"):
        field = name.split("_")[1].replace("dir", "direction")
        other = "direction" if field == "origin" else "origin"
        v = hc.rays(name)[field]
        n = (~np.isfinite(v)).sum(-1)
        assert (n >= 1).all() and (n >= 2).mean() >= 0.24 and (n == 3).sum() >= 50, name
        for value in (np.inf, -np.inf):
            assert (v == value).any(axis=(0, 1)).all(), (name, value)    # in every component
        assert np.isnan(v).any(axis=(0, 1)).all(), name
        assert hc.rays(name)[other].tobytes() == base[other].tobytes()
    z = hc.rays("zero_dir")["direction"]
    assert (z == 0).all() and len(np.unique(np.signbit(z).reshape(-1, 3), axis=0)) == 8
    for name, sign in (("tiny", -1), ("tiny_inf", -1), ("huge", 1)):
        k = hc.exponents(name).astype(np.float64)
        want = (base["direction"].astype(np.float64) * (2.0 ** (sign * k))[..., None]).astype(np.float32)
        assert hc.rays(name)["direction"].tobytes() == want.tobytes() and np.isfinite(want).all(), name
    assert hc.exponents("tiny").min() == 60 and hc.exponents("tiny").max() == 95
    assert hc.exponents("tiny_inf").min() == 74 and hc.exponents("tiny_inf").max() == 81
    assert hc.exponents("huge").min() == 55 and hc.exponents("huge").max() == 127
    o = hc.rays("far_origin")["origin"]
    i = np.arange(W * H).reshape(H, W)
    assert (np.abs(o[i % 3 == 0]).max(-1) == np.float32(3.0e38)).all() and np.isfinite(o).all()
    assert (o[i % 3 == 0] == np.float32(-3.0e38)).any() and (o[i % 3 == 0] == np.float32(3.0e38)).any()
    assert (o[i % 3 == 2] == base["origin"][i % 3 == 2] * np.float32(2.0 ** 40)).all()
    assert np.abs(o[i % 3 == 1]).max() > 1e31
    for m in hc.MASKS:
        share = hc.mask(m).mean()
        assert 0.2 <= share <= 0.99, (m, share)
    assert hc.mask("wave").reshape(-1)[63::64].sum() == 0 and hc.mask("wave").sum() == W * H - (W * H) // 64
    assert not hc.mask("tiles")[:8, :8].any() and hc.mask("tiles")[:8, 8:16].all()
    for name in hc.FAMILIES:
        assert hc.rays(name).shape == (H, W) and not hc.rays(name).flags.writeable


@pytest.mark.parametrize("name", hc.ALL_MISS + ("huge",))
def test_non_finite_zero_far_and_huge_rays_miss_and_still_colour_the_sky(name):
    c = hc.counts(name)
    print(name, c)
    for use_bvh in (True, False):
        h = hc.hits(name, use_bvh)
        sel = hc.exponents("huge") >= 64 if name == "huge" else np.ones((H, W), bool)
        assert not _hit(h)[sel].any(), (name, use_bvh)
        for depth in hc.DEPTHS:   # a miss is the sky at every depth
            assert hc.colours(name, depth, use_bvh)[sel].tobytes() == hc.colours(name, 1, use_bvh)[sel].tobytes()
    assert hc.colours(name).tobytes() == hc.colours(name, use_bvh=False).tobytes()
    if name in ("nf_origin", "nf_dir", "far_origin"):   # the direction's y varies (nf_dir: also NaN through the cast)
        assert c["colours"] >= 50, c
    else:   # zero_dir: dy = +-0; huge: the gradient beyond int's range (trace.h int_x86)
        assert 1 <= c["colours"] <= 2, c


def test_tiny_inf_records_infinite_t_with_nan_normals():
    c = hc.counts("tiny_inf")
    print("tiny_inf", c)
    h, b = hc.hits("tiny_inf"), hc.hits("tiny_inf", False)
    inf_t = _hit(h) & np.isposinf(h["t"])
    assert inf_t.sum() >= 200
    assert np.isnan(h["normal"][inf_t]).any(-1).all() and not np.isfinite(h["point"][inf_t]).all(-1).any()
    # x86's default NaN, the one pattern the reference produces here
    nan_bits = np.unique(h["normal"].view(np.uint32)[np.isnan(h["normal"])])
    print("oracle NaN patterns:", [hex(v) for v in nan_bits])
    assert list(nan_bits) == [0xffc00000]
    assert (_hit(h) & np.isfinite(h["t"])).sum() >= 50          # hits with finite t beside them
    assert not np.isposinf(b["t"]).any() and hc.nan_elements(b) == 0   # brute force (strict <) records none
    assert (hc.colours("tiny_inf") != hc.colours("tiny_inf", use_bvh=False)).any(-1).sum() >= 100
    assert len(np.unique(h["sphere"][inf_t])) >= 2               # inf-t hits on different spheres
    # a later leaf with t = +inf replaces an earlier one (hit.c's t <= best): some inf-t ray has an inf-t hit on
    # another sphere than the recorded one too
    spheres, _, _ = cases.scene(hc.N)
    r = hc.rays("tiny_inf")[inf_t][:64]
    ties = 0
    for ray, rec in zip(r, h["sphere"][inf_t][:64]):
        pairs = cases._oracle().sphere_pairs(np.repeat(ray[None], len(spheres)), spheres)
        ties += int(((pairs["hit"] != 0) & np.isposinf(pairs["t"]) & (np.arange(len(spheres)) != rec)).any())
    print("tiny_inf: of 64 inf-t rays,", ties, "have an inf-t hit on a second sphere")
    assert ties >= 1


def test_tiny_straddles_the_three_regimes():
    k, h = hc.exponents("tiny"), hc.hits("tiny")
    rows = {}
    for lo, hi in ((60, 69), (70, 73), (74, 81), (82, 95)):
        m = (k >= lo) & (k <= hi)
        rows[lo] = (int(m.sum()), int(_hit(h)[m].sum()), int(np.isposinf(h["t"][m]).sum()))
    print("tiny: k range -> (rays, hits, inf-t hits)", rows)
    assert rows[60][1] >= 100 and rows[60][2] == 0      # ordinary
    assert rows[74][2] >= 50 and rows[74][1] > rows[74][2]   # t = +inf beside finite t
    assert rows[82][0] >= 200 and rows[82][1] == 0      # everything misses
    print("tiny", hc.counts("tiny"))


@pytest.mark.parametrize("name", hc.MIXED)
def test_unsubstituted_pixels_of_a_mixed_set_equal_the_base_set(name):
    """The same pixel index, so the same RNG stream: a neighbour of a hostile
    ray has the hit record and the colours of the base set. This is what makes
    "neighbours undisturbed" checkable on the GPU."""
    keep = ~hc.substituted(name)
    src = "tiny_inf" if name.endswith("_tiny") else None
    assert keep.sum() >= 17 and (~keep).sum() >= 200
    assert hc.rays(name)[keep].tobytes() == hc.base()[keep].tobytes()
    for use_bvh in (True, False):
        assert _same_records(hc.hits(name, use_bvh), hc.hits("base", use_bvh))[keep].all()
        for depth in hc.DEPTHS:
            assert (hc.colours(name, depth, use_bvh)[keep] == hc.colours("base", depth, use_bvh)[keep]).all()
            if src:
                assert (hc.colours(name, depth, use_bvh)[~keep] == hc.colours(src, depth, use_bvh)[~keep]).all()
    c = hc.counts(name)
    print(name, c)
    assert _hit(hc.hits(name))[keep].any()
    if src:
        assert c["inf_t"] >= 100
    else:
        assert not _hit(hc.hits(name))[~keep].any()


def test_no_nan_outside_the_tiny_and_mixed_sets():
    total = {}
    for name in hc.FAMILIES:
        for use_bvh in (True, False):
            n = hc.nan_elements(hc.hits(name, use_bvh))
            total[name, use_bvh] = n
            if name not in hc.MAY_HOLD_NAN or not use_bvh:
                assert n == 0, (name, use_bvh, n)
    print("oracle NaN elements per (family, use_bvh):", {k: v for k, v in total.items() if v})
    for name in hc.LATTICE_SETS:
        assert hc.nan_elements(hc.lattice_hits(name, False)) == 0
    assert hc.nan_elements(hc.lattice_hits("lattice_nf_origin")) == 0


def test_the_lattice_sets():
    s, _, nodes = hc.lattice()
    import test_filtered_forms as ff
    assert ff.origin_bound(s, nodes)[0] == 0                       # no origin bound
    for name in hc.LATTICE_SETS:
        assert 1000 <= len(hc.lattice_rays(name)) <= 2000
    assert not _hit(hc.lattice_hits("lattice_nf_origin")).any()
    assert not _hit(hc.lattice_hits("lattice_nf_origin", False)).any()
    assert len(np.unique(hc.lattice_colours("lattice_nf_origin"), axis=0)) >= 50
    h = hc.lattice_hits("lattice_tiny_inf")
    inf_t = _hit(h) & np.isposinf(h["t"])
    print("lattice_tiny_inf:", len(h), "rays,", int(_hit(h).sum()), "hits,", int(inf_t.sum()), "with t = +inf,",
          hc.nan_elements(h), "NaN elements; brute force hits", int(_hit(hc.lattice_hits("lattice_tiny_inf", False)).sum()))
    assert inf_t.sum() >= 200 and (_hit(h) & np.isfinite(h["t"])).sum() >= 50
    # the recorded sphere is a duplicate, and its twin's own quadratic gives +inf too
    dup = hc.lattice_duplicates()
    assert len(dup) == 16
    on_dup = np.flatnonzero(inf_t & np.isin(h["sphere"], dup))
    assert len(on_dup) >= 4
    key = np.column_stack([s["center"], s["radius"]])
    for j in on_dup:
        twin = [d for d in dup if d != h["sphere"][j] and (key[d] == key[h["sphere"][j]]).all()]
        assert len(twin) == 1
        p = cases._oracle().sphere_pairs(hc.lattice_rays("lattice_tiny_inf")[j:j + 1], s[twin[0]:twin[0] + 1])
        assert p["hit"][0] == 1 and np.isposinf(p["t"][0])   # (which twin wins is hit.c's later-leaf rule)
    # the mixed set: its ordinary rays are the base set's, and some of them tie at FINITE t between duplicates
    m, base = hc.lattice_hits("lattice_mixed_quad_tiny"), hc.lattice_hits("lattice_base")
    keep = np.arange(len(m)) % 4 != 0
    assert m[keep].tobytes() == base[keep].tobytes() and m[~keep].tobytes() == h[~keep].tobytes()
    finite_tie = keep & _hit(m) & np.isfinite(m["t"]) & np.isin(m["sphere"], dup)
    print("lattice_mixed_quad_tiny:", int(finite_tie.sum()), "ordinary rays record a duplicate at finite t,",
          int((_hit(m) & np.isposinf(m["t"])).sum()), "hostile ones t = +inf")
    assert finite_tie.sum() >= 8 and (_hit(m) & np.isposinf(m["t"])).sum() >= 100
    # (the twins never tie here: the build keeps each pair in one leaf and hit.c tests a leaf's first sphere
    # only, so the duplicate's twin is in no leaf node -- hostile_ray_cases.twins() is the scene where they do)
    tested = set(int(v) for v in hc.lattice()[2]["sphere"])
    assert sum(1 for d in dup if int(d) in tested) == 8


def test_the_twins_tie_on_every_hit():
    """Every hit of the twins scene is an exact tie between sphere 2j and its
    duplicate 2j + 1: hit.c's tree walk records the later leaf (the odd index),
    brute force the first (the even one), at finite t and at t = +inf."""
    import importlib
    mirt = importlib.import_module("cs201_sah-bvh_ray_tracer_amd")
    s, _, nodes = hc.twins()
    mirt.validate_bvh(nodes, len(s))
    info, _ = mirt.scene_layout(s, mirt.Bvh(nodes))
    assert info["ordered"] and info["encloses"] and info["o_bound"] > 0
    assert (s[0::2]["center"] == s[1::2]["center"]).all() and (s[0::2]["radius"] == s[1::2]["radius"]).all()
    h, b = hc.twins_hits(), hc.twins_hits(False)
    finite, inf_t = _hit(h) & np.isfinite(h["t"]), _hit(h) & np.isposinf(h["t"])
    generic = ~(np.abs(hc.twins_rays()["direction"]) >= 2.0 ** -40).all(-1)
    print("twins:", int(finite.sum()), "finite ties,", int(inf_t.sum()), "ties at t = +inf,", int((~_hit(h)).sum()),
          "misses; brute force hits", int(_hit(b).sum()))
    assert finite.sum() >= 500 and inf_t.sum() >= 100 and (~_hit(h)).sum() >= 20
    assert (h["sphere"][_hit(h)] % 2 == 1).all() and (b["sphere"][_hit(b)] % 2 == 0).all()
    assert (finite & ~generic).sum() >= 500 and generic[inf_t].all()   # the finite ties reach cand_better
    plain = finite & ~generic
    assert (b["sphere"][plain] == h["sphere"][plain] - 1).all() and not _hit(b)[inf_t].any()
    assert len(np.unique(hc.twins_colours(5), axis=0)) >= 50


def test_hostile_cameras_render_and_cover_hits_and_misses():
    rows = {}
    for name in hc.CAMERAS:
        for w, h in hc.CAMERA_SIZES:
            frame = hc.camera_frame(name, w, h)
            rows[name, w] = (len(np.unique(frame.reshape(-1, 4), axis=0)),
                             int((hc.camera_planes(name, w, h)["sphere"] >= 0).sum()))
            assert frame.shape == (h, w, 4) and (frame[..., 3] == 255).all()
    print("cameras: (name, width) -> (colours, primary hits)", rows)
    for name in ("nan_x", "nan_y", "nan_z", "inf_z", "1e30_x", "3e38_y"):
        assert rows[name, 44] == (rows[name, 44][0], 0) and rows[name, 44][0] >= 50, name
    assert rows["fov_nan", 44] == (1, 0)
    assert rows["fov_0", 44][1] == 44 * 26                 # every ray is `forward`
    for name in ("forward_y0", "forward_x0"):
        cam = hc.camera(name)
        f = np.array([cam.forward.x, cam.forward.y, cam.forward.z])
        assert (f == 0).sum() == 1, (name, f)
        assert rows[name, 44][1] >= 100, name

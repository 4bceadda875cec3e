"""Every walk on non-finite rays and on rays at the float range's ends
(tests/hostile_ray_cases.py), against the CPU oracle: mirt_intersect_rays,
mirt_any_hit_rays, mirt_trace_rays, ray frames on every schedule, hostile
cameras through the packet kernel, the primary cache and the reprojected loop.

The comparison rule. hit, sphere, t and colours byte for byte. point and normal
byte for byte wherever the oracle's float is not a NaN; where it is, the
product's must be a NaN too (sign and payload are not compared: x86 produces
0xffc00000 for inf / inf; the tests print the device's patterns, and gfx950's
correctly rounded division gave 0xffc00000 as well when this was written).
The elements compared that way are exactly the oracle's NaN elements; every test
prints and asserts their number, and tests/test_hostile_rays_host.py shows there
are none outside the tiny* and mixed_* sets. The product's own identities (a ray
frame against mirt_trace_rays, the planes against mirt_intersect_rays, a cached
frame against the walked one, the reprojected loop against mirt_reproject_host)
stay byte for byte without exception.

Why every loop these rays enter terminates (read in csrc/trace.h and
csrc/render.hip; a NaN or an infinity only ever changes the outcome of a
comparison, never how far a loop index moves):

  closest_bvh / lane_step (the flat DFS, and the DFS segments of the four-wide
    walks): `next` becomes next + 1 or the node's skip link, both greater than
    next by the tree's construction, whatever the box and sphere tests say; the
    walk ends at num_nodes.
  closest_bvh_chunked (rays with a zero or tiny direction component, so every
    tiny* ray and every NaN direction): `cur` moves to base + stop or to a skip
    link of a node at or behind cur; both exceed cur. The replay of the chunk's
    masks is scalar integer code.
  wide_lane_step / wide_walk_step: a step pops the LDS stack, or replaces the
    node by its children (n - 1 pushes, bounded by kWideStack, else the subtree
    is walked as a DFS segment). Each node is entered at most once per walk
    because a slot's test has one boolean outcome; the sort keys pass through
    fminf(e, 3.0e38f), which maps a NaN or infinite entry to a finite key, so
    the n passing slots still sort before the failing ones (+inf keys) and only
    references of passing inner slots are pushed. The per-step gate loop clears
    one bit of a four-bit mask per iteration.
  quad_step / solo_step: the same walk with the slots in four lanes; rank is a
    count of comparisons (a NaN key cannot occur behind the fminf), n comes from
    a ballot of `inner`, pushes are bounded by CAP or fall back to a segment.
  closest_packet_ordered: a step descends, takes a child, or pops one of at most
    tree-depth + 1 stack entries; masks only lose lanes on the way down.
  the bounce kernel's queue loop: the refill loop ends when a segment yields
    (b < sz) or all kQSeg segments are dry; a chain ends at a miss or at depth
    (level only grows); a deferred walk whose confirmation fails walks its level
    once more with kExactWalk set, which cannot fail again. A non-finite origin
    misses every sphere (disc is NaN), so such a chain ends at once.
  hemisphere / hemisphere_wave: the rejection loop reads only the RNG stream,
    never the normal (a NaN normal only decides the final flip), and is capped
    at 4096 tries / rounds.
"""

import numpy as np
import pytest

import hostile_ray_cases as hc
import reproject_cases as rpc
import test_planes_cases as cases
from test_planes_gpu import schedules, upload
from test_ray_frames_gpu import SCHEDULES

pytestmark = pytest.mark.gpu

W, H, N = hc.W, hc.H, hc.N
PLANES = ("t", "sphere", "normal")


def _defaults(abi):
    return {abi.OPT_TRAVERSAL: abi.TRAV_WAVEFRONT, abi.OPT_FAST_SLAB: 1, abi.OPT_DEFER: 1, abi.OPT_PRUNE: 1,
            abi.OPT_ORDERED: 1, abi.OPT_QUAD_BATCH: 1, abi.OPT_LEAF_BATCH: 2, abi.OPT_CONFIRM_ONCE: 2,
            abi.OPT_PRIMARY_CACHE: 0}


class options:
    """Options set for one block; the library defaults afterwards (LEAF_BATCH and CONFIRM_ONCE read back the
    value in effect, not the stored one, so they cannot be restored from mirt_get_option)."""

    def __init__(self, r, abi, opts):
        self.r, self.abi, self.opts = r, abi, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.r.set_option(k, v)

    def __exit__(self, *a):
        d = _defaults(self.abi)
        for k in self.opts:
            self.r.set_option(k, d[k])


def walks(abi):
    return [("quad batch", {}), ("per-lane four-wide", {abi.OPT_QUAD_BATCH: 0}),
            ("DFS", {abi.OPT_ORDERED: 0, abi.OPT_PRUNE: 0}), ("exact slab", {abi.OPT_FAST_SLAB: 0}),
            ("prune off", {abi.OPT_PRUNE: 0}), ("leaf batch on", {abi.OPT_LEAF_BATCH: 1}),
            ("confirm once on", {abi.OPT_CONFIRM_ONCE: 1}), ("confirm once off", {abi.OPT_CONFIRM_ONCE: 0})]


DEVICE_NAN = set()   # the NaN bit patterns the device produced, printed by the tests that meet one


def nan_for_nan(got, want, what):
    """Float arrays, byte for byte except that the oracle's NaN elements need only be NaN; returns their number."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.size} elements differ, first at "
                            f"{np.argwhere(diff)[0]}: {got[diff][0]!r} != {want[diff][0]!r}")
    bad = nan & ~np.isnan(got)
    assert not bad.any(), f"{what}: {int(bad.sum())} of the oracle's {int(nan.sum())} NaN elements are no NaN: {got[bad][0]!r}"
    DEVICE_NAN.update(hex(v) for v in np.unique(got.view(np.uint32)[nan]))
    return int(nan.sum())


def same_records(got, want, what, rays=None):
    """abi.HIT records against the oracle's under the rule above; returns the number of NaN-for-NaN elements."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    for k in ("hit", "sphere", "pad"):
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, (f"{what}: {k} differs on {len(bad)} of {len(got)} rays, first ray {bad[0]}"
                               f"{'' if rays is None else ' ' + str(np.asarray(rays).reshape(-1)[bad[0]])}: "
                               f"{got[bad[0]]} != {want[bad[0]]}")
    bad = np.flatnonzero(got["t"].view(np.uint32) != want["t"].view(np.uint32))
    assert len(bad) == 0, f"{what}: t differs on {len(bad)} rays, first ray {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    return nan_for_nan(got["point"], want["point"], what + " point") + nan_for_nan(got["normal"], want["normal"],
                                                                                     what + " normal")


def same_planes(got, want, what):
    for k in ("t", "sphere"):
        diff = np.asarray(got[k]).view(np.uint32) != np.asarray(want[k]).view(np.uint32)
        assert not diff.any(), f"{what}: plane {k}: {int(diff.sum())} of {diff.size} differ"
    return nan_for_nan(got["normal"], want["normal"], what + " plane normal")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = (got != want).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}"


def same_bytes(got, want, what):
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), what


def plane_nans(records):
    return int(np.isnan(records["normal"]).sum())


def upload_lattice(gpu, mirt):
    s, _, nodes = hc.lattice()
    gpu.upload(s, mirt.Bvh(nodes))
    info, _ = gpu.resident_layout()
    assert info["o_bound"] == 0


def check_per_ray(gpu, mirt, rays, tree_hits, brute_hits, what):
    """closest_hit on every walk and any_hit, tree and brute force; returns nothing, prints the NaN counts."""
    abi = mirt.abi
    flat = np.ascontiguousarray(rays).reshape(-1)
    want, brute = np.asarray(tree_hits).reshape(-1), np.asarray(brute_hits).reshape(-1)
    counted = []
    for name, opts in walks(abi):
        with options(gpu, abi, opts):
            counted.append(same_records(gpu.closest_hit(flat), want, f"{what}, {name}", flat))
            flags = gpu.any_hit(flat, use_bvh=True)
            bad = np.flatnonzero(flags != want["hit"])
            assert len(bad) == 0, f"{what}, {name}: any_hit differs on {len(bad)} rays, first {flat[bad[0]]}"
    n_brute = same_records(gpu.closest_hit(flat, use_bvh=False), brute, what + ", brute force", flat)
    assert (gpu.any_hit(flat, use_bvh=False) == brute["hit"]).all(), what
    print(f"  {what}: NaN-for-NaN elements per walk {counted} (oracle {hc.nan_elements(want)}), brute force {n_brute}; "
          f"device NaN patterns so far {sorted(DEVICE_NAN)}")
    assert set(counted) == {hc.nan_elements(want)} and n_brute == hc.nan_elements(brute) == 0


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_closest_hit_and_any_hit_on_every_walk(gpu, mirt, name):
    upload(gpu, mirt, N)
    check_per_ray(gpu, mirt, hc.rays(name), hc.hits(name), hc.hits(name, False), name)
    if name in hc.MIXED:   # neighbours undisturbed: stated once more against the base set's own records
        keep = ~hc.substituted(name).reshape(-1)
        got = gpu.closest_hit(np.ascontiguousarray(hc.rays(name)).reshape(-1))
        same_bytes(got[keep], hc.hits("base").reshape(-1)[keep], name + ": the unsubstituted rays")


# Found by this file on its first run: every hit the reference records with t = +inf was a miss on the device, on
# every walk and in every frame (153 of `tiny`'s 1144 rays, 773 of tiny_inf's, 840 of the lattice's 1750). A ray
# with a direction component below 2^-40 takes closest_bvh_chunked, which accepted a chunk's winner only for
# tmin < INFINITY; and the packet walk (trace_ray's level 0) and the chunked walk hold a ray with an exactly zero
# component to boxes around its own coordinate from the start (pruned_any), a geometric rule that hit.c's
# arithmetic does not obey once d.d underflows: with a == 0 every sphere whose leaf box passes "hits" at +inf.
# Such rays (4 d.d below the normal range) now take the chunked walk and walk it unpruned.
# (origin, direction) against test_planes_cases.scene(1000), float32 as printed: |d| about 2^-77, an ordinary
# one, two of the centre column (d.x == 0), and one at 2^-75.
REGRESSION_INFINITE_T = [
    ((0.0, 4.0, 50.0), (-4.5489597e-24, 1.8391726e-24, -4.4401553e-24)),
    ((0.0, 4.0, 50.0), (0.0, 2.5323865e-24, -6.1137217e-24)),
    ((0.0, 4.0, 50.0), (0.0, 1.2556097e-25, -3.9407026e-25)),
    ((0.0, 4.0, 50.0), (-1.7106556e-23, 7.729968e-24, -1.8661794e-23)),
]


def test_regression_infinite_t(gpu, mirt):
    """The named rays above on every walk, in trace_ray and as a (4 x 1) ray
    frame on every schedule: hit.c's record, t = +inf and a NaN normal."""
    abi, o = mirt.abi, cases._oracle()
    spheres = upload(gpu, mirt, N)
    _, tree, _ = cases.scene(N)
    rays = np.zeros(len(REGRESSION_INFINITE_T), abi.RAY)
    rays["origin"] = [p[0] for p in REGRESSION_INFINITE_T]
    rays["direction"] = [p[1] for p in REGRESSION_INFINITE_T]
    want = o.intersect(tree, spheres, rays)
    assert (want["hit"] == 1).all() and np.isposinf(want["t"]).all() and np.isnan(want["normal"]).all()
    assert len(set(want["sphere"])) >= 3
    brute = o.intersect(tree, spheres, rays, use_bvh=False)
    assert not brute["hit"].any()   # renderer.c's strict `<` never records t = +inf
    check_per_ray(gpu, mirt, rays, want, brute, "REGRESSION_INFINITE_T")
    n = len(rays)
    for schedule in SCHEDULES:
        depth, use_bvh, opts = schedules(abi)[schedule]
        col = o.trace_rays(rays, spheres, tree, depth=depth, use_bvh=use_bvh)
        with options(gpu, abi, opts):
            same(gpu.trace_ray(rays, depth=depth, use_bvh=use_bvh), col, f"trace_ray under {schedule}")
            rgba, got = gpu.render_rays(rays.reshape(1, n), n, 1, planes=PLANES, depth=depth, use_bvh=use_bvh)
            same(rgba, col.reshape(1, n, 4), f"a ray frame on {schedule}")
            same_planes(got, cases.planes_of(want if use_bvh else brute, (1, n)), f"a ray frame on {schedule}")


@pytest.mark.parametrize("name", hc.LATTICE_SETS)
def test_the_lattice_without_an_origin_bound(gpu, mirt, name):
    """fp16-exact boxes, touching spheres, o_bound == 0; also trace_ray at depths 1 and 5."""
    abi = mirt.abi
    upload_lattice(gpu, mirt)
    rays = hc.lattice_rays(name)
    check_per_ray(gpu, mirt, rays, hc.lattice_hits(name), hc.lattice_hits(name, False), name)
    for what, opts, use_bvh in (("default", {}, True), ("DFS", {abi.OPT_ORDERED: 0, abi.OPT_PRUNE: 0}, True),
                                ("brute force", {}, False)):
        with options(gpu, abi, opts):
            for depth in (1, 5):
                same(gpu.trace_ray(rays, depth=depth, use_bvh=use_bvh), hc.lattice_colours(name, depth, use_bvh),
                     f"{name} trace_ray {what} depth {depth}")


def test_a_nan_origin_component_takes_the_exact_test_without_a_bound(gpu, mirt, oracle):
    """fmaxf drops a NaN: an origin (NaN, +-0, +-0) has max|o| = 0 for the
    bounce walk's and the camera pass's "origin within the bound" check. On a
    scene without an origin bound (o_bound == 0, boxes never grown) such a lane
    must still be `generic`, so the margin-free forms EQUAL hit.c's flag on
    every pair, as test_filtered_forms' zero-origin test shows for plain zeros.
    hit.c's own fminf / fmaxf drop the NaN axis, so both outcomes occur."""
    import test_filtered_forms as ff
    abi = mirt.abi
    s, b = ff._unbounded_scene(mirt)
    gpu.upload(s, b)
    info, _ = gpu.resident_layout()
    assert info["o_bound"] == 0
    rays, boxes = ff.zero_origin_pairs(np.random.default_rng(6), 48_000)
    i = np.arange(len(rays))
    rays["origin"][i, i % 3] = np.nan
    two = i % 4 == 3   # and a quarter with two NaN components
    rays["origin"][i[two], (i[two] + 1) % 3] = np.nan
    ref = oracle.aabb_pairs(rays, boxes)
    one = ~two
    print(f"  NaN-origin pairs: oracle passes {100 * (ref[one] != 0).mean():.1f}% with one NaN component, "
          f"{100 * (ref[two] != 0).mean():.1f}% with two")
    assert (ref[one] != 0).mean() >= 0.10 and (ref[one] == 0).mean() >= 0.02   # (two axes left: most pairs pass)
    best = np.full(len(rays), np.float32(np.inf))
    for form in (abi.BOX_FORM_CONS_BOUNCE, abi.BOX_FORM_CONS_CAMERA, abi.BOX_FORM_SLAB_BOX):
        got = gpu.box_form_pairs(rays, boxes, best, form)
        bad = np.flatnonzero(got != ref)
        assert len(bad) == 0, f"form {form}: {len(bad)} of {len(rays)} pairs differ, first {rays[bad[0]]} {boxes[bad[0]]}"


def test_a_box_entered_at_infinity_is_not_beyond_an_infinite_best(gpu, mirt, oracle):
    """Origins at -sign(d) 3.0e38 on every axis with |d| = 2^-6: all six plane
    distances overflow to +inf, hit.c's tmin = tmax = +inf passes
    tmax >= tmin && tmax > EPS, and the pruning limit of a walk without a hit
    (or with a hit at t = +inf) is +inf too. The pruning growth is finite here
    (an infinite origin makes the entry estimate NaN instead), so the entry
    estimate is +inf itself, and `entry > lim` must stay false: every form
    equals hit.c's flag."""
    import test_filtered_forms as ff
    abi = mirt.abi
    s, b = ff.two_sphere_scene(mirt, 100.0)
    gpu.upload(s, b)
    rays, boxes = ff.edge_grazing(np.random.default_rng(8), 4096)
    d = rays["direction"].astype(np.float64)
    rays["direction"] = d / np.linalg.norm(d, axis=1)[:, None] * 2.0 ** -6
    rays["origin"] = np.where(rays["direction"] > 0, -3.0e38, 3.0e38).astype(np.float32)
    ref = oracle.aabb_pairs(rays, boxes)
    assert (ref == 1).all()
    best = np.full(len(rays), np.float32(np.inf))
    for form in (abi.BOX_FORM_SLAB, abi.BOX_FORM_SLAB_BOX, abi.BOX_FORM_CONS, abi.BOX_FORM_CONS_BOUNCE,
                 abi.BOX_FORM_CONS_CAMERA):
        got = gpu.box_form_pairs(rays, boxes, best, form)
        bad = np.flatnonzero(got != ref)
        assert len(bad) == 0, f"form {form}: {len(bad)} of {len(rays)} pairs fail, first {rays[bad[0]]} {boxes[bad[0]]}"


def test_the_twins_tie_to_the_later_leaf(gpu, mirt):
    """Exact duplicates in leaves of their own: every hit is an exact tie, at
    finite t in the walks that merge candidates with cand_better (quad batch,
    the four-wide walks, the bounce kernel's drain) and at t = +inf in the
    chunked walk. hit.c records the later leaf, brute force the first sphere."""
    abi = mirt.abi
    s, _, nodes = hc.twins()
    gpu.upload(s, mirt.Bvh(nodes))
    info, _ = gpu.resident_layout()
    assert info["ordered"]
    rays = hc.twins_rays()
    check_per_ray(gpu, mirt, rays, hc.twins_hits(), hc.twins_hits(False), "twins")
    w, h = hc.TWINS_W, hc.TWINS_H
    for what, opts, use_bvh in (("default", {}, True), ("DFS", {abi.OPT_ORDERED: 0, abi.OPT_PRUNE: 0}, True),
                                ("tile", {abi.OPT_TRAVERSAL: abi.TRAV_TILE}, True), ("brute force", {}, False)):
        with options(gpu, abi, opts):
            for depth in (1, 5, 8):
                want = hc.twins_colours(depth, use_bvh)
                same(gpu.trace_ray(rays, depth=depth, use_bvh=use_bvh), want, f"twins trace_ray {what} depth {depth}")
                rgba, got = gpu.render_rays(rays.reshape(h, w), w, h, planes=PLANES, depth=depth, use_bvh=use_bvh)
                same(rgba, want.reshape(h, w, 4), f"twins ray frame {what} depth {depth}")
                same_planes(got, cases.planes_of(hc.twins_hits(use_bvh), (h, w)), f"twins ray frame {what}")


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_trace_ray(gpu, mirt, name):
    abi = mirt.abi
    upload(gpu, mirt, N)
    flat = np.ascontiguousarray(hc.rays(name)).reshape(-1)
    for what, opts, use_bvh in (("default", {}, True), ("DFS", {abi.OPT_ORDERED: 0, abi.OPT_PRUNE: 0}, True),
                                ("brute force", {}, False)):
        with options(gpu, abi, opts):
            for depth in hc.DEPTHS:
                got = gpu.trace_ray(flat, depth=depth, use_bvh=use_bvh).reshape(H, W, 4)
                same(got, hc.colours(name, depth, use_bvh), f"{name} trace_ray {what} depth {depth}")
                if name in hc.MIXED:
                    keep = ~hc.substituted(name)
                    same_bytes(got[keep], hc.colours("base", depth, use_bvh)[keep], name + ": the unsubstituted rays")


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_ray_frames_on_every_schedule(gpu, mirt, name):
    abi = mirt.abi
    upload(gpu, mirt, N)
    rays = hc.rays(name)
    flat = np.ascontiguousarray(rays).reshape(-1)
    counted = []
    for schedule in SCHEDULES:
        depth, use_bvh, opts = schedules(abi)[schedule]
        what = f"{name} on {schedule}"
        with options(gpu, abi, opts):
            rgba, got = gpu.render_rays(rays, W, H, planes=PLANES, depth=depth, use_bvh=use_bvh)
            same(rgba, hc.colours(name, depth, use_bvh), what + " against the oracle")
            want = hc.hits(name, use_bvh)
            counted.append(same_planes(got, cases.planes_of(want, (H, W)), what))
            assert counted[-1] == plane_nans(want)
            # the product's own identities: no exception to byte equality
            same_bytes(rgba, gpu.render_rays(rays, W, H, depth=depth, use_bvh=use_bvh), what + " without planes")
            same_bytes(rgba, gpu.trace_ray(flat, depth=depth, use_bvh=use_bvh), what + " against mirt_trace_rays")
            rec = gpu.closest_hit(flat, use_bvh=use_bvh).reshape(H, W)
            for k in PLANES:
                same_bytes(got[k], rec[k], f"{what}: plane {k} against mirt_intersect_rays")
            same_bytes(got["t"][rec["hit"] == 0], np.zeros(int((rec["hit"] == 0).sum()), np.float32), what)
    print(f"  {name}: NaN-for-NaN plane elements per schedule {counted}; device NaN patterns {sorted(DEVICE_NAN)}")
    # the bounce pass's own options under the wavefront schedule
    for what, opts in walks(abi)[5:]:
        with options(gpu, abi, opts):
            same(gpu.render_rays(rays, W, H, depth=5), hc.colours(name, 5), f"{name}, {what}")
            same(gpu.render_rays(rays, W, H, depth=8), hc.colours(name, 8), f"{name}, {what}, depth 8")


@pytest.mark.parametrize("name", ["tiny_inf", "mixed_tiles_tiny"])
def test_ray_frames_in_shards_and_four_accumulating_samples(gpu, mirt, oracle, name):
    upload(gpu, mirt, N)
    rays = hc.rays(name)
    want = hc.colours(name, 5, True, seed=3, sample=2)
    seen = []
    for shard in range(3):
        kw = dict(depth=5, seed=3, sample=2, row_block=8, shard=shard, num_shards=3)
        rows = mirt.shard_rows(mirt.frame_desc(W, H, **kw))
        seen += list(rows)
        rgba, got = gpu.render_rays(np.ascontiguousarray(rays[rows]), W, H, planes=PLANES, **kw)
        same(rgba, want[rows], f"{name}: shard {shard}")
        same_planes(got, cases.planes_of(hc.hits(name)[rows], (len(rows), W)), f"{name}: shard {shard}")
    assert sorted(seen) == list(range(H))
    # samples = 4 into a buffer that already holds two frames
    n = W * H
    acc = np.zeros(3 * n, np.float32)
    shown = None
    for k in range(6):
        shown = oracle.accumulate(hc.colours(name, 5, True, seed=5, sample=k), acc, k == 0, k + 1).reshape(H, W, 4)
    gpu.render_rays(rays, W, H, depth=5, seed=5, sample=0)
    gpu.render_rays(rays, W, H, depth=5, seed=5, sample=1, accumulate=True, frames=2)
    got = gpu.render_rays(np.stack([rays] * 4), W, H, depth=5, seed=5, sample=2, samples=4, accumulate=True, frames=3)
    same(got, shown, f"{name}: four accumulating samples")
    same_bytes(gpu.accum(3 * n), acc, f"{name}: the accumulation buffer")


CAMERA_SCHEDULES = ["wavefront_ordered_d5", "tile_d5", "unordered_deferred_d5", "exact_slab_d5"]


@pytest.mark.parametrize("name", hc.CAMERAS)
def test_hostile_cameras(gpu, mirt, name):
    """render_frame and render_frame_planes against oracle.render on four
    schedules; with the primary cache on, the second frame of the same camera is
    a HIT -- the key is compared bitwise (mirt.h), so a NaN equals itself -- and
    has the first frame's bytes."""
    abi = mirt.abi
    upload(gpu, mirt, N)
    cam = hc.camera(name)
    for w, h in hc.CAMERA_SIZES:
        want = hc.camera_frame(name, w, h)
        for schedule in CAMERA_SCHEDULES:
            depth, use_bvh, opts = schedules(abi)[schedule]
            what = f"camera {name} {w}x{h} on {schedule}"
            with options(gpu, abi, opts):
                same(gpu.render_frame(cam, w, h, depth=depth, use_bvh=use_bvh), want, what)
                rgba, got = gpu.render_frame_planes(cam, w, h, depth=depth, use_bvh=use_bvh)
                same(rgba, want, what + " with planes")
                assert same_planes(got, hc.camera_planes(name, w, h, use_bvh), what) == 0
        with options(gpu, abi, {abi.OPT_PRIMARY_CACHE: 1}):
            first = gpu.render_frame(cam, w, h, depth=5)
            st = gpu.primary_cache_stats()
            assert (st["last"], st["valid"]) == ("fill", 1), (name, st)
            second = gpu.render_frame(cam, w, h, depth=5)
            st = gpu.primary_cache_stats()
            assert (st["last"], st["reason"]) == ("hit", ""), (name, st)
            same_bytes(second, first, f"camera {name} {w}x{h}: the frame from the cache")
            same(first, want, f"camera {name} {w}x{h}: the filling frame")


def test_the_reprojected_loop_through_hostile_cameras(gpu, mirt):
    """[A, NaN-x, A, 1e30, A]: every frame equals mirt_reproject_host fed that
    frame's own planes and the previous records, byte for byte."""
    upload(gpu, mirt, N)
    L = mirt.load()
    gpu.history_reset()
    prev = None
    for k, name in enumerate(["A", "nan_x", "A", "1e30_x", "A"]):
        cam = hc.camera(name)
        kw = dict(depth=5, seed=1, sample=k)
        raw_pl, pl = gpu.render_frame_planes(cam, W, H, planes=("t", "sphere"), **kw)
        hist, want = rpc.host_step(L, cam, raw_pl, pl["t"], pl["sphere"], prev, rpc.DEFAULT)
        prev = (cam, hist, pl["t"], pl["sphere"])
        out, raw = gpu.render_frame_reprojected(cam, W, H, params=rpc.DEFAULT, raw=True, **kw)
        same_bytes(raw, raw_pl, f"frame {k} ({name}): raw")
        same_bytes(out, want, f"frame {k} ({name}): out")
        same_bytes(gpu.history_read(), hist, f"frame {k} ({name}): the records")
        st = gpu.history_stats()
        assert st["reused"] + st["fresh"] + st["sky"] == W * H, (name, st)
        assert st["frames"] == k + 1
        if name != "A":
            assert st["sky"] == W * H, (name, st)
    gpu.history_reset()

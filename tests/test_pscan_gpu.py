"""The primary scan on the GPU (MIRT_OPT_PRIMARY_SCAN): the camera pass finds
each pixel's closest hit by a depth-sorted scan of the leaves per tile instead
of the packet walk. "Equal" below always means: equal, byte for byte
(tobytes() ==), to the same call on the same ctx with the option at 0 -- and
where an accumulation buffer is involved, accum() equal too. The stats say
which path ran. Every test restores the options it sets. Cameras and scenes:
tests/pscan_cases.py."""
import ctypes as C

import numpy as np
import pytest

import hostile_sphere_cases as hsc
import pscan_cases as cases
import test_planes_cases as planes

pytestmark = pytest.mark.gpu


def upload(r, mirt, n):
    spheres, _, nodes = planes.scene(n)
    r.upload(spheres, mirt.Bvh(nodes))
    return spheres


def frame(r, mirt, cam, W, H, **kw):
    """The blocking frame of mirt.frame_desc(W, H, **kw): bytes of (rows, W, 4) uint8."""
    fd = mirt.frame_desc(W, H, **kw)
    out = np.zeros((len(mirt.shard_rows(fd)), W, 4), np.uint8)
    rc = r.L.mirt_render_frame(r.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(out))
    assert rc == 0, (rc, r.L.mirt_last_error().decode())
    return out.tobytes()


class options:
    """Options set for one block and restored after it."""

    def __init__(self, r, opts):
        self.r, self.opts = r, opts

    def __enter__(self):
        self.old = {k: self.r.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.r.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.r.set_option(k, v)


def both(r, mirt, fn, on=1, extra=None):
    """fn() with the option at 0, then at `on` (from 0: nothing kept): (the two results, the stats after the second)."""
    scan = mirt.abi.OPT_PRIMARY_SCAN
    with options(r, {scan: 0}):
        want = fn()
        st0 = r.primary_scan_stats()
        assert (st0["last"], st0["reason"], st0["bytes"]) == ("bypass", "OFF", 0)
    with options(r, {scan: 0, **(extra or {})}):
        r.set_option(scan, on)
        got = fn()
        st = r.primary_scan_stats()
        r.set_option(scan, 0)
        assert r.primary_scan_stats()["bytes"] == 0      # setting 0 released the memory
    return want, got, st


def check(r, mirt, fn, label, expect=("scan", ""), **kw):
    want, got, st = both(r, mirt, fn, **kw)
    assert (st["last"], st["reason"]) == expect, (label, st)
    assert got == want, f"{label}: differs from the same call with the option off"
    return st


def test_the_option_defaults_to_automatic(mirt):
    with mirt.Renderer(0) as r:
        assert r.get_option(mirt.abi.OPT_PRIMARY_SCAN) == 2
        assert r.get_option(mirt.abi.OPT_PRIMARY_SCAN_BUDGET) == 256
        assert r.get_option(mirt.abi.OPT_PRIMARY_SCAN_REBUILD) == 0
        for opt, bad in ((mirt.abi.OPT_PRIMARY_SCAN, 3), (mirt.abi.OPT_PRIMARY_SCAN_BUDGET, 0)):
            with pytest.raises(mirt.MirtError):
                r.set_option(opt, bad)


@pytest.mark.parametrize("depth", [1, 5])
def test_160x90_of_2000_spheres(gpu, mirt, depth):
    """The reference frame: equal at depth 1 (the camera pass alone) and depth 5,
    with the automatic setting too; at the default budget at least 90 % of the
    tiles that hold a candidate finish in the scan, and the sky tiles end on
    their count."""
    upload(gpu, mirt, 2000)
    cam = cases.camera("default", 2000)
    for on in (1, 2):
        st = check(gpu, mirt, lambda: frame(gpu, mirt, cam, 160, 90, depth=depth, seed=3), f"depth {depth} on {on}",
                   on=on)
        print(st)
        tiles = st["tiles_scan"] + st["tiles_walk"] + st["tiles_empty"]
        assert tiles == 20 * 12 and st["rebuilds"] == 1 and 1900 < st["leaves"] <= 2000   # one record per live leaf
        assert st["tiles_scan"] >= 0.9 * (st["tiles_scan"] + st["tiles_walk"]), st
        assert st["tiles_empty"] > 0 and st["leaves_tested"] > 0


@pytest.mark.parametrize("W,H", [(77, 45), (9, 7)])
def test_sizes_that_are_no_multiple_of_eight(gpu, mirt, W, H):
    upload(gpu, mirt, 1000)
    cam = cases.camera("default")
    for depth in (1, 5):
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, W, H, depth=depth, seed=2), f"{W}x{H} depth {depth}")


@pytest.mark.parametrize("samples", [2, 5])
def test_several_samples_in_one_launch(gpu, mirt, samples):
    """8x8 tiles straddling frames (2) and the 4x4x4 packets (5) read the one slab."""
    upload(gpu, mirt, 1000)
    cam = cases.camera("default")

    def run():
        out = frame(gpu, mirt, cam, 77, 45, depth=5, seed=4, samples=samples, frames=samples)
        return out, gpu.accum(77 * 45 * 3).tobytes()
    check(gpu, mirt, run, f"samples {samples}")


def test_two_frames_in_flight(gpu, mirt):
    """mirt_multi, two lanes over two ranks of one device: frames in flight on
    several ctxs, each with its own per-camera data, shards of row_block 8."""
    spheres, _, nodes = planes.scene(1000)
    cam = cases.camera("default")
    W, H = 77, 45
    got = {}
    for on in (0, 1):
        with mirt.MultiRenderer([0, 0], lanes=2) as m:
            m.upload(spheres, mirt.Bvh(nodes))
            m.set_option(mirt.abi.OPT_PRIMARY_SCAN, on)
            bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(2)]
            try:
                frames = []
                for rnd in range(2):
                    for k in range(2):
                        m.render_frame_async(cam, mirt.frame_desc(W, H, depth=5, seed=2, sample=2 * rnd + k), bufs[k])
                    m.wait()
                    frames += [b.array.tobytes() for b in bufs]
                got[on] = frames
                if on:
                    for lane in range(2):
                        for rank in range(2):
                            st = m.primary_scan_stats(lane, rank)
                            assert (st["last"], st["scanned"], st["rebuilds"]) == ("scan", 2, 1), (lane, rank, st)
            finally:
                for b in bufs:
                    b.close()
    assert got[1] == got[0]


@pytest.mark.parametrize("nframes", [2, 4])
def test_nframes_in_one_launch(gpu, mirt, nframes):
    """mirt_multi_render_frames_async with nframes successive frames in one
    launch (the shape bench.py times): two ranks of one device, shards of
    row_block 8, `samples = nframes` inside each ctx, frame j read back from
    slab j; 2 has 8x8 tiles straddling frames, 4 takes the 4x4x4 packets. Every
    frame equals the same launch with the option at 0, and every rank scanned."""
    spheres, _, nodes = planes.scene(1000)
    cam = cases.camera("default")
    W, H = 77, 45
    got = {}
    for on in (0, 1):
        with mirt.MultiRenderer([0, 0], lanes=2) as m:
            m.upload(spheres, mirt.Bvh(nodes))
            m.set_option(mirt.abi.OPT_PRIMARY_SCAN, on)
            bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(2 * nframes)]
            try:
                for k in range(2):     # one launch per lane, nframes frames each
                    m.render_frames_async(cam, mirt.frame_desc(W, H, depth=5, seed=2, sample=k * nframes),
                                          bufs[k * nframes:(k + 1) * nframes], nframes=nframes)
                m.wait()
                got[on] = [b.array.tobytes() for b in bufs]
                for lane in range(2):
                    for rank in range(2):
                        st = m.primary_scan_stats(lane, rank)
                        want = ("scan", "", 1, 1) if on else ("bypass", "OFF", 0, 0)
                        assert (st["last"], st["reason"], st["scanned"], st["rebuilds"]) == want, (lane, rank, st)
            finally:
                for b in bufs:
                    b.close()
    assert len(set(got[0])) == 2 * nframes      # the frames differ from each other (other samples)
    for j in range(2 * nframes):
        assert got[1][j] == got[0][j], j


def test_the_accumulating_loop_with_a_camera_move(gpu, mirt):
    """Three still frames, a move, three more: equal frames and accumulation;
    the per-camera data are built once for the still frames and again after the move."""
    upload(gpu, mirt, 1000)
    cam0 = cases.camera("default")
    cam1 = cases.camera("default")
    cam1.position.x += 0.5
    seq = [(cam0, False, 1), (cam0, True, 2), (cam0, True, 3), (cam1, False, 1), (cam1, True, 2), (cam1, True, 3)]
    rebuilds = []

    def loop():
        out = []
        for k, (cam, acc, frames) in enumerate(seq):
            out.append(frame(gpu, mirt, cam, 77, 45, depth=5, seed=2, sample=k, accumulate=acc, frames=frames))
            out.append(gpu.accum(77 * 45 * 3).tobytes())
            rebuilds.append(gpu.primary_scan_stats()["rebuilds"])
        return out
    st = check(gpu, mirt, loop, "loop")
    assert rebuilds[6:] == [1, 1, 1, 2, 2, 2] and st["scanned"] == 6, rebuilds


def test_rebuilding_every_frame_gives_the_same_frames(gpu, mirt):
    upload(gpu, mirt, 1000)
    cam = cases.camera("default")
    st = check(gpu, mirt, lambda: [frame(gpu, mirt, cam, 77, 45, depth=5, seed=2, sample=k) for k in range(3)],
               "rebuild", extra={mirt.abi.OPT_PRIMARY_SCAN_REBUILD: 1})
    assert st["rebuilds"] == 3


def test_shards(gpu, mirt):
    """Shard 1 of 3: at row_block 8 a tile's rows are one image band (scanned);
    at row_block 4 they are not (a bypass, SHARD)."""
    upload(gpu, mirt, 1000)
    cam = cases.camera("default")
    for depth in (1, 5):
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, 77, 45, depth=depth, shard=1, num_shards=3, row_block=8),
              "row_block 8")
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, 77, 45, depth=depth, shard=1, num_shards=3, row_block=16),
              "row_block 16")
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, 77, 45, depth=depth, shard=1, num_shards=3, row_block=4),
              "row_block 4", expect=("bypass", "SHARD"))


@pytest.mark.parametrize("name,W,H,n", cases.FRAMES, ids=[f"{c[0]}_{c[1]}x{c[2]}_{c[3]}" for c in cases.FRAMES])
def test_cameras(gpu, mirt, name, W, H, n):
    upload(gpu, mirt, n)
    cam = cases.camera(name, n)
    for depth in (1, 5):
        st = check(gpu, mirt, lambda: frame(gpu, mirt, cam, W, H, depth=depth, seed=5), f"{name} depth {depth}")
    if name == "looking_away":
        assert st["tiles_empty"] == ((W + 7) // 8) * ((H + 7) // 8)


@pytest.mark.parametrize("name", cases.BAD_CAMERAS)
def test_cameras_the_scan_bypasses(gpu, mirt, name):
    upload(gpu, mirt, 100)
    cam, _ = cases.bad_camera(name)
    check(gpu, mirt, lambda: frame(gpu, mirt, cam, 44, 26, depth=5), name, expect=("bypass", "CAMERA"))


def _built(spheres):
    o = planes._oracle()
    s = spheres.copy()
    tree = o.build(s)
    nodes = o.flatten(tree)
    o.free(tree)
    return s, nodes


def test_two_coincident_spheres_the_tie_goes_to_the_larger_index(gpu, mirt, oracle):
    s = planes._oracle().render_scene(1, 200)
    s["center"][0] = (0.0, 4.0, 20.0)
    s["radius"][0] = 6.0
    s["color"][0] = (255, 0, 0, 255)
    s[1] = s[0]
    s["color"][1] = (0, 255, 0, 255)
    s, nodes = _built(s)
    twins = np.flatnonzero((s["center"] == s["center"][np.flatnonzero(s["radius"] == 6.0)[0]]).all(axis=1))
    assert len(twins) == 2
    gpu.upload(s, mirt.Bvh(nodes))
    cam = cases.abi.default_camera()
    for depth in (1, 5):
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, 80, 48, depth=depth), f"twins depth {depth}")
    # and it is the oracle's frame: the twin with the larger index shows at the centre
    with options(gpu, {mirt.abi.OPT_PRIMARY_SCAN: 1}):
        img = gpu.render_frame(cam, 80, 48, depth=1)
    tree = oracle.build(s2 := s.copy())
    assert (s2 == s).all()
    ref = oracle.render(cam, 80, 48, s2, tree, depth=1, mode=1, seed=1)
    oracle.free(tree)
    assert img.tobytes() == ref.tobytes()


def test_a_silhouette_that_ends_on_a_tile_border(gpu, mirt):
    """A sphere tangent to the plane of the image's centre column (u = 0 at
    x = 80 of 160) and to the centre row's: its silhouette ends where tile
    columns 9 | 10 and rows 5 | 6 of a 160 x 96 frame meet."""
    s = planes._oracle().render_scene(1, 100)
    cam = cases.abi.default_camera()
    s["center"][0] = (cam.position.x - 3.0, cam.position.y - 3.0, 10.0)
    s["radius"][0] = 3.0
    s["center"][1] = (cam.position.x + 2.0, cam.position.y + 2.0, 12.0)
    s["radius"][1] = 2.0
    s, nodes = _built(s)
    gpu.upload(s, mirt.Bvh(nodes))
    for depth in (1, 5):
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, 160, 96, depth=depth), f"border depth {depth}")


def test_a_tree_that_does_not_nest_is_a_bypass(gpu, mirt):
    """The oracle's tree with the root's box cut in half: the boxes no longer
    nest, the ordered walks are off and with them the scan; the reason says so."""
    spheres, _, nodes = planes.scene(100)
    nodes = nodes.copy()
    nodes["bmax"][0][0] = 0.5 * (nodes["bmin"][0][0] + nodes["bmax"][0][0])
    gpu.upload(spheres, mirt.Bvh(nodes))
    cam = cases.camera("default", 100)
    want, got, st = both(gpu, mirt, lambda: frame(gpu, mirt, cam, 44, 26, depth=5))
    assert (st["last"], st["reason"]) == ("bypass", "SCHEDULE"), st   # (TREE: the next test)
    assert got == want


def test_a_nesting_tree_beyond_the_coordinate_bound_is_a_bypass_tree(gpu, mirt):
    """One sphere 70,000 units off: the tree nests and is ordered (the camera
    pass is the ordered packet kernel), but its coordinates exceed the 6e4 bound
    the margins assume, so o_bound is 0 and the reason is TREE exactly."""
    s = planes._oracle().render_scene(1, 100)
    s["center"][0] = (70000.0, 0.0, 0.0)
    s, nodes = _built(s)
    lay, _ = mirt.scene_layout(s, mirt.Bvh(nodes))
    assert lay["encloses"] and lay["ordered"] and lay["o_bound"] == 0.0, {k: lay[k] for k in ("encloses", "ordered", "o_bound")}
    gpu.upload(s, mirt.Bvh(nodes))
    cam = cases.abi.default_camera()
    for depth in (1, 5):
        check(gpu, mirt, lambda: frame(gpu, mirt, cam, 44, 26, depth=depth), f"far sphere depth {depth}",
              expect=("bypass", "TREE"))


def test_automatic_mode_leaves_a_sparse_scene_to_the_walk(gpu, mirt):
    """10,000 spheres at a tenth of their radius: most tiles that hold a record
    keep a sky pixel and read far into the records. Option 2 scans the first
    frame, finds more than 16 chunks per such tile and bypasses (SPARSE) from
    then on, until another scene is installed; option 1 keeps scanning. Equal
    bytes throughout."""
    abi = mirt.abi
    s = planes._oracle().render_scene(1, 10000)
    s["radius"] *= 0.1
    s, nodes = _built(s)
    gpu.upload(s, mirt.Bvh(nodes))
    cam = cases.abi.default_camera()
    seen = []

    def run():
        out = []
        for k in range(3):
            out.append(frame(gpu, mirt, cam, 160, 90, depth=5, seed=2, sample=k))
            st = gpu.primary_scan_stats()        # (waits for the frame: the verdict has landed)
            seen.append((st["last"], st["reason"]))
            if st["last"] == "scan":
                assert st["chunks"] > 16 * (st["tiles_scan"] + st["tiles_walk"]), st
        return out
    want, got, st = both(gpu, mirt, run, on=2)
    assert got == want and seen[3:] == [("scan", ""), ("bypass", "SPARSE"), ("bypass", "SPARSE")], seen
    del seen[:]
    check(gpu, mirt, run, "option 1")
    assert seen[3:] == [("scan", "")] * 3, seen
    # a dense scene installed on the same ctx is scanned again under option 2
    upload(gpu, mirt, 2000)
    with options(gpu, {abi.OPT_PRIMARY_SCAN: 2}):
        for k in range(2):
            frame(gpu, mirt, cases.camera("default", 2000), 160, 90, depth=5, sample=k)
            st = gpu.primary_scan_stats()
            assert (st["last"], st["reason"]) == ("scan", ""), st


def test_budget_one_sends_covered_tiles_to_the_walk_list(gpu, mirt):
    upload(gpu, mirt, 2000)
    cam = cases.camera("default", 2000)
    for depth in (1, 5):
        st = check(gpu, mirt, lambda: frame(gpu, mirt, cam, 160, 90, depth=depth, seed=3), f"budget 1 depth {depth}",
                   extra={mirt.abi.OPT_PRIMARY_SCAN_BUDGET: 1})
        print(st)
        assert st["budget"] == 1 and st["tiles_walk"] > st["tiles_scan"] > 0, st


def test_other_frames_are_bypasses_with_their_reason(gpu, mirt):
    abi = mirt.abi
    upload(gpu, mirt, 1000)
    cam = cases.camera("default")
    run = lambda **kw: (lambda: frame(gpu, mirt, cam, 44, 26, **kw))
    check(gpu, mirt, run(depth=5, jitter=True), "jitter", expect=("bypass", "JITTER"))
    check(gpu, mirt, run(depth=5, use_bvh=False), "brute force", expect=("bypass", "SCHEDULE"))
    check(gpu, mirt, run(depth=0), "depth 0", expect=("bypass", "SCHEDULE"))
    check(gpu, mirt, run(depth=5), "tile schedule", expect=("bypass", "SCHEDULE"),
          extra={abi.OPT_TRAVERSAL: abi.TRAV_TILE})
    check(gpu, mirt, run(depth=5), "cache on", expect=("bypass", "CACHE"), extra={abi.OPT_PRIMARY_CACHE: 1})


@pytest.mark.parametrize("name", hsc.SCENES)
def test_hostile_spheres(gpu, mirt, name):
    """The hostile-sphere scenes through the option: a bypass or equal bytes."""
    s, _, nodes = hsc.scene(name)
    gpu.upload(s, mirt.Bvh(nodes))
    for cam_name, W, H in hsc.ray_sets(name):
        cam = hsc.camera(name, cam_name)
        for depth in (1, 5):
            want, got, st = both(gpu, mirt, lambda: frame(gpu, mirt, cam, W, H, depth=depth))
            assert got == want, (name, cam_name, depth, st["last"], st["reason"])
            assert st["last"] == "scan" or st["reason"] in ("TREE", "SCHEDULE", "CAMERA"), st

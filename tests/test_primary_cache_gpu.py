"""The primary cache on the GPU (MIRT_OPT_PRIMARY_CACHE): a frame whose camera
rays are those of the frame that filled the cache starts from the stored hits
instead of the walk. "Equal" below always means: equal, byte for byte, to the
same call on the same ctx with the option at 0 -- and where an accumulation
buffer is involved, accum() equal too. Every test restores the option it sets.
The cases and their oracle planes are tests/test_planes_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import test_planes_cases as cases

pytestmark = pytest.mark.gpu


def upload(r, mirt, n):
    spheres, _, nodes = cases.scene(n)
    r.upload(spheres, mirt.Bvh(nodes))
    return spheres


def frame(r, mirt, cam, W, H, **kw):
    """The blocking frame of mirt.frame_desc(W, H, **kw): (rows, W, 4) uint8."""
    fd = mirt.frame_desc(W, H, **kw)
    out = np.zeros((len(mirt.shard_rows(fd)), W, 4), np.uint8)
    rc = r.L.mirt_render_frame(r.h, C.byref(cam), C.byref(fd), mirt.abi.ptr(out))
    assert rc == 0, (rc, r.L.mirt_last_error().decode())
    return out


class cache:
    """The option set to `value` for one block (from 0: the cache starts empty) and restored after it."""

    def __init__(self, r, mirt, value=1):
        self.r, self.opt, self.value = r, mirt.abi.OPT_PRIMARY_CACHE, value

    def __enter__(self):
        self.old = self.r.get_option(self.opt)
        self.r.set_option(self.opt, 0)
        self.r.set_option(self.opt, self.value)
        return self

    def __exit__(self, *a):
        self.r.set_option(self.opt, self.old)


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


def last(r):
    st = r.primary_cache_stats()
    return (st["last"], st["reason"])


def run_steps(r, mirt, steps, on):
    """Every step's result (bytes) and, with the option on, how its last frame met the cache."""
    got = []
    with cache(r, mirt, 1 if on else 0):
        for label, step, _ in steps:
            res = step()
            st = r.primary_cache_stats()
            got.append((res, (st["last"], st["reason"]), st["valid"]))
    return got


def check_steps(r, mirt, steps):
    """steps: (label, callable -> bytes, expected (last, reason)). Once with
    the option off, once with it on: equal results, the expected classes."""
    want = run_steps(r, mirt, steps, False)
    got = run_steps(r, mirt, steps, True)
    for (label, _, expect), (w, wl, _), (g, gl, valid) in zip(steps, want, got):
        assert wl == ("bypass", "OFF"), label
        assert gl == expect, (label, gl, expect)
        assert g == w, f"{label}: the frame differs from the frame with the option off"
        assert valid == 1, label
    assert r.get_option(mirt.abi.OPT_PRIMARY_CACHE) == 0
    st = r.primary_cache_stats()
    assert st["bytes"] == 0 and st["valid"] == 0     # setting 0 released the memory


def moved_camera(mirt, name="A", dx=0.5):
    cam = cases.camera(name)
    cam.position.x += dx
    return cam


def test_the_accumulating_loop(gpu, mirt):
    """main.c:349-408 at case A: a fresh frame, two accumulating ones, a camera
    move, three more -- fill, hit, hit, fill (CAMERA), hit, hit, hit; the slab
    after the first fill is the oracle's t and sphere planes bit for bit."""
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    upload(gpu, mirt, c["n"])
    cam0, cam1 = cases.camera("A"), moved_camera(mirt)
    seq = [(cam0, False, 1), (cam0, True, 2), (cam0, True, 3), (cam1, False, 1), (cam1, True, 2), (cam1, True, 3),
           (cam1, True, 4)]

    def loop():
        out = []
        for k, (cam, acc, frames) in enumerate(seq):
            out.append(frame(gpu, mirt, cam, W, H, depth=5, seed=2, sample=k, accumulate=acc, frames=frames))
            st = gpu.primary_cache_stats()
            out.append((st["last"], st["reason"]))
            if k == 0 and st["valid"]:
                t, s = gpu.primary_cache_read()
                want = cases.expected("A")
                assert t.shape == (H, W) and t.view(np.uint32).tobytes() == want["t"].view(np.uint32).tobytes()
                assert s.tobytes() == want["sphere"].tobytes()
                assert (st["width"], st["rows"], st["scene_id"]) == (W, H, gpu.scene_id())
                assert st["bytes"] >= 8 * W * H
        return out[0::2], out[1::2], gpu.accum(W * H * 3)

    with cache(gpu, mirt, 0):
        want, classes, want_acc = loop()
        assert classes == [("bypass", "OFF")] * 7
    with cache(gpu, mirt):
        got, classes, got_acc = loop()
        st = gpu.primary_cache_stats()
    assert classes == [("fill", "EMPTY"), ("hit", ""), ("hit", ""), ("fill", "CAMERA"), ("hit", ""), ("hit", ""),
                       ("hit", "")]
    assert (st["hits"], st["fills"], st["bypassed"]) == (5, 2, 0)
    for k in range(len(seq)):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got_acc.tobytes() == want_acc.tobytes()
    assert any(got[k].tobytes() != got[k + 1].tobytes() for k in range(6))   # the frames do differ among themselves


SHAPES = {
    "depth1_primary_only": ("A", dict(depth=1)),
    "depth2": ("A", dict(depth=2)),
    "depth5": ("A", dict(depth=5)),
    "samples3_tiles_straddle_frames": ("A", dict(depth=5, samples=3)),
    "samples5_packets": ("A", dict(depth=5, samples=5)),
    "samples5_depth1": ("A", dict(depth=1, samples=5)),
    "shard": ("A", dict(depth=5, num_shards=3, shard=1, row_block=4)),
    "shard_samples3": ("A", dict(depth=5, num_shards=3, shard=1, row_block=4, samples=3)),
    "shard_samples5": ("A", dict(depth=5, num_shards=3, shard=1, row_block=4, samples=5)),
    "lead_skip3": ("A", dict(depth=5, num_shards=3, shard=1, row_block=4, lead_skip=3)),
    "case_b_unbounded_fill": ("B", dict(depth=5)),
    "case_c": ("C", dict(depth=5)),
    "case_c_samples5": ("C", dict(depth=5, samples=5)),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_of_the_cached_index(gpu, mirt, shape):
    """First as a fill, again as a hit, each equal; several frames in one call
    also equal `samples` single-frame calls' last display and accumulation."""
    name, kw = SHAPES[shape]
    c = cases.CASES[name]
    W, H = c["W"], c["H"]
    upload(gpu, mirt, c["n"])
    cam = cases.camera(name)
    fd = mirt.frame_desc(W, H, **kw)
    rows = len(mirt.shard_rows(fd))
    assert 0 < rows <= H
    if name == "B":
        info, _ = gpu.resident_layout()
        assert info["ordered"] and 600 > 4 * info["o_bound"] > 0
    n = kw.get("samples", 1)
    with cache(gpu, mirt, 0):
        want = frame(gpu, mirt, cam, W, H, seed=3, sample=4, **kw)
        want_acc = gpu.accum(rows * W * 3)
        if n > 1:
            one = {k: v for k, v in kw.items() if k != "samples"}
            for j in range(n):
                single = frame(gpu, mirt, cam, W, H, seed=3, sample=4 + j, accumulate=j > 0, frames=1 + j, **one)
            assert single.tobytes() == want.tobytes() and gpu.accum(rows * W * 3).tobytes() == want_acc.tobytes()
    with cache(gpu, mirt):
        for expect in (("fill", "EMPTY"), ("hit", "")):
            got = frame(gpu, mirt, cam, W, H, seed=3, sample=4, **kw)
            assert last(gpu) == expect
            assert got.tobytes() == want.tobytes(), expect
            assert gpu.accum(rows * W * 3).tobytes() == want_acc.tobytes(), expect
        st = gpu.primary_cache_stats()
        assert (st["width"], st["rows"]) == (W, rows)
        if n > 1:   # the single frames of the same camera: hits, all of them
            for j in range(n):
                single = frame(gpu, mirt, cam, W, H, seed=3, sample=4 + j, accumulate=j > 0, frames=1 + j, **one)
                assert last(gpu) == ("hit", "")
            assert single.tobytes() == want.tobytes() and gpu.accum(rows * W * 3).tobytes() == want_acc.tobytes()
        if name == "B":   # filled by the unbounded kernel, read by the one cached kernel
            t, s = gpu.primary_cache_read()
            assert t.tobytes() == cases.expected("B")["t"].tobytes()
            assert s.tobytes() == cases.expected("B")["sphere"].tobytes()


def test_a_hit_frame_reads_the_cache(gpu, mirt):
    """A slab of misses makes the next hit frame pure sky: the brute-force
    frame of an empty scene, which depends on ray.dy only. Slabs that could
    index out of bounds are refused whole."""
    c = cases.CASES["A"]
    W, H, n = c["W"], c["H"], c["n"]
    upload(gpu, mirt, n)
    cam0, cam1 = cases.camera("A"), moved_camera(mirt)
    with mirt.Renderer(0) as empty:
        empty.upload(np.zeros(0, mirt.abi.SPHERE), None)
        sky = frame(empty, mirt, cam0, W, H, depth=5, use_bvh=False)
    with cache(gpu, mirt, 0):
        plain0 = frame(gpu, mirt, cam0, W, H, depth=5)
        plain1 = frame(gpu, mirt, cam1, W, H, depth=5)
    assert plain0.tobytes() != sky.tobytes()
    with cache(gpu, mirt):
        assert frame(gpu, mirt, cam0, W, H, depth=5).tobytes() == plain0.tobytes() and last(gpu) == ("fill", "EMPTY")
        gpu.primary_cache_write(np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32))
        got = frame(gpu, mirt, cam0, W, H, depth=5)
        assert last(gpu) == ("hit", "")
        assert got.tobytes() == sky.tobytes()
        # a moved camera fills again
        assert frame(gpu, mirt, cam1, W, H, depth=5).tobytes() == plain1.tobytes() and last(gpu) == ("fill", "CAMERA")
        t, s = gpu.primary_cache_read()
        hit = np.argwhere(s >= 0)[0]
        bad = []
        for what, value in (("sphere == num_spheres", n), ("sphere == -2", -2)):
            s2 = s.copy()
            s2[tuple(hit)] = value
            bad.append((what, t, s2))
        t2 = t.copy()
        t2[tuple(hit)] = np.nan
        bad.append(("t = NaN at a hit", t2, s))
        t3 = t.copy()
        t3[tuple(hit)] = 0.0
        bad.append(("t = 0 at a hit", t3, s))
        bad.append(("wrong n", t.reshape(-1)[:-1], s.reshape(-1)[:-1]))
        for what, tt, ss in bad:
            with pytest.raises(mirt.MirtError):
                gpu.primary_cache_write(tt, ss)
            t4, s4 = gpu.primary_cache_read()
            assert t4.tobytes() == t.tobytes() and s4.tobytes() == s.tobytes(), what   # nothing was written
            assert frame(gpu, mirt, cam1, W, H, depth=5).tobytes() == plain1.tobytes(), what
            assert last(gpu) == ("hit", ""), what
        gpu.primary_cache_write(t, s)   # and the slab as read is accepted
        assert frame(gpu, mirt, cam1, W, H, depth=5).tobytes() == plain1.tobytes() and last(gpu) == ("hit", "")


def test_scene_installs_invalidate(mirt):
    """Every install gives the scene a new id, so the next frame fills (SCENE):
    upload, build_scene, refit_scene, update_scene refitting and rebuilding."""
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    cam = cases.camera("A")
    spheres, _, nodes = cases.scene(c["n"])
    rng = np.random.default_rng(11)

    def moved(s, sigma):
        out = np.array(s)
        out["center"] += rng.normal(0.0, sigma, (len(out), 3)).astype(np.float32)
        return out

    with mirt.Renderer(0) as r:
        state = {"s": np.array(spheres)}

        def build():
            state["s"] = r.build_scene(np.array(spheres))

        def refit():
            state["s"] = moved(state["s"], 0.05)
            r.refit_scene(state["s"])

        def update(max_decay, rebuilt):
            reordered, _, res = r.update_scene(moved(state["s"], 2.0 if rebuilt else 0.05), max_decay=max_decay)
            assert res["rebuilt"] == rebuilt, res
            state["s"] = reordered

        installs = [("upload", lambda: r.upload(spheres, mirt.Bvh(nodes))),
                    ("upload again", lambda: r.upload(spheres, mirt.Bvh(nodes))),
                    ("build_scene", build), ("refit_scene", refit),
                    ("update_scene refit", lambda: update(0.0, 0)), ("update_scene rebuild", lambda: update(1e-6, 1))]
        ids = set()
        with cache(r, mirt):
            for k, (what, install) in enumerate(installs):
                install()
                ids.add(r.scene_id())
                got = frame(r, mirt, cam, W, H, depth=5, sample=k)
                assert last(r) == ("fill", "SCENE" if k else "EMPTY"), what
                assert r.primary_cache_stats()["scene_id"] == r.scene_id()
                with cache(r, mirt, 0):   # the same call with the option at 0 (the cache is dropped: EMPTY next)
                    want = frame(r, mirt, cam, W, H, depth=5, sample=k)
                assert got.tobytes() == want.tobytes(), what
                for expect in (("fill", "EMPTY"), ("hit", "")):
                    assert frame(r, mirt, cam, W, H, depth=5, sample=k).tobytes() == want.tobytes(), (what, expect)
                    assert last(r) == expect, what
        assert len(ids) == len(installs)


def test_camera_and_geometry_invalidate_the_rest_hits(gpu, mirt):
    import torch
    abi = mirt.abi
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    upload(gpu, mirt, c["n"])
    cam = cases.camera("A")
    cam_pos = moved_camera(mirt)
    cam_yaw = cases.camera("A")
    cam_yaw.yaw = np.float32(cam_yaw.yaw + 0.05)
    mirt.camera_update(cam_yaw)
    cam_fov = cases.camera("A")
    cam_fov.fov = 50.0
    shard = dict(num_shards=3, shard=1, row_block=4)

    def f(cam, W=W, H=H, accum=False, opts=None, **kw):
        def step():
            with options(gpu, opts or {}):
                out = frame(gpu, mirt, cam, W, H, **{"depth": 5, **kw})
            rows = out.shape[0]
            return out.tobytes() + (gpu.accum(rows * W * 3).tobytes() if accum else b"")
        return step

    def on_a_torch_stream():
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        d_out = torch.zeros(W * H, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        gpu.render_frame_device(cam, mirt.frame_desc(W, H, depth=5, sample=9), d_out.data_ptr(),
                                stream=stream.cuda_stream)
        stream.synchronize()
        return d_out.cpu().numpy().tobytes()

    FILL_C, FILL_G, HIT = ("fill", "CAMERA"), ("fill", "GEOMETRY"), ("hit", "")
    steps = [
        ("base", f(cam), ("fill", "EMPTY")),
        ("position", f(cam_pos), FILL_C), ("position again", f(cam_pos), HIT),
        ("yaw", f(cam_yaw), FILL_C), ("fov", f(cam_fov), FILL_C), ("back", f(cam), FILL_C),
        ("width", f(cam, W=52), FILL_G), ("width again", f(cam, W=52), HIT),
        ("height", f(cam, H=30), FILL_G), ("back from height", f(cam), FILL_G),
        ("row_block", f(cam, row_block=4), FILL_G),
        ("a shard", f(cam, **shard), FILL_G), ("the shard again", f(cam, **shard), HIT),
        ("another shard", f(cam, **{**shard, "shard": 2}), FILL_G),
        ("lead_skip", f(cam, **{**shard, "shard": 2, "lead_skip": 3}), FILL_G),
        ("back to the frame", f(cam), FILL_G),
        # none of these is in the key
        ("seed", f(cam, seed=7), HIT), ("sample", f(cam, sample=5), HIT),
        ("max_depth 2", f(cam, depth=2), HIT), ("max_depth 1", f(cam, depth=1), HIT),
        ("fresh, with the buffer", f(cam, accum=True, sample=6), HIT),
        ("accumulate", f(cam, accum=True, sample=7, accumulate=True, frames=2), HIT),
        ("samples", f(cam, accum=True, sample=8, samples=3), HIT),
        ("bounce threshold", f(cam, opts={abi.OPT_BOUNCE_THRESHOLD: 40}), HIT),
        ("queue order 1", f(cam, opts={abi.OPT_QUEUE_ORDER: 1}), HIT),
        ("queue order 2", f(cam, opts={abi.OPT_QUEUE_ORDER: 2}), HIT),
        ("zero copy off", f(cam, opts={abi.OPT_ZERO_COPY: 0}), HIT),
        ("a caller's stream", on_a_torch_stream, HIT),
        ("and back on the ctx's", f(cam, sample=10), HIT),
    ]
    check_steps(gpu, mirt, steps)


def test_bypasses_leave_the_cache_alone(gpu, mirt):
    abi = mirt.abi
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    upload(gpu, mirt, c["n"])
    cam = cases.camera("A")

    def f(opts=None, **kw):
        def step():
            with options(gpu, opts or {}):
                return frame(gpu, mirt, cam, W, H, **{"depth": 5, **kw}).tobytes()
        return step

    def with_planes():
        rgba, pl = gpu.render_frame_planes(cam, W, H, depth=5)
        assert pl["sphere"].tobytes() == cases.expected("A")["sphere"].tobytes()
        return rgba.tobytes() + b"".join(pl[k].tobytes() for k in ("t", "sphere", "normal"))

    def counted():
        return repr(sorted(gpu.count_frame(cam, W, H, depth=5).items())).encode()

    S = ("bypass", "SCHEDULE")
    steps = [
        ("fill", f(), ("fill", "EMPTY")),
        ("jitter", f(jitter=True), ("bypass", "JITTER")), ("jittered samples", f(jitter=True, samples=5), ("bypass", "JITTER")),
        ("planes", with_planes, ("bypass", "PLANES")),
        ("tile", f({abi.OPT_TRAVERSAL: abi.TRAV_TILE}), S), ("brute force", f(use_bvh=False), S),
        ("unordered", f({abi.OPT_ORDERED: 0}), S), ("exact slab", f({abi.OPT_FAST_SLAB: 0}), S),
        ("no pruning", f({abi.OPT_PRUNE: 0}), S),
        ("count_frame", counted, S),
        ("plain", f(), ("hit", "")),
        ("jittered tile", f({abi.OPT_TRAVERSAL: abi.TRAV_TILE}, jitter=True), S),   # the first reason in the order
        ("plain again", f(sample=3), ("hit", "")),
    ]
    check_steps(gpu, mirt, steps)
    with cache(gpu, mirt):
        for _, step, _ in steps:
            step()
        st = gpu.primary_cache_stats()
        assert (st["fills"], st["hits"], st["bypassed"]) == (1, 2, 10)
        t, s = gpu.primary_cache_read()   # still the first frame's hits
        assert t.tobytes() == cases.expected("A")["t"].tobytes() and s.tobytes() == cases.expected("A")["sphere"].tobytes()


def test_scene_group_members_fill_once_each_and_again_after_an_install(mirt):
    """Two ctxs share one scene, async frames in flight on both: each has its
    own cache; an install through one makes both fill; frames enqueued before
    it finish on the old scene."""
    c = cases.CASES["A"]
    W, H = c["W"], c["H"]
    cam = cases.camera("A")
    spheres, _, nodes = cases.scene(c["n"])
    after = np.array(spheres)
    after["center"] += np.random.default_rng(5).normal(0.0, 0.5, (len(after), 3)).astype(np.float32)

    with mirt.Renderer(0) as r1, mirt.Renderer(0) as r2:
        r2.share_scene(r1)
        rs = (r1, r2)
        bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(8)]

        def procedure(on):
            r1.upload(spheres, mirt.Bvh(nodes))
            assert r1.scene_id() == r2.scene_id() != 0
            classes = []
            with cache(r1, mirt, on), cache(r2, mirt, on):
                old = [frame(rs[k % 2], mirt, cam, W, H, depth=5, sample=k).tobytes() for k in (4, 5)] if not on else None
                for k in range(6):   # 0..3: fill, fill, hit, hit; 4, 5 stay in flight over the install
                    rs[k % 2].render_frame_async(cam, mirt.frame_desc(W, H, depth=5, sample=k), bufs[k])
                    classes.append(last(rs[k % 2]))
                r1.update_scene(after)
                assert r1.scene_id() == r2.scene_id()
                for k in (6, 7):
                    rs[k % 2].render_frame_async(cam, mirt.frame_desc(W, H, depth=5, sample=k), bufs[k])
                    classes.append(last(rs[k % 2]))
                r1.wait()
                r2.wait()
                stats = [r.primary_cache_stats() for r in rs]
            return [b.array.tobytes() for b in bufs], classes, stats, old

        try:
            want, off, _, old = procedure(0)
            got, classes, stats, _ = procedure(1)
        finally:
            for b in bufs:
                b.close()
    assert off == [("bypass", "OFF")] * 8
    assert classes == [("fill", "EMPTY")] * 2 + [("hit", "")] * 4 + [("fill", "SCENE")] * 2
    for st in stats:
        assert (st["fills"], st["hits"], st["bypassed"]) == (2, 2, 0)
    for k in range(8):
        assert got[k] == want[k], k
    assert got[4] == old[0] and got[5] == old[1]        # in flight over the install: the old scene's frames
    assert got[6] != got[0] and got[7] != got[1]        # the scene did move


def expected_counts(seq, lanes):
    """Per lane: (fills, hits) the classification rule gives for the frames
    that lane's ctxs issued -- frame k runs on lane k % lanes; a ctx fills on
    its first frame and whenever the camera differs from its previous frame's."""
    out = []
    for lane in range(lanes):
        fills = hits = 0
        held = None
        for k, (cam_id, _, _) in enumerate(seq):
            if k % lanes != lane:
                continue
            if held == cam_id:
                hits += 1
            else:
                fills += 1
                held = cam_id
        out.append((fills, hits))
    return out


@pytest.mark.parametrize("devices,direct,W,H,rb", [([0, 0], False, 44, 26, 8), ([0, 0, 0], True, 77, 45, 16)])
def test_multi_lanes_accumulating_loop_with_the_cache(gpu, mirt, devices, direct, W, H, rb):
    """The loop of test_the_accumulating_loop through mirt_multi, three lanes,
    lengthened so that every lane sees two still frames per camera: frames
    equal the blocking one-ctx sequence; per (lane, rank) the hits and fills are
    those the rule gives for the frames that ctx issued."""
    c = cases.CASES["A"]
    spheres, _, nodes = cases.scene(c["n"])
    upload(gpu, mirt, c["n"])
    cams = [cases.camera("A"), moved_camera(mirt)]
    seq = [(i, k > 0, k + 1) for i in (0, 1) for k in range(6)]   # (camera, accumulate, frames)
    lanes = 3
    with cache(gpu, mirt, 0):
        want = [frame(gpu, mirt, cams[i], W, H, depth=5, seed=2, sample=k, accumulate=a, frames=f)
                for k, (i, a, f) in enumerate(seq)]
    expect = expected_counts(seq, lanes)
    assert all(fills == 2 and hits == 2 for fills, hits in expect)
    with mirt.MultiRenderer(devices, lanes=lanes, host_direct=direct) as m:
        m.upload(spheres, mirt.Bvh(nodes))
        m.set_option(mirt.abi.OPT_PRIMARY_CACHE, 1)
        assert m.get_option(mirt.abi.OPT_PRIMARY_CACHE) == 1
        bufs = [mirt.HostBuffer((H, W, 4)) for _ in range(lanes)]
        got = []
        try:
            for k, (i, a, f) in enumerate(seq):
                fd = mirt.frame_desc(W, H, depth=5, seed=2, sample=k, accumulate=a, frames=f, row_block=rb)
                m.render_frame_async(cams[i], fd, bufs[k % lanes])
                if k % lanes == lanes - 1:
                    m.wait()
                    got += [bufs[j % lanes].array.copy() for j in range(len(got), k + 1)]
            stats = {(l, r): m.primary_cache_stats(l, r) for l in range(lanes) for r in range(len(devices))}
            m.set_option(mirt.abi.OPT_PRIMARY_CACHE, 0)
            assert all(m.primary_cache_stats(l, r)["bytes"] == 0 for l, r in stats)
        finally:
            for b in bufs:
                b.close()
    for k in range(len(seq)):
        assert got[k].tobytes() == want[k].tobytes(), k
    for (l, r), st in stats.items():
        assert (st["fills"], st["hits"], st["bypassed"]) == (*expect[l], 0), (l, r, st)
        assert st["valid"] == 1 and st["last"] == "hit" and st["width"] == W and 0 < st["rows"] < H

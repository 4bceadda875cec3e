"""Product host code (libmirt.so, no GPU calls) against the reference's golden
vectors: glibc rand restatement, scene generators, the bit-identical BVH
build (flat and pointer-tree forms), shard geometry, and the C ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, sha


def test_rand_matches_glibc(mirt, golden):
    for seed, vals in golden["rand"].items():
        st = mirt.RandState(int(seed))
        assert [st.rand() for _ in range(len(vals))] == vals, seed


def test_rand_matches_libc_directly(mirt):
    libc = C.CDLL("libc.so.6")
    for seed in [3, 99, 2**31 - 1, 2**31]:
        libc.srand(C.c_uint(seed))
        st = mirt.RandState(seed)
        assert [st.rand() for _ in range(1000)] == [libc.rand() for _ in range(1000)]


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [20, 100, 1000])
def test_scene_and_flat_tree(mirt, small, seed, n):
    s = mirt.create_random_spheres(n, seed)
    assert s.tobytes() == small[f"render_{n}_{seed}_pre"].tobytes()
    b = mirt.build_bvh(s)
    assert s.tobytes() == small[f"render_{n}_{seed}_post"].tobytes()
    assert b.nodes.tobytes() == small[f"render_{n}_{seed}_tree"].tobytes()


@pytest.mark.parametrize("n", [20, 1000])
def test_pointer_tree_dropin(mirt, small, n):
    """mirt_build_bvh_node returns the reference's 56-B pointer layout; its
    flattening equals the reference tree."""
    s = small[f"render_{n}_1_pre"].copy()
    root = mirt.build_bvh_node(s)
    assert s.tobytes() == small[f"render_{n}_1_post"].tobytes()
    f = mirt.flatten_bvh(root, s)
    assert f.nodes.tobytes() == small[f"render_{n}_1_tree"].tobytes()
    mirt.free_bvh(root)


def test_bench_scene_tree(mirt, small):
    s = mirt.create_benchmark_spheres(1000, 1)
    assert s.tobytes() == small["bench_1000_1_pre"].tobytes()
    b = mirt.build_bvh(s, 0, 999, 20)                       # benchmark.c:317
    assert b.nodes.tobytes() == small["bench_1000_1_tree"].tobytes()


@pytest.mark.parametrize("key", ["render_10000_1", "render_100000_1", "bench_1000000_1", "render_1000000_1"])
def test_large_trees_bit_identical(mirt, golden, key):
    kind, n, seed = key.split("_")
    n = int(n)
    s = mirt.create_random_spheres(n, 1) if kind == "render" else mirt.create_benchmark_spheres(n, 1)
    g = golden["scenes"][key]
    assert sha(s) == g["scene_sha"]
    b = mirt.build_bvh(s)
    assert sha(s) == g["post_sha"]
    assert len(b) == g["nodes"]
    assert sha(b.nodes) == g["tree_sha"]


def test_degenerate_builds(mirt, oracle):
    """Coincident centres (no SAH plane separates them: bvh.c:139-141
    fallback, empty children, depth-40 chains), N = 0 and 1, equal to the
    oracle's straightforward restatement."""
    from oracle.lib import abi
    cases = []
    s = np.zeros(50, abi.SPHERE)
    s["center"] = [1.0, 2.0, 3.0]
    s["radius"] = 0.5
    cases.append(s)
    s2 = np.zeros(37, abi.SPHERE)
    s2["center"][:, 0] = np.repeat(np.float32([-1, 0, 2]), [12, 13, 12])
    s2["radius"] = np.float32(0.75)
    cases.append(s2)
    cases.append(np.zeros(1, abi.SPHERE))
    cases.append(np.zeros(0, abi.SPHERE))
    for c in cases:
        a, b = c.copy(), c.copy()
        got = mirt.build_bvh(a)
        t = oracle.build(b)
        ref = oracle.flatten(t)
        oracle.free(t)
        assert a.tobytes() == b.tobytes()
        assert got.nodes.tobytes() == ref.tobytes()


@pytest.mark.parametrize("H,rb,world,d", [(1080, 8, 1, 0), (1080, 8, 2, 0), (1080, 8, 8, 0), (1080, 8, 3, 0),
                                          (90, 8, 7, 0), (13, 4, 5, 0), (2160, 16, 8, 0), (1080, 8, 8, 2),
                                          (1080, 8, 2, 7), (1080, 8, 3, 1), (90, 8, 7, 3), (13, 4, 5, 5),
                                          (187, 8, 8, 4), (7, 8, 3, 2), (2160, 16, 8, 6)])
def test_shard_rows_partition(mirt, H, rb, world, d):
    """Every row in exactly one shard, compact rows in image order; the C
    geometry (mirt_shard_rows, csrc/shard.h) equals shard.py's. d: the
    lead-skip weighting (shard 0 sits out d of every 8 rounds)."""
    from importlib import import_module
    shard = import_module("cs201_sah-bvh_ray_tracer_amd.shard")
    seen = []
    src_shard, pos = shard.row_sources(H, rb, world, d)
    for s in range(world):
        fd = mirt.frame_desc(64, H, row_block=rb, shard=s, num_shards=world, lead_skip=d)
        rows = mirt.shard_rows(fd)
        assert len(rows) == shard.shard_row_count(H, rb, world, s, d)
        assert (rows == shard.shard_rows_of(H, rb, world, s, d)).all()
        assert (np.diff(rows) > 0).all()
        if d == 0:
            assert all((y // rb) % world == s for y in rows)
        seen.extend(rows.tolist())
        for k, y in enumerate(rows):
            assert int(src_shard[y]) == s and int(pos[y]) == k
    assert sorted(seen) == list(range(H))
    assert shard.slab_rows(H, rb, world, d) == max(shard.shard_row_count(H, rb, world, s, d) for s in range(world))
    if d and H >= 8 * rb * world:
        # shard 0 renders (8 - d) blocks of every 8 world - d
        share = shard.shard_row_count(H, rb, world, 0, d) / H
        assert abs(share - (8 - d) / (8 * world - d)) < 0.05


def test_lead_skip_needs_shards(mirt):
    """lead_skip in 0..7, and only for a frame split over two shards or more."""
    for fd in (mirt.frame_desc(64, 64, lead_skip=1), mirt.frame_desc(64, 64, num_shards=2, lead_skip=8),
               mirt.frame_desc(64, 64, num_shards=2, lead_skip=-1)):
        with pytest.raises(mirt.MirtError):
            mirt.shard_rows(fd)


def test_invalid_frame_desc_raises(mirt):
    fd = mirt.frame_desc(0, 10)
    with pytest.raises(mirt.MirtError):
        mirt.shard_rows(fd)
    fd = mirt.frame_desc(10, 10, shard=3, num_shards=2)
    with pytest.raises(mirt.MirtError):
        mirt.shard_rows(fd)


def test_abi_exports_every_declared_symbol(mirt):
    """libmirt.so loads and exports every function include/*.h declares
    (and abi.SIGNATURES covers exactly those)."""
    declared = set()
    for h in ("mirt.h", "mirt_dropin.h", "mirt_multi.h"):
        hdr = open(os.path.join(ROOT, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        declared |= set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", hdr))
    L = mirt.load()
    for name in declared:
        assert hasattr(L, name), name
    assert declared == {n for n, _, _ in mirt.abi.SIGNATURES}


def test_struct_layouts(mirt, golden):
    abi = mirt.abi
    sz = golden["sizeof"]
    assert abi.SPHERE.itemsize == sz["Sphere"] == 20
    assert abi.CAMERA.itemsize == sz["Camera"] == 64
    assert sz["BVHNode"] == 56 and sz["HitRecord"] == 40 and abi.HIT.itemsize == 40
    import ctypes
    assert ctypes.sizeof(abi.HitRecord) == 40 and ctypes.sizeof(abi.Ray) == 24 and ctypes.sizeof(abi.Aabb) == 24


def test_default_camera_and_update(mirt, small):
    cam = mirt.default_camera()
    ref = mirt.abi.Camera.from_numpy(small["cameras"][0])
    assert bytes(cam) == bytes(ref)
    turned = mirt.abi.Camera.from_numpy(small["cameras"][1])
    c2 = mirt.default_camera()
    c2.yaw, c2.pitch, c2.position = turned.yaw, turned.pitch, turned.position
    mirt.camera_update(c2)                                   # camera.c:10-18
    assert bytes(c2) == bytes(turned)


def test_no_gpu_create_fails_loudly(mirt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(mirt.MirtError):
        mirt.Renderer(0)


@pytest.mark.parametrize("levels", ["0", "1", "4", "6"])
def test_threaded_build_same_tree(mirt, golden, levels, monkeypatch):
    """The build forks child subtrees onto threads (MIRT_BVH_FORK_LEVELS);
    any number of fork levels gives the reference's tree, bit for bit."""
    monkeypatch.setenv("MIRT_BVH_FORK_LEVELS", levels)
    g = golden["scenes"]["render_100000_1"]
    s = mirt.create_random_spheres(100000, 1)
    b = mirt.build_bvh(s)
    assert sha(b.nodes) == g["tree_sha"]
    s = mirt.create_random_spheres(70000, 3)
    ref = s.copy()
    monkeypatch.setenv("MIRT_BVH_FORK_LEVELS", "0")
    one = mirt.build_bvh(ref)
    monkeypatch.setenv("MIRT_BVH_FORK_LEVELS", levels)
    root = mirt.build_bvh_node(s)
    try:
        assert (s == ref).all()
        assert mirt.flatten_bvh(root, s).nodes.tobytes() == one.nodes.tobytes()
    finally:
        mirt.free_bvh(root)


def test_tree_cache_file(mirt, small, tmp_path):
    """mirt_bvh_build_flat_cached: a miss builds and
    writes the file, a hit loads the same reordered spheres and nodes bit for
    bit; a file for other spheres, a corrupted or truncated file is rebuilt."""
    path = tmp_path / "scene.bvh"
    for attempt, want in [(0, 0), (1, 1)]:
        s = small["render_1000_1_pre"].copy()
        b, cached = mirt.build_bvh_cached(path, s)
        assert cached == want, attempt
        assert s.tobytes() == small["render_1000_1_post"].tobytes()
        assert b.nodes.tobytes() == small["render_1000_1_tree"].tobytes()
    # other spheres (and other build arguments) miss and overwrite
    s = small["bench_1000_1_pre"].copy()
    b, cached = mirt.build_bvh_cached(path, s, 0, 999, 20)  # benchmark.c:317
    assert cached == 0 and b.nodes.tobytes() == small["bench_1000_1_tree"].tobytes()
    s = small["bench_1000_1_pre"].copy()
    assert mirt.build_bvh_cached(path, s, 0, 1000, 20)[1] == 0
    assert mirt.build_bvh_cached(path, small["bench_1000_1_pre"].copy(), 0, 1000, 20)[1] == 1
    # corrupt one payload byte, then truncate: both rebuild the same tree
    raw = bytearray(path.read_bytes())
    raw[len(raw) // 2] ^= 0x40
    path.write_bytes(bytes(raw))
    s = small["render_1000_1_pre"].copy()
    b, cached = mirt.build_bvh_cached(path, s)
    assert cached == 0 and b.nodes.tobytes() == small["render_1000_1_tree"].tobytes()
    path.write_bytes(path.read_bytes()[:-7])
    s = small["render_1000_1_pre"].copy()
    assert mirt.build_bvh_cached(path, s)[1] == 0
    assert s.tobytes() == small["render_1000_1_post"].tobytes()
    # an unwritable path still returns the built tree, flagged -1
    s = small["render_1000_1_pre"].copy()
    b, cached = mirt.build_bvh_cached(tmp_path / "no_such_dir" / "x.bvh", s)
    assert cached == -1 and b.nodes.tobytes() == small["render_1000_1_tree"].tobytes()
    assert not list(tmp_path.glob("*.tmp.*"))


def _node(sphere, skip, lo=(0, 0, 0), hi=(1, 1, 1)):
    return (lo, hi, sphere, skip)


def test_validate_flat_tree(mirt, small):
    """mirt_bvh_validate_flat (run by both uploads and the cache loader)
    accepts the reference's trees and rejects every malformed shape that
    could send the layout builders or kernels out of bounds."""
    abi = mirt.abi
    for key in ("render_1000_1_tree", "bench_1000_1_tree"):
        mirt.validate_bvh(small[key], 1000)
    mirt.validate_bvh(np.zeros(0, abi.NODE), 0)
    E = abi.NODE_EMPTY
    bad = {
        # inner node whose right child is the end of the array
        "right_child_at_end": [_node(-1, 2), _node(0, 2)],
        "truncated": [_node(-1, 3), _node(0, 2), _node(1, 3)][:2],
        "root_skip": [_node(-1, 3), _node(0, 2), _node(1, 3), _node(2, 4)],
        "leaf_skip": [_node(-1, 3), _node(0, 3), _node(1, 3)],
        "not_nested": [_node(-1, 5), _node(-1, 4), _node(0, 3), _node(1, 4), _node(2, 6), _node(3, 6)][:5],
        "right_overruns": [_node(-1, 4), _node(-1, 3), _node(0, 3), _node(1, 5), _node(2, 5)],
        "sphere_range": [_node(-1, 3), _node(0, 2), _node(7, 3)],
        "bad_sphere": [_node(-1, 3), _node(0, 2), _node(-5, 3)],
        "empty_inner": [_node(-1, 3 | E), _node(0, 2), _node(1, 3)],
        "skip_backwards": [_node(-1, 3), _node(0, 0), _node(1, 3)],
    }
    for name, rows in bad.items():
        arr = np.array(rows, dtype=abi.NODE)
        with pytest.raises(mirt.MirtError):
            mirt.validate_bvh(arr, 3)
            raise AssertionError(name)
    ok = np.array([_node(-1, 3), _node(0, 2), _node(3, 3 | E)], dtype=abi.NODE)   # sentinel + empty leaf
    mirt.validate_bvh(ok, 3)


def _fnv_words(h, b):
    n8 = len(b) // 8 * 8
    for w in np.frombuffer(b[:n8], dtype="<u8").tolist():
        h = ((h ^ w) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    for c in b[n8:]:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_tree_cache_rejects_forged_files(mirt, small, tmp_path):
    """The cache hashes carry no secret: a file rewritten with a
    recomputed payload hash but a malformed tree, or spheres that are not a
    permutation of the input, is treated as a miss and rebuilt."""
    import struct
    path = tmp_path / "scene.bvh"
    s = small["render_1000_1_pre"].copy()
    mirt.build_bvh_cached(path, s)
    raw = bytearray(path.read_bytes())
    hdr, body = raw[:48], raw[48:]
    ns = 1000
    sph = np.frombuffer(bytes(body[:20 * ns]), dtype=mirt.abi.SPHERE).copy()
    nodes = np.frombuffer(bytes(body[20 * ns:]), dtype=mirt.abi.NODE).copy()

    def forge(sph2, nodes2):
        payload = _fnv_words(1469598103934665603, sph2.tobytes() + nodes2.tobytes())
        h = bytes(hdr[:40]) + struct.pack("<Q", payload)
        path.write_bytes(h + sph2.tobytes() + nodes2.tobytes())

    # 1. an inner node's right child pointed past its parent's subtree
    n2 = nodes.copy()
    inner = np.nonzero(n2["sphere"] < 0)[0]
    n2["skip"][inner[3] + 1] = len(n2)          # left child's subtree "ends" at the array end
    forge(sph, n2)
    s = small["render_1000_1_pre"].copy()
    b, cached = mirt.build_bvh_cached(path, s)
    assert cached == 0 and b.nodes.tobytes() == small["render_1000_1_tree"].tobytes()
    # 2. a leaf index out of range
    n2 = nodes.copy()
    n2["sphere"][np.nonzero(n2["sphere"] >= 0)[0][5]] = 5000
    forge(sph, n2)
    s = small["render_1000_1_pre"].copy()
    assert mirt.build_bvh_cached(path, s)[1] == 0
    # 3. spheres that are not a permutation of the input
    s2 = sph.copy()
    s2["radius"][17] += 1.0
    forge(s2, nodes)
    s = small["render_1000_1_pre"].copy()
    assert mirt.build_bvh_cached(path, s)[1] == 0
    assert s.tobytes() == small["render_1000_1_post"].tobytes()
    # the genuine file still hits
    assert mirt.build_bvh_cached(path, small["render_1000_1_pre"].copy())[1] == 1


def test_sanitizer_builds(tmp_path):
    """The host C++ (threaded build, validation, tree cache file incl. corrupt,
    truncated and unwritable files, the scene layout builders) under ASan+UBSan and under TSan
    (tests/c/san_host.cpp via `make -C csrc san`): every check holds and no
    sanitizer reports."""
    import subprocess
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "san"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    for exe in ("san_asan", "san_tsan"):
        p = subprocess.run([os.path.join(csrc, "build", exe), str(tmp_path)], capture_output=True, text=True,
                           timeout=600, env=env)
        assert p.returncode == 0 and "san_host: ok" in p.stdout, (exe, p.stdout[-1500:], p.stderr[-3000:])


@pytest.mark.parametrize("kind,n,start,end,depth", [("render", 10000, 0, None, 0), ("render", 100000, 0, None, 0),
                                                    ("bench", 20000, 0, None, 0), ("bench", 20000, 0, 19999, 20)])
def test_phantom_leaves_are_covered(mirt, kind, n, start, end, depth):
    """Every 0-sphere leaf of the BASELINE scenes' trees (and of a
    benchmark.c:317-style build over [0, n - 1) from depth 20) points at a
    sphere some non-empty leaf tests first, or at the never-hit index N: so
    the upload keeps the fast walks (scene_layout.cpp orphan_phantoms / dead_leaf)
    on the trees the bench and the parity tests run."""
    s = mirt.create_random_spheres(n, 1) if kind == "render" else mirt.create_benchmark_spheres(n, 1)
    nd = mirt.build_bvh(s, start, end, depth).nodes
    ns = (end if end is not None else n) - start
    leaf = nd["sphere"] >= 0
    empty = leaf & ((nd["skip"] & mirt.abi.NODE_EMPTY) != 0)
    tested = set(nd["sphere"][leaf & ~empty].tolist())
    pointed = set(nd["sphere"][empty].tolist())
    assert pointed - tested <= {start + ns}, sorted(pointed - tested)[:5]


@pytest.mark.parametrize("H,rb,world,d", [(1080, 8, 1, 0), (1080, 8, 8, 0), (45, 8, 3, 0), (90, 8, 7, 0),
                                          (13, 4, 5, 0), (187, 8, 8, 0), (7, 8, 3, 0), (1080, 8, 8, 2),
                                          (187, 8, 8, 5), (45, 8, 3, 1), (90, 8, 7, 7), (13, 4, 5, 3)])
def test_delivery_index_math_restated(H, rb, world, d):
    """shard.py's restatements of multi.hip's two deliveries (the gather's
    deinterleave_kernel and host-direct's strided copies, short last block
    included) rebuild a frame from its shards' compact slabs."""
    from importlib import import_module
    shard = import_module("cs201_sah-bvh_ray_tracer_amd.shard")
    rng = np.random.default_rng(H * 31 + world)
    full = rng.integers(0, 1 << 31, size=(2, H, 11), dtype=np.int64)
    src, _ = shard.row_sources(H, rb, world, d)
    slabs = [full[:, [y for y in range(H) if src[y] == s]] for s in range(world)]
    for s in range(world):
        assert slabs[s].shape[1] == shard.shard_row_count(H, rb, world, s, d)
    assert (shard.assemble_gather(slabs, H, rb, d) == full).all()
    assert (shard.assemble_direct(slabs, H, rb, d) == full).all()

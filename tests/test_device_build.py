"""mirt_bvh_build_flat_device: the SAH build on the GPU returns the host
builder's flat tree and reordered sphere array, compared on bytes; and its
partition kernels reproduce bvh.c:172-201's swap loop."""
import numpy as np
import pytest

from conftest import sha

pytestmark = pytest.mark.gpu


def dev_build(gpu, mirt, s, start=0, end=None, depth=0, on_device=1):
    """Device build of s (in place) -> nodes; checks the statistics and the tree's form."""
    b = gpu.build_bvh(s, start, end, depth)
    st = gpu.last_build_stats()
    assert st["on_device"] == on_device, st
    assert st["nodes"] == len(b)
    if on_device:
        assert 1 <= st["levels"] <= max(1, 41 - depth) and st["device_ms"] > 0.0
        assert st["total_ms"] >= st["device_ms"]
    else:
        assert st["device_ms"] == 0.0
    mirt.validate_bvh(b.nodes, len(s))
    return b.nodes


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [20, 100, 1000])
def test_reference_fixtures(gpu, mirt, small, n, seed):
    s = small[f"render_{n}_{seed}_pre"].copy()
    nodes = dev_build(gpu, mirt, s)
    assert same(s, small[f"render_{n}_{seed}_post"])
    assert same(nodes, small[f"render_{n}_{seed}_tree"])


def test_benchmark_fixture(gpu, mirt, small):
    s = small["bench_1000_1_pre"].copy()
    nodes = dev_build(gpu, mirt, s, 0, 999, 20)          # benchmark.c:317
    assert same(s, small["bench_1000_1_post"])
    assert same(nodes, small["bench_1000_1_tree"])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 64, 65])
def test_tiny(gpu, mirt, n):
    s = mirt.create_random_spheres(n, 3)
    ref = s.copy()
    want = mirt.build_bvh(ref).nodes
    nodes = dev_build(gpu, mirt, s)
    assert same(s, ref) and same(nodes, want)


def test_sub_range(gpu, mirt):
    s = mirt.create_random_spheres(300, 4)
    ref = s.copy()
    want = mirt.build_bvh(ref, 5, 297, 33).nodes
    nodes = dev_build(gpu, mirt, s, 5, 297, 33)
    assert same(s, ref) and same(nodes, want)
    assert not same(s, mirt.create_random_spheres(300, 4))   # the range was reordered


def test_degenerate(gpu, mirt, oracle):
    """The inputs of test_degenerate_builds: coincident centres (no plane wins:
    axis 0, split 0.0, chains of empty leaves down to depth 40), three clusters
    on x, n = 1 and n = 0, against the oracle's build."""
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
        nodes = dev_build(gpu, mirt, a)
        t = oracle.build(b)
        ref = oracle.flatten(t)
        oracle.free(t)
        assert same(a, b)
        assert same(nodes, ref)


def quantised_scene(mirt, seed):
    """Coordinates and radii on multiples of 1/8, few distinct values, one axis
    constant: centres land exactly on split planes, boxes have zero extent,
    costs tie, and groups of equal centres are stuck down to depth 40."""
    r = np.random.default_rng(seed)
    n = 4096 if seed == 0 else int(r.integers(2, 4097))
    span = int(r.integers(1, 33))
    s = np.zeros(n, mirt.abi.SPHERE)
    s["center"] = r.integers(-span, span + 1, (n, 3)) / 8.0
    s["center"][:, seed % 3] = r.integers(-4, 5) / 8.0
    s["radius"] = r.integers(0, 4, n) / 8.0
    s["color"] = r.integers(0, 256, (n, 4))
    return s


@pytest.mark.parametrize("group", range(4))
def test_ties_and_flat_axes(gpu, mirt, group):
    for seed in range(12 * group, 12 * group + 12):
        s = quantised_scene(mirt, seed)
        ref = s.copy()
        want = mirt.build_bvh(ref).nodes
        nodes = dev_build(gpu, mirt, s)
        assert same(s, ref), seed
        assert same(nodes, want), seed


def golden_scene(gpu, mirt, golden, key):
    n = int(key.split("_")[1])
    s = mirt.create_random_spheres(n, 1)
    g = golden["scenes"][key]
    assert sha(s) == g["scene_sha"]
    nodes = dev_build(gpu, mirt, s)
    assert sha(s) == g["post_sha"]
    assert len(nodes) == g["nodes"]
    assert sha(nodes) == g["tree_sha"]


@pytest.mark.parametrize("key", ["render_10000_1", "render_100000_1"])
def test_golden_shas(gpu, mirt, golden, key):
    golden_scene(gpu, mirt, golden, key)


def test_golden_sha_1m(gpu, mirt, golden):
    golden_scene(gpu, mirt, golden, "render_1000000_1")


# ---- the partition kernels on caller-given keys

def swap_loop(centre, lo, hi, split, perm):
    """bvh.c:172-201 on perm[lo:hi] (perm[j] = source index at position j)."""
    mid = lo
    for i in range(lo, hi):
        if centre[perm[i]] < split:
            perm[i], perm[mid] = perm[mid], perm[i]
            mid += 1


def pattern(kind, n, rng):
    """float32 keys for split 0.5: 0 goes left, 1 stays right."""
    if kind == "left":
        f = np.zeros(n)
    elif kind == "right":
        f = np.ones(n)
    elif kind == "alternating":
        f = np.arange(n) % 2 == 0
    elif kind == "one_right_then_left":       # the longest chain: the right element walks every left one
        f = np.arange(n) == 0
    else:
        f = rng.random(n) < rng.random()
    return np.asarray(f, np.float32)


KINDS = ["left", "right", "alternating", "one_right_then_left", "random"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 64, 65, 4097])
def test_partition_probe_one_segment(gpu, n, kind):
    rng = np.random.default_rng(n)
    centre = pattern(kind, n, rng)
    got = gpu.partition_probe(centre, [0, n], [0.5])
    want = np.arange(n, dtype=np.int32)
    swap_loop(centre, 0, n, np.float32(0.5), want)
    assert (got == want).all()


def test_partition_probe_many_segments(gpu):
    """37 segments of mixed patterns and lengths, empty ones among them, with a
    gap before the first and after the last; every segment its own split."""
    rng = np.random.default_rng(37)
    lens = [0, 1, 2, 64, 65, 0, 300, 1, 4097, 0, 0, 63, 129, 2, 1000, 7, 0, 64, 65, 2048, 3, 1, 0, 511, 513, 2, 0,
            100, 4097, 1, 64, 0, 65, 17, 2049, 5, 0]
    assert len(lens) == 37
    seg = np.cumsum([11] + lens).astype(np.int32)
    n = int(seg[-1]) + 9
    centre = rng.random(n).astype(np.float32)
    split = np.zeros(37, np.float32)
    for k, m in enumerate(lens):
        split[k] = np.float32(0.5 + k)
        centre[seg[k]:seg[k + 1]] = pattern(KINDS[k % 5], m, rng) + np.float32(k)
    got = gpu.partition_probe(centre, seg, split)
    want = np.arange(n, dtype=np.int32)
    for k in range(37):
        swap_loop(centre, int(seg[k]), int(seg[k + 1]), split[k], want)
    assert (got == want).all()


# ---- inputs the kernels decline, and the tree in use

def test_declined_inputs(gpu, mirt, small):
    """A NaN radius, and a sphere box with a -0.0 coordinate: the host builder
    runs on the untouched input; the next ordinary scene is built on the device."""
    for case in ("nan", "negzero"):
        s = small["render_100_1_pre"].copy()
        if case == "nan":
            s["radius"][17] = np.nan
        else:
            s["center"][5] = [-0.0, 1.0, 2.0]
            s["radius"][5] = 0.0
        ref = s.copy()
        want = mirt.build_bvh(ref).nodes
        b = gpu.build_bvh(s)
        st = gpu.last_build_stats()
        assert st["on_device"] == 0 and st["device_ms"] == 0.0 and st["nodes"] == len(b), case
        assert same(s, ref) and same(b.nodes, want), case
    s = small["render_100_1_pre"].copy()
    nodes = dev_build(gpu, mirt, s, on_device=1)
    assert same(s, small["render_100_1_post"]) and same(nodes, small["render_100_1_tree"])


def test_device_tree_renders_the_golden_frame(gpu, mirt, golden, small):
    s = small["render_100_1_pre"].copy()
    b = gpu.build_bvh(s)
    assert gpu.last_build_stats()["on_device"] == 1
    gpu.upload(s, b)
    cam = mirt.abi.Camera.from_numpy(small["cameras"][0])
    img = gpu.render_frame(cam, 160, 90, depth=5, seed=1)
    assert sha(img) == golden["frames"]["160x90_render100_d5_m1_b1_s1_c0_step1"]["sha"]

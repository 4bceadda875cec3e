"""The finish of the device build (MIRT_OPT_BUILD_FINISH, subtree_kernel of
csrc/bvh_device.hip): once no open node of a level holds more than F spheres,
one wave per open node builds the node's whole subtree. Every case compares
the spheres and the nodes on bytes with the host builder (the oracle's build
for the degenerate ones), and the finish's statistics -- where it took over,
how many subtrees and nodes it wrote, that pass B moved nothing -- with the
values build_finish_cases.finish_expect derives from the host tree."""
import struct

import numpy as np
import pytest
import torch

from build_finish_cases import finish_expect
from conftest import sha

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_stats(gpu, want_nodes, end, F, what=""):
    """last_build_finish against the host tree; F: the range in effect."""
    fin = gpu.last_build_finish()
    exp = finish_expect(want_nodes, F, end)
    assert fin["range"] == F and fin["moved"] == 0, (what, fin)
    assert {k: fin[k] for k in ("round", "subtrees", "nodes")} == {k: exp[k] for k in ("round", "subtrees", "nodes")}, \
        (what, fin, exp)
    assert (fin["finish_ms"] > 0.0) == (exp["round"] >= 0), (what, fin)
    return exp


def check_build(gpu, mirt, s, start=0, end=None, depth=0, F=64, want=None, what=""):
    """Device build of s[start:end] against the host builder (or the given
    (spheres, nodes)), bytes and statistics; returns the expected statistics."""
    end = len(s) if end is None else end
    if want is None:
        ref = s.copy()
        want = (ref, mirt.build_bvh(ref, start, end, depth).nodes)
    got = gpu.build_bvh(s, start, end, depth).nodes
    assert same(s, want[0]), what
    assert same(got, want[1]), what
    st = gpu.last_build_stats()
    assert st["on_device"] == 1 and st["nodes"] == len(got), (what, st)
    exp = check_stats(gpu, want[1], end, F, what)
    assert st["levels"] == exp["levels"], (what, st, exp)
    return exp


class finish_range:
    """MIRT_OPT_BUILD_FINISH set for a block, the default (1) restored."""

    def __init__(self, gpu, mirt, value):
        self.gpu, self.opt, self.value = gpu, mirt.abi.OPT_BUILD_FINISH, value

    def __enter__(self):
        self.gpu.set_option(self.opt, self.value)
        assert self.gpu.get_option(self.opt) == self.value

    def __exit__(self, *a):
        self.gpu.set_option(self.opt, 1)


def test_default_is_automatic(gpu, mirt):
    assert gpu.get_option(mirt.abi.OPT_BUILD_FINISH) == 1


# ---- the whole tree in the finish

@pytest.mark.parametrize("n", [2, 3, 7, 63, 64])
def test_whole_tree_in_the_finish(gpu, mirt, n):
    exp = check_build(gpu, mirt, mirt.create_random_spheres(n, 3))
    assert exp["round"] == 0 and exp["levels"] == 1 and exp["subtrees"] == 1


def test_65_runs_one_level_round_first(gpu, mirt):
    exp = check_build(gpu, mirt, mirt.create_random_spheres(65, 3))
    assert exp["round"] == 1 and exp["levels"] == 2


@pytest.mark.parametrize("n", [0, 1])
def test_nothing_to_finish(gpu, mirt, n):
    exp = check_build(gpu, mirt, mirt.create_random_spheres(n, 3))
    assert exp["round"] == -1 and exp["levels"] == 1


# ---- the depth cap

def test_degenerate_groups(gpu, mirt, oracle):
    """test_degenerate's inputs, against the oracle's build: coincident centres
    chain empty leaves down to a depth-40 leaf holding the whole group."""
    from oracle.lib import abi
    s = np.zeros(50, abi.SPHERE)
    s["center"] = [1.0, 2.0, 3.0]
    s["radius"] = 0.5
    s2 = np.zeros(37, abi.SPHERE)
    s2["center"][:, 0] = np.repeat(np.float32([-1, 0, 2]), [12, 13, 12])
    s2["radius"] = np.float32(0.75)
    for c in (s, s2):
        a, b = c.copy(), c.copy()
        t = oracle.build(b)
        ref = oracle.flatten(t)
        oracle.free(t)
        exp = check_build(gpu, mirt, a, want=(b, ref), what=str(len(c)))
        assert exp["round"] == 0 and exp["nodes"] == len(ref)
        assert (ref["sphere"] >= 0).sum() > 40          # the chain's empty leaves


@pytest.mark.parametrize("depth", [0, 33, 39, 40])
def test_64_from_depth(gpu, mirt, depth):
    """From depth 39 the finish root's children are all leaves; at depth 40 the
    root is a leaf and there is no finish."""
    exp = check_build(gpu, mirt, mirt.create_random_spheres(64, 7), 0, 64, depth, what=str(depth))
    if depth == 40:
        assert exp == dict(round=-1, subtrees=0, nodes=0, levels=1)
    else:
        assert exp["round"] == 0
    if depth == 39:
        assert exp["nodes"] == 3


# ---- sub-ranges: leaf indices count from the array, the rest is untouched

@pytest.mark.parametrize("n,start,end,depth", [(300, 5, 297, 33), (40, 3, 38, 0)])
def test_sub_range(gpu, mirt, n, start, end, depth):
    s = mirt.create_random_spheres(n, 4)
    before = s.copy()
    exp = check_build(gpu, mirt, s, start, end, depth)
    assert exp["round"] >= 0
    assert same(s[:start], before[:start]) and same(s[end:], before[end:])
    assert not same(s, before)


# ---- the partition inside a wave

def pattern_scene(mirt, kind):
    """64 spheres on the x axis in two tight groups far apart, so that the
    root's plane falls between the groups: `left` of each sphere in array
    order is the pattern the wave partitions."""
    n = 64
    rng = np.random.default_rng(5)
    if kind == "alternating":
        left = np.arange(n) % 2 == 0
    elif kind == "one_right_then_left":                 # the longest chain: the right sphere walks every left one
        left = np.arange(n) != 0
    else:
        left = rng.random(n) < 0.4
    s = np.zeros(n, mirt.abi.SPHERE)
    s["center"][:, 0] = np.where(left, 0.0, 100.0) + np.arange(n) / 64.0
    s["center"][:, 1] = rng.integers(-8, 9, n) / 16.0
    s["radius"] = np.float32(0.25)
    s["color"] = rng.integers(0, 256, (n, 4))
    return s, left


@pytest.mark.parametrize("kind", ["alternating", "one_right_then_left", "random"])
def test_partition_patterns(gpu, mirt, kind):
    s, left = pattern_scene(mirt, kind)
    ref = s.copy()
    nodes = mirt.build_bvh(ref).nodes
    # the root's plane did separate the groups: its left child holds exactly the left spheres, in order
    nl = int(left.sum())
    assert same(np.sort(ref["center"][:nl, 0]), np.sort(s["center"][left, 0]))
    exp = check_build(gpu, mirt, s, want=(ref, nodes), what=kind)
    assert exp["round"] == 0


@pytest.mark.parametrize("x", [-1.0, 1.0])
def test_all_left_and_all_right(gpu, mirt, x):
    """64 points at one place: no plane has a finite cost, the fallback plane
    0.0 on axis 0 sends all of them left (x < 0) or right, 40 times over."""
    s = np.zeros(64, mirt.abi.SPHERE)
    s["center"][:, 0] = x
    s["color"][:, 0] = np.arange(64)
    exp = check_build(gpu, mirt, s, what=str(x))
    assert exp["round"] == 0 and exp["nodes"] == 81


def test_centres_on_the_split_plane(gpu, mirt):
    """The box is [-1, 7], so the planes are the integers 0..6 exactly; centres
    on multiples of 1/2 put several spheres exactly on every plane: the strict
    < sends them right."""
    n = 64
    s = np.zeros(n, mirt.abi.SPHERE)
    s["center"][:, 0] = (np.arange(n) * 7 % 13) * 0.5
    ends = np.isin(s["center"][:, 0], [0.0, 6.0])
    s["radius"] = np.where(ends, 1.0, 0.25).astype(np.float32)
    s["color"][:, 0] = np.arange(n)
    ref = s.copy()
    nodes = mirt.build_bvh(ref).nodes
    assert nodes[0]["bmin"][0] == -1.0 and nodes[0]["bmax"][0] == 7.0
    assert (s["center"][:, 0] == 3.0).sum() >= 2
    check_build(gpu, mirt, s, want=(ref, nodes))


# ---- ties and flat axes

def quantised_scene(mirt, seed):
    """test_device_build's: coordinates and radii on eighths, few distinct
    values, one axis constant, radii including 0; n from 2..4096."""
    r = np.random.default_rng(seed)
    n = int(r.integers(2, 4097))
    span = int(r.integers(1, 33))
    s = np.zeros(n, mirt.abi.SPHERE)
    s["center"] = r.integers(-span, span + 1, (n, 3)) / 8.0
    s["center"][:, seed % 3] = r.integers(-4, 5) / 8.0
    s["radius"] = r.integers(0, 4, n) / 8.0
    s["color"] = r.integers(0, 256, (n, 4))
    return s


@pytest.mark.parametrize("group", range(3))
def test_ties_and_flat_axes(gpu, mirt, group):
    for seed in range(100 + 4 * group, 104 + 4 * group):
        check_build(gpu, mirt, quantised_scene(mirt, seed), what=str(seed))


# ---- every F gives the same bytes

SWEEP = [0, 2, 4, 16, 32, 64]


@pytest.mark.parametrize("F", SWEEP)
def test_sweep_render_1000(gpu, mirt, small, F):
    s = small["render_1000_1_pre"].copy()
    with finish_range(gpu, mirt, F):
        check_build(gpu, mirt, s, F=F, want=(small["render_1000_1_post"], small["render_1000_1_tree"]))


@pytest.fixture(scope="module")
def tree_10k(mirt):
    s = mirt.create_random_spheres(10000, 1)
    return s, mirt.build_bvh(s).nodes


@pytest.mark.parametrize("F", SWEEP)
def test_sweep_golden_10k(gpu, mirt, golden, tree_10k, F):
    g = golden["scenes"]["render_10000_1"]
    s = mirt.create_random_spheres(10000, 1)
    with finish_range(gpu, mirt, F):
        exp = check_build(gpu, mirt, s, F=F, want=tree_10k)
    assert sha(s) == g["post_sha"] and sha(tree_10k[1]) == g["tree_sha"]
    if F == 0:
        assert exp["round"] == -1 and exp["levels"] == 41
    if F == 64:
        assert exp["round"] == 8 and exp["levels"] == 9 and exp["subtrees"] == 256


@pytest.mark.parametrize("n,F", [(131072, 64), (131073, 0)])
def test_automatic_rule(gpu, mirt, n, F):
    """MIRT_OPT_BUILD_FINISH 1: F = 64 for a build of at most 131,072 spheres,
    off beyond; the same bytes either side."""
    s = mirt.create_random_spheres(n, 6)
    ref = s.copy()
    want = mirt.build_bvh(ref).nodes
    got = gpu.build_bvh(s).nodes
    assert same(s, ref) and same(got, want)
    fin = gpu.last_build_finish()
    assert fin["range"] == F and fin["moved"] == 0 and (fin["round"] >= 0) == (F > 0), fin
    assert gpu.last_build_stats()["levels"] == (fin["round"] + 1 if F else 41)


@pytest.mark.parametrize("value", [65, -1, 3000])
def test_option_values(gpu, mirt, value):
    try:
        with pytest.raises(mirt.MirtError):
            gpu.set_option(mirt.abi.OPT_BUILD_FINISH, value)
        assert gpu.get_option(mirt.abi.OPT_BUILD_FINISH) == 1
    finally:
        gpu.set_option(mirt.abi.OPT_BUILD_FINISH, 1)


# ---- the callers

def fbits(x):
    return struct.pack("<f", x)


def assert_same_layout(mirt, got, want, what=""):
    ginfo, gparts = got
    winfo, wparts = want
    for k, v in winfo.items():
        ok = fbits(ginfo[k]) == fbits(v) if isinstance(v, float) else int(ginfo[k]) == int(v)
        assert ok, f"{what}: info.{k} is {ginfo[k]!r}, the host has {v!r}"
    for name, _ in mirt.abi.LAYOUT_PARTS:
        assert gparts[name].tobytes() == wparts[name].tobytes(), f"{what}: part {name} differs"


@pytest.mark.parametrize("n", [64, 1000])
def test_build_scene(gpu, mirt, n):
    s = mirt.create_random_spheres(n, 9)
    ref = s.copy()
    nodes = mirt.build_bvh(ref).nodes
    got = gpu.build_scene(s)
    st = gpu.last_scene_build_stats()
    assert same(got, ref)
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(ref, nodes), str(n))
    exp = check_stats(gpu, nodes, n, 64, str(n))
    assert exp["round"] >= 0
    assert st["on_device"] == 1 and st["nodes"] == len(nodes) and st["levels"] == exp["levels"], st


def moved(s, sigma, seed):
    r = np.random.default_rng(seed)
    out = s.copy()
    out["center"] += r.normal(0.0, sigma, (len(s), 3)).astype(np.float32)
    out["radius"] *= r.uniform(0.5, 1.5, len(s)).astype(np.float32)
    return out


@pytest.mark.parametrize("ptr_form", [False, True])
@pytest.mark.parametrize("n", [64, 1000])
def test_update_rebuilds_through_the_finish(gpu, mirt, n, ptr_form):
    """The rebuild branch builds on spheres whose colour word is their index:
    perm and reordered are right only if the colour words ride through the
    finish with their spheres."""
    s = mirt.create_random_spheres(n, 11)
    b = mirt.build_bvh(s)
    s2 = moved(s, 3.0, n)
    tagged = s2.copy()
    tagged["color"] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    tree = mirt.build_bvh(tagged, 0, n, 0).nodes
    perm = np.ascontiguousarray(tagged["color"]).view("<u4").reshape(n).astype(np.int32)
    gpu.upload_device(s, b)
    src = s2
    if ptr_form:
        src = torch.from_numpy(np.ascontiguousarray(s2).view(np.uint8).reshape(n, 20).copy()).to("cuda:0")
    reordered, got_perm, res = gpu.update_scene(src, 0, n, 1e-9)      # any tree is past 1e-9: rebuild
    if ptr_form:
        reordered, got_perm = reordered.cpu().numpy(), got_perm.cpu().numpy()
    assert res["rebuilt"] == 1 and res["on_device"] == 1, res
    assert same(got_perm, perm)
    assert same(reordered, s2[perm])
    assert_same_layout(mirt, gpu.resident_layout(), mirt.scene_layout(s2[perm].copy(), tree), str(n))
    exp = check_stats(gpu, tree, n, 64, str(n))
    assert exp["round"] >= 0


# ---- a declined input

def test_declined_input(gpu, mirt):
    s = mirt.create_random_spheres(40, 2)
    s["radius"][17] = np.nan
    ref = s.copy()
    want = mirt.build_bvh(ref).nodes
    b = gpu.build_bvh(s)
    assert gpu.last_build_stats()["on_device"] == 0
    assert same(s, ref) and same(b.nodes, want)
    fin = gpu.last_build_finish()
    assert fin["round"] == -1 and fin["subtrees"] == 0 and fin["nodes"] == 0 and fin["moved"] == 0, fin
    exp = check_build(gpu, mirt, mirt.create_random_spheres(40, 2))
    assert exp["round"] == 0

"""The device layouts an upload derives from a scene (csrc/scene_layout.cpp),
read on the CPU through mirt_scene_layout: byte goldens taken from the commit
before the builders left render.hip (tests/golden/make_golden_layouts.py says
how), and the invariants every walk's exactness argument leans on, checked
from the flat tree alone."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_layouts", os.path.join(GOLDEN, "make_golden_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "layouts.json")) as _f:
    LAYOUTS = json.load(_f)["scenes"]


@pytest.fixture(scope="module")
def scenes(mirt, small):
    """name -> (spheres, nodes, info, parts): every layout computed once."""
    out = {}
    for name, (s, nodes) in gen.scenes(mirt, small).items():
        info, parts = mirt.scene_layout(s, nodes)
        for a in (s, nodes, *parts.values()):
            a.setflags(write=False)
        out[name] = (s, nodes, info, parts)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fbits(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------- goldens

def test_golden_covers_the_scenes(scenes):
    assert list(LAYOUTS) == list(scenes)
    assert set(gen.BUILT) <= set(scenes)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_bytes_match_parent(scenes, name):
    """Every part's bytes and every info field, floats as bits, equal what the
    parent commit's builders gave."""
    _, _, info, parts = scenes[name]
    assert gen.record(info, parts) == LAYOUTS[name]


def test_golden_flags(scenes):
    """The flags each scene was chosen for (they are in the goldens too)."""
    info = {k: v[2] for k, v in scenes.items()}
    assert info["orphan_phantom"]["encloses"] == 0
    assert info["edge_huge"]["o_bound"] == 0 and info["edge_huge"]["encloses"] == 1
    assert info["edge_tiny_far"]["o_bound"] > 0 and info["edge_offset"]["o_bound"] > 0
    assert info["single_leaf"]["wide_root"] == 0 and info["single_leaf"]["num_leaves"] == 1
    assert info["hand_falling"]["ordered"] == 0 and info["hand_falling"]["encloses"] == 1
    assert info["hand_chain70"]["ordered"] == 0 and info["hand_chain70"]["encloses"] == 1
    assert info["hand_chain300"]["ordered"] == 0
    assert info["hand_sticks_out"]["encloses"] == 0 and info["hand_nan_centre"]["encloses"] == 0
    assert info["no_tree"]["num_pnodes"] == 1 and info["no_tree"]["num_hnodes"] == 1
    assert info["empty"]["num_leaves"] == 0
    for k in ("render_1000_2", "bench_1000_1", "render_10000_1", "bench_100000_1", "cluster"):
        assert info[k]["encloses"] == 1 and info[k]["ordered"] == 1 and info[k]["o_bound"] > 0, k


# ------------------------------------------------------------- invariants

class Flat:
    """The flat tree's own facts, from the nodes alone."""

    def __init__(self, abi, s, nd, info):
        self.ns, self.nn = len(s), len(nd)
        self.sphere = nd["sphere"].astype(np.int64)
        self.skip = (nd["skip"] & abi.SKIP_MASK).astype(np.int64)
        self.empty = (nd["skip"] & abi.NODE_EMPTY) != 0
        self.leaf = self.sphere >= 0
        self.live = self.leaf & (self.sphere < self.ns) & ~self.empty
        self.live_spheres = np.sort(self.sphere[self.live])
        self.leaf_of = np.full(self.ns + 1, -1, np.int64)     # sphere -> its live flat leaf
        self.leaf_of[self.sphere[self.live]] = np.nonzero(self.live)[0]
        self.lo = nd["bmin"].astype(np.float64)
        self.hi = nd["bmax"].astype(np.float64)
        # the growth of inner slot boxes, as the upload computes it: C = (largest |coordinate| of a
        # non-empty node's box or of a sphere point) * (1 + 2^-10) + 2^-10 in double, growth 2^-19 C
        cb = float(info["c_max"])
        box = np.concatenate([nd["bmin"][~self.empty], nd["bmax"][~self.empty]]).astype(np.float64)
        box = np.abs(box[np.isfinite(box)])
        if box.size:
            cb = max(cb, float(box.max()))
        self.cb = cb * (1.0 + 2.0 ** -10) + 2.0 ** -10
        self.grow = self.cb * 2.0 ** -19 if info["o_bound"] > 0 else 0.0


@pytest.fixture(scope="module")
def flat(mirt, scenes):
    return {k: Flat(mirt.abi, scenes[k][0], scenes[k][1], scenes[k][2]) for k in gen.BUILT}


@pytest.mark.parametrize("name", gen.BUILT)
def test_bound_constants(mirt, scenes, flat, name):
    """o_bound is the float of C where the boxes nest and C stays in the fp16
    range, else 0; r_max and c_max are the spheres'."""
    s, nd, info, _ = scenes[name]
    f = flat[name]
    r = np.abs(s["radius"])
    assert fbits(info["r_max"]) == fbits(r.max()) and fbits(info["c_max"]) == fbits((np.abs(s["center"]).max(1) + r).max())
    want = np.float32(f.cb) if info["encloses"] and f.cb < 6.0e4 else np.float32(0.0)
    assert fbits(info["o_bound"]) == fbits(want)
    assert info["leaf_box_off"] == (16 * info["num_leaves"] + 255) // 256 * 256
    assert info["leaf_big"] == int(64 * info["num_hnodes"] + 48 * info["num_leaves"] > 32 << 20)


@pytest.mark.parametrize("name", gen.BUILT)
def test_dnodes_and_sphere_arrays(mirt, scenes, flat, name):
    """dnodes repeat the flat nodes with each leaf's sphere inline; inner nodes
    and the sentinel carry the quiet NaN 0x7fc00000; geo / color are the
    spheres' with the never-hit sentinel last."""
    s, nd, info, p = scenes[name]
    f = flat[name]
    d = p["dnodes"]
    for k in ("bmin", "bmax"):
        assert d[k].tobytes() == nd[k].tobytes()
    assert (d["sphere"] == nd["sphere"]).all() and (d["skip"] == nd["skip"]).all() and not d["pad"].any()
    want = np.concatenate([s["center"], s["radius"][:, None]], axis=1)
    assert bits(p["geo"][:-1]).tobytes() == bits(want).tobytes()
    assert (bits(p["geo"][-1]) == 0x7FC00000).all()
    assert p["color"][:-1].tobytes() == s["color"].tobytes() and p["color"][-1] == 0xFF000000
    idx = np.where(f.leaf, f.sphere, f.ns)
    assert bits(d["geo"]).tobytes() == bits(p["geo"][idx]).tobytes()


def _contains(f, slot_lo, slot_hi, node, grow):
    """slot boxes (float64, n x 3) contain flat nodes `node`'s boxes grown by `grow` on each face."""
    return (slot_lo <= f.lo[node] - grow).all() and (slot_hi >= f.hi[node] + grow).all()


@pytest.mark.parametrize("name", gen.BUILT)
def test_pnodes_invariants(mirt, scenes, flat, name):
    abi = mirt.abi
    s, nd, info, p = scenes[name]
    f = flat[name]
    pn = p["pnodes"]
    assert info["num_pnodes"] == len(pn) == 1 + int((~f.leaf).sum())
    assert pn["flat"][0] == 0xFFFFFFFF and pn["end"][0] == f.nn
    inner_flat = np.nonzero(~f.leaf)[0]
    assert (pn["flat"][1:] == inner_flat).all() and (pn["end"][1:] == f.skip[inner_flat]).all()
    # the walk from PNode 0
    front, leaves, seen = np.array([0]), [], 0
    while front.size:
        seen += front.size
        assert seen <= len(pn)
        ref = np.concatenate([pn["ref0"][front], pn["ref1"][front]]).astype(np.int64)
        box = np.concatenate([pn["c0"][front], pn["c1"][front]])
        some = ref != abi.P_NONE
        is_leaf = some & ((ref & abi.P_LEAF) != 0)
        is_inner = some & ~is_leaf
        sp = ref[is_leaf] & abi.P_INDEX
        assert (sp < f.ns).all()
        leaves.append(sp)
        # a leaf slot carries its flat leaf's box bit for bit
        node = f.leaf_of[sp]
        assert (node >= 0).all()
        assert bits(box[is_leaf]).tobytes() == bits(np.concatenate([nd["bmin"][node], nd["bmax"][node]], 1)).tobytes()
        # an inner slot's box contains its flat node's, grown where the scene is bounded
        q = ref[is_inner]
        assert (q > 0).all() and (q < len(pn)).all()
        b = box[is_inner].astype(np.float64)
        assert _contains(f, b[:, :3], b[:, 3:], pn["flat"][q].astype(np.int64), f.grow)
        front = q
    assert (np.sort(np.concatenate(leaves)) == f.live_spheres).all()


def _half(u16):
    return u16.astype(np.uint16).view(np.float16).astype(np.float64)


@pytest.mark.parametrize("name", gen.BUILT)
def test_hnodes_invariants(mirt, scenes, flat, name):
    abi = mirt.abi
    s, nd, info, p = scenes[name]
    f = flat[name]
    hn, hx, lg, lb = p["hnodes"], p["haux"], p["leaf_geo"], p["leaf_box"]
    assert len(hx) == len(hn) == info["num_hnodes"] and len(lg) == len(lb) == info["num_leaves"]
    assert hx["flat"][0] == 0xFFFFFFFF and hx["end"][0] == f.nn
    hflat = hx["flat"][1:].astype(np.int64)
    assert (~f.leaf[hflat]).all() and (hx["end"][1:] == f.skip[hflat]).all()
    # the leaf arrays: the sphere, and the flat leaf's exact box
    assert (lb["sphere"] >= 0).all() and (lb["sphere"] < f.ns).all() and not lb["pad"].any()
    want = np.concatenate([s["center"], s["radius"][:, None]], axis=1)[lb["sphere"]]
    assert bits(lg).tobytes() == bits(want).tobytes()
    node = f.leaf_of[lb["sphere"]]
    assert (node >= 0).all()
    assert lb["lo"].tobytes() == nd["bmin"][node].tobytes() and lb["hi"].tobytes() == nd["bmax"][node].tobytes()
    # the walk from HNode 0 (whose only slot is the root)
    assert (hn["slot"]["ref"][0, 1:] == abi.P_NONE).all()
    front, leaves, seen = np.array([0]), [], 0
    while front.size:
        seen += front.size
        assert seen <= len(hn)
        slot = hn["slot"][front]                             # n x 4
        ref = slot["ref"].astype(np.int64)
        some = ref != abi.P_NONE
        is_leaf = some & ((ref & abi.P_LEAF) != 0)
        is_inner = some & ~is_leaf
        li = ref[is_leaf] & abi.P_INDEX
        assert (li < len(lb)).all()
        leaves.append(li)
        q = ref[is_inner]
        assert (q > 0).all() and (q < len(hn)).all()
        # the flat node each slot stands for, inside the HNode's own flat segment [flat + 1, end)
        stands = np.full(ref.shape, -1, np.int64)
        stands[is_leaf] = node[li]
        stands[is_inner] = hx["flat"][q]
        seg_lo = (hx["flat"][front].astype(np.int64) + 1) & 0xFFFFFFFF
        seg_hi = hx["end"][front].astype(np.int64)
        assert ((stands >= seg_lo[:, None]) & (stands < seg_hi[:, None]))[some].all()
        # fp16 intervals, decoded exactly, contain the box (grown where the scene is bounded)
        lo, hi = _half(slot["box"] & 0xFFFF), _half(slot["box"] >> 16)
        assert _contains(f, lo[some], hi[some], stands[some], f.grow)
        front = q
    li = np.concatenate(leaves)
    assert (np.sort(li) == np.arange(len(lb))).all()          # every leaf once
    assert (np.sort(lb["sphere"]) == f.live_spheres).all()
    root = int(hn["slot"]["ref"][0, 0])
    inner_root = root != abi.P_NONE and not root & abi.P_LEAF
    assert info["wide_root"] == (root if inner_root else 0)
    if f.nn and f.leaf[0]:
        assert info["wide_root"] == 0


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_ndepth(mirt, scenes, name):
    """Node depths recomputed level by level, clamped at 255 (hand_chain300 goes past it)."""
    s, nd, info, p = scenes[name]
    f = Flat(mirt.abi, s, nd, info)
    want = np.zeros(max(f.nn, 1), np.int64)
    front = np.array([0]) if f.nn and not f.leaf[0] else np.array([], np.int64)
    while front.size:
        kids = np.concatenate([front + 1, f.skip[front + 1]])
        want[kids] = np.minimum(np.concatenate([want[front], want[front]]) + 1, 255)
        front = kids[~f.leaf[kids]]
    assert (p["ndepth"] == want).all()
    if name == "hand_chain300":
        assert want.max() == 255 and (want == 255).sum() > 40


# ----------------------------------------------------------- probe errors

def test_probe_rejects_malformed_tree(mirt):
    abi = mirt.abi
    s = mirt.create_random_spheres(3, 1)
    bad = np.array([gen._node(-1, 3), gen._node(0, 2), gen._node(7, 3)], abi.NODE)   # sphere 7 of 3
    L = mirt.load()
    rc = L.mirt_scene_layout(abi.ptr(s), 3, abi.ptr(bad), 3, 0, None, 0, None)
    assert rc == -1                                             # MIRT_E_INVALID
    assert L.mirt_last_error().decode() == "mirt_scene_layout: malformed node 2 (sphere 7, skip 3)"
    with pytest.raises(mirt.MirtError, match="mirt_scene_layout: malformed node 2"):
        mirt.scene_layout(s, bad)
    one_child = np.array([gen._node(-1, 2), gen._node(0, 2)], abi.NODE)
    assert L.mirt_scene_layout(abi.ptr(s), 3, abi.ptr(one_child), 2, 0, None, 0, None) == -1
    assert L.mirt_last_error().decode().startswith("mirt_scene_layout: ")
    assert L.mirt_scene_layout(abi.ptr(s), 3, None, 0, 99, None, 0, None) == -1      # no such part
    assert L.mirt_scene_layout(None, 3, None, 0, 0, None, 0, None) == -1             # spheres missing


def test_probe_small_cap_writes_nothing(mirt, scenes):
    abi = mirt.abi
    s, nd, info, parts = scenes["render_100_1"]
    L = mirt.load()
    for part, (name, dtype) in enumerate(abi.LAYOUT_PARTS):
        want = parts[name]
        buf = np.full(want.nbytes + 16, 0xAB, np.uint8)
        raw = abi.SceneLayoutInfo()
        args = (abi.ptr(s), len(s), abi.ptr(nd), len(nd), part)
        assert L.mirt_scene_layout(*args, abi.ptr(buf), want.nbytes - 1, C.byref(raw)) == want.nbytes
        assert (buf == 0xAB).all()
        assert raw.num_pnodes == info["num_pnodes"] and raw.leaf_box_off == info["leaf_box_off"]
        assert L.mirt_scene_layout(*args, abi.ptr(buf), want.nbytes, None) == want.nbytes
        assert buf[:want.nbytes].tobytes() == want.tobytes() and (buf[want.nbytes:] == 0xAB).all()

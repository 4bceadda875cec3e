"""The device build's finish (MIRT_OPT_BUILD_FINISH, mirt_last_build_finish)
as far as it can be seen without a GPU: the option, the struct and the entry
point are declared, exported and bound; bad arguments are MIRT_E_INVALID
before any HIP call; and the helper that derives the finish's statistics from
a host tree is pinned against the host builder on the 10k scene."""
import ctypes as C
import os
import re

import pytest

from build_finish_cases import finish_expect
from conftest import ROOT

E_INVALID = -1


def test_declared_exported_bound(mirt):
    L = mirt.load()
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bMIRT_OPT_BUILD_FINISH\s*=\s*23\b", hdr)
    assert mirt.abi.OPT_BUILD_FINISH == 23
    assert re.search(r"typedef struct mirt_build_finish_stats\s*\{\s*int32_t\s+range\s*;\s*int32_t\s+round\s*;"
                     r"\s*int32_t\s+subtrees\s*;\s*int32_t\s+nodes\s*;\s*int32_t\s+moved\s*;\s*float\s+finish_ms\s*;"
                     r"\s*\}\s*mirt_build_finish_stats\s*;", hdr)
    assert re.search(r"\bint\s+mirt_last_build_finish\s*\(\s*mirt_ctx\s*\*\s*ctx\s*,\s*mirt_build_finish_stats\s*\*"
                     r"\s*out\s*\)\s*;", hdr)
    assert hasattr(L, "mirt_last_build_finish")
    assert "mirt_last_build_finish" in {n for n, _, _ in mirt.abi.SIGNATURES}
    assert [f for f, _ in mirt.abi.BuildFinishStats._fields_] == ["range", "round", "subtrees", "nodes", "moved",
                                                                  "finish_ms"]
    assert C.sizeof(mirt.abi.BuildFinishStats) == 24
    assert C.sizeof(mirt.abi.BuildStats) == 20 and C.sizeof(mirt.abi.SceneBuildStats) == 24   # layouts kept
    assert callable(mirt.Renderer.last_build_finish)
    assert L.mirt_version().decode().startswith("mirt 0.7")


def test_null_arguments_are_invalid(mirt):
    """NULL ctx, and NULL out with a block of zero bytes standing in for a
    ctx: both are refused before the context is looked at."""
    L = mirt.load()
    st = mirt.abi.BuildFinishStats()
    assert L.mirt_last_build_finish(None, C.byref(st)) == E_INVALID
    assert b"mirt_last_build_finish" in L.mirt_last_error()
    fake = C.create_string_buffer(4096)
    assert L.mirt_last_build_finish(C.cast(fake, C.c_void_p), None) == E_INVALID
    assert b"mirt_last_build_finish" in L.mirt_last_error()
    assert bytes(fake) == bytes(4096)


@pytest.fixture(scope="module")
def tree_10k(mirt):
    s = mirt.create_random_spheres(10000, 1)
    return mirt.build_bvh(s).nodes


def test_helper_on_the_10k_scene(tree_10k, golden):
    """The values of the host builder's tree of create_random_spheres(10000, 1):
    with F = 64 the hand-off is at round 8, 256 open nodes, 29,144 nodes below;
    F = 4 hands off at round 15; F = 2 never (stuck groups of 4 spheres persist
    to depth 39), nor does F = 0."""
    assert len(tree_10k) == golden["scenes"]["render_10000_1"]["nodes"]
    assert finish_expect(tree_10k, 64, 10000) == dict(round=8, subtrees=256, nodes=29144, levels=9)
    assert finish_expect(tree_10k, 4, 10000)["round"] == 15
    assert finish_expect(tree_10k, 2, 10000) == dict(round=-1, subtrees=0, nodes=0, levels=41)
    assert finish_expect(tree_10k, 0, 10000) == dict(round=-1, subtrees=0, nodes=0, levels=41)

"""The C surface of the primary cache (MIRT_OPT_PRIMARY_CACHE,
mirt_primary_cache_stats_get / _read / _write) as far as it can be seen without
a GPU: the entry points exist, the header and abi.py agree on them and on
mirt_primary_cache_stats, option id 24 is an option and takes 0 and 1 only,
NULL arguments and a cache that is not valid are MIRT_E_INVALID before any HIP
call (on a machine without a GPU a HIP call would be MIRT_E_DEVICE), and the
camera-packet kernel's two cache forms keep the budgets of their siblings."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

E_INVALID = -1
CALLS = {"mirt_primary_cache_stats_get": 2, "mirt_primary_cache_read": 4, "mirt_primary_cache_write": 4}


def header():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def fake_ctx():
    """A block of zero bytes stands in for a context: option 0, no cache."""
    fake = C.create_string_buffer(16384)
    return fake, C.cast(fake, C.c_void_p)


def test_exported_declared_and_bound(mirt):
    L, hdr, abi = mirt.load(), header(), mirt.abi
    bound = {n: (r, a) for n, r, a in abi.SIGNATURES}
    for name, nargs in CALLS.items():
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(bound[name][1]), name
        assert bound[name][0] is C.c_int
    assert bound["mirt_primary_cache_read"][1][3] is C.c_size_t and bound["mirt_primary_cache_write"][1][3] is C.c_size_t
    # the struct, field by field in the header's order
    m = re.search(r"typedef struct mirt_primary_cache_stats\s*\{(.*?)\}\s*mirt_primary_cache_stats\s*;", hdr, re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"uint64_t": C.c_uint64, "int32_t": C.c_int32}[ctype]) for n in names.split(",")]
    S = abi.PrimaryCacheStats
    assert [(f, t) for f, t in S._fields_] == fields
    assert [f for f, _ in fields] == ["hits", "fills", "bypassed", "scene_id", "bytes", "valid", "last", "reason",
                                      "width", "rows"]
    assert C.sizeof(S) == 64
    # the enums
    enums = dict(re.findall(r"\b(MIRT_(?:OPT_PRIMARY_CACHE|PCACHE_\w+))\s*=\s*(\d+)", hdr))
    assert int(enums["MIRT_OPT_PRIMARY_CACHE"]) == 24 == abi.OPT_PRIMARY_CACHE
    assert (abi.PCACHE_BYPASS, abi.PCACHE_FILL, abi.PCACHE_HIT) == tuple(
        int(enums["MIRT_PCACHE_" + k]) for k in ("BYPASS", "FILL", "HIT"))
    for value, name in abi.PCACHE_REASON.items():
        if name:
            assert int(enums["MIRT_PCACHE_" + name]) == value, name
    for name in ("primary_cache_stats", "primary_cache_read", "primary_cache_write"):
        assert callable(getattr(mirt.Renderer, name)), name
    assert callable(mirt.MultiRenderer.primary_cache_stats)


def test_option_24_takes_zero_and_one(mirt):
    """Off is the default and setting it again holds no memory to release, so
    no HIP call; every other value, and the retired id 20, are refused."""
    L = mirt.load()
    fake, ctx = fake_ctx()
    opt = mirt.abi.OPT_PRIMARY_CACHE
    assert L.mirt_get_option(ctx, opt) == 0
    assert L.mirt_set_option(ctx, opt, 0) == 0 and L.mirt_get_option(ctx, opt) == 0
    for bad in (-1, 2, 24):
        assert L.mirt_set_option(ctx, opt, bad) == E_INVALID, bad
        assert L.mirt_get_option(ctx, opt) == 0
    assert L.mirt_set_option(ctx, 20, 0) == E_INVALID and L.mirt_set_option(ctx, 25, 0) == E_INVALID
    assert L.mirt_set_option(None, opt, 1) == E_INVALID and L.mirt_get_option(None, opt) == E_INVALID
    # on: a flag and zeroed counters, still no memory and no HIP call
    assert L.mirt_set_option(ctx, opt, 1) == 0 and L.mirt_get_option(ctx, opt) == 1
    st = mirt.abi.PrimaryCacheStats()
    assert L.mirt_primary_cache_stats_get(ctx, C.byref(st)) == 0
    assert (st.hits, st.fills, st.bypassed, st.bytes, st.valid, st.scene_id) == (0, 0, 0, 0, 0, 0)
    assert L.mirt_set_option(ctx, opt, 0) == 0 and L.mirt_get_option(ctx, opt) == 0


def test_invalid_before_any_hip_call(mirt):
    L, abi = mirt.load(), mirt.abi
    fake, ctx = fake_ctx()
    st = abi.PrimaryCacheStats()
    t, s = np.full(64, 7.5, np.float32), np.full(64, 3, np.int32)
    assert L.mirt_primary_cache_stats_get(None, C.byref(st)) == E_INVALID
    assert L.mirt_primary_cache_stats_get(ctx, None) == E_INVALID
    # with the option off: zeros, and the last frame "bypassed because off"
    assert L.mirt_primary_cache_stats_get(ctx, C.byref(st)) == 0
    assert bytes(st)[:44] == bytes(44) and (st.width, st.rows) == (0, 0)
    assert abi.PCACHE_KIND[st.last] == "bypass"
    for name in ("mirt_primary_cache_read", "mirt_primary_cache_write"):
        f = getattr(L, name)
        for what, args in [("NULL ctx", (None, abi.ptr(t), abi.ptr(s), 64)), ("NULL t", (ctx, None, abi.ptr(s), 64)),
                           ("NULL sphere", (ctx, abi.ptr(t), None, 64)),
                           ("no valid cache", (ctx, abi.ptr(t), abi.ptr(s), 64)),
                           ("no valid cache, n 0", (ctx, abi.ptr(t), abi.ptr(s), 0))]:
            assert f(*args) == E_INVALID, (name, what)
            assert L.mirt_last_error().decode().startswith(name + ":"), (name, what)
    assert bytes(fake) == bytes(16384) and (t == 7.5).all() and (s == 3).all()


def test_cache_instantiations_keep_their_siblings_budgets():
    """From the kernel metadata of `make asm`: the fill forms keep 64 VGPRs and
    carry no more scratch than their plain siblings; the cached form has no
    scratch, at most 64 VGPRs and its siblings' LDS. One cached form serves the
    bounded and the unbounded camera (there is no walk in it)."""
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asm"], check=True)
    spec = importlib.util.spec_from_file_location("check_budget", os.path.join(ROOT, "scripts", "check_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata(mod.ASM)
    PLAIN, FILL, READ = "JEEE", "JN4mirt9CacheFillEEE", "JN4mirt9CacheReadEEE"

    def one(sub):
        names = [k for k in meta if sub in k]
        assert len(names) == 1, (sub, names)
        return meta[names[0]]

    for stem in ("primary_kernelILb1ELb1ELb1E", "primary_kernelILb1ELb1ELb0E"):   # ordered: bounded / unbounded
        a, b = one(stem + PLAIN), one(stem + FILL)
        print(stem, "plain", a["next_free_vgpr"], "VGPRs", a["private_segment_fixed_size"], "B scratch; fill",
              b["next_free_vgpr"], "VGPRs", b["private_segment_fixed_size"], "B scratch")
        assert b["next_free_vgpr"] <= 64, stem
        assert b["private_segment_fixed_size"] <= a["private_segment_fixed_size"], stem
        assert b["group_segment_fixed_size"] == a["group_segment_fixed_size"], stem
    cached = [k for k in meta if READ in k]
    assert len(cached) == 1 and "primary_kernelILb1ELb1ELb0E" + READ in cached[0], cached
    c, a = meta[cached[0]], one("primary_kernelILb1ELb1ELb0E" + PLAIN)
    print("cached", c["next_free_vgpr"], "VGPRs", c["private_segment_fixed_size"], "B scratch",
          c["group_segment_fixed_size"], "B LDS")
    assert c["private_segment_fixed_size"] == 0 and c["next_free_vgpr"] <= 64
    assert c["group_segment_fixed_size"] == a["group_segment_fixed_size"]
    # the cache forms exist for the ordered camera-packet kernel only
    assert len([k for k in meta if FILL in k]) == 2 and not [k for k in meta if "render_kernel" in k and "Cache" in k]
    assert mod.check() == []

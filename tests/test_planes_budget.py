"""The frame kernels' instantiations with planes against their plain siblings,
from the metadata of the device assembly (`make asm`): storing the primary hit
may not put more of a kernel into scratch than the same kernel carries without
planes. CPU only (hipcc cross-compiles)."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the mangled template argument that marks an instantiation with planes
# (class... PLANES = mirt::Planes); its plain sibling has the empty pack "J" "E"
WITH, WITHOUT = "JN4mirt6PlanesEEE", "JEEE"
# camera-packet kernel: ordered bounded / ordered unbounded / unordered / unordered exact slab;
# tile kernel: fast / exact slab (COUNT = false)
SIBLINGS = ["primary_kernelILb1ELb1ELb1E", "primary_kernelILb1ELb1ELb0E", "primary_kernelILb1ELb0ELb0E",
            "primary_kernelILb0ELb0ELb0E", "render_kernelILb1ELb0E", "render_kernelILb0ELb0E"]


def test_plane_instantiations_carry_no_more_scratch_than_their_siblings():
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asm"], check=True)
    spec = importlib.util.spec_from_file_location("check_budget", os.path.join(ROOT, "scripts", "check_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata(mod.ASM)
    for stem in SIBLINGS:
        plain = [k for k in meta if stem + WITHOUT in k]
        planes = [k for k in meta if stem + WITH in k]
        assert len(plain) == 1 and len(planes) == 1, (stem, plain, planes)
        a, b = meta[plain[0]], meta[planes[0]]
        print(stem, "plain", a["next_free_vgpr"], "VGPRs", a["private_segment_fixed_size"], "B scratch; planes",
              b["next_free_vgpr"], "VGPRs", b["private_segment_fixed_size"], "B scratch")
        assert b["private_segment_fixed_size"] <= a["private_segment_fixed_size"], stem
        assert b["group_segment_fixed_size"] == a["group_segment_fixed_size"], stem
    # the ordered camera-packet kernels keep their 8 waves per SIMD with planes
    for stem in SIBLINGS[:2]:
        assert meta[[k for k in meta if stem + WITH in k][0]]["next_free_vgpr"] <= 64
    assert mod.check() == []

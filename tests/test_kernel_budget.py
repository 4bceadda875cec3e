"""The register budgets the bounce kernels are built to (scripts/check_budget.py):
the device assembly is compiled as `make asm` does and its metadata checked.
CPU only (hipcc cross-compiles); about a minute of compile time."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bounce_kernels_keep_their_register_budget():
    csrc = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asm"], check=True)
    spec = importlib.util.spec_from_file_location("check_budget", os.path.join(ROOT, "scripts", "check_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.check() == []

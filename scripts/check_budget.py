"""Register budgets of the frame kernels, read from the metadata of the device
assembly (`make -C cs201_sah-bvh_ray_tracer_amd/csrc asm`): several devices
in bounce_kernel exist only to keep `bounce_kernel<true, 2, false>` at 96
VGPRs without scratch under this compiler, so a compiler or source change
that brings scratch back fails here instead of passing unseen.

    python scripts/check_budget.py [cs201_sah-bvh_ray_tracer_amd/csrc/build/render-gfx950.s]
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "cs201_sah-bvh_ray_tracer_amd", "csrc", "build", "render-gfx950.s")

# kernel (substring of the mangled name) -> (max VGPRs, max scratch bytes, LDS bytes or None)
BUDGETS = {
    "bounce_kernelILb1ELi2ELb0E": (96, 0, 21760),    # the timed bounce kernel: 5 waves per SIMD, no scratch
    "bounce_kernelILb1ELi4ELb0E": (96, 32, 21760),   # the leaf-batch walk (spills by design)
}


def kernel_metadata(path):
    """mangled name -> {field: int} from the .amdhsa_kernel blocks."""
    out = {}
    text = open(path).read()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2))}
    return out


def check(path=ASM):
    meta = kernel_metadata(path)
    bad = []
    for key, (vgprs, scratch, lds) in BUDGETS.items():
        names = [n for n in meta if key in n]
        if len(names) != 1:
            bad.append(f"{key}: {len(names)} kernels match")
            continue
        k = meta[names[0]]
        got = (k["next_free_vgpr"], k["private_segment_fixed_size"], k["group_segment_fixed_size"])
        print(f"{key}: {got[0]} VGPRs, {got[1]} B scratch, {got[2]} B LDS")
        if got[0] > vgprs or got[1] > scratch or (lds is not None and got[2] != lds):
            bad.append(f"{key}: {got} exceeds the budget {(vgprs, scratch, lds)}")
    return bad


if __name__ == "__main__":
    problems = check(sys.argv[1] if len(sys.argv) > 1 else ASM)
    for p in problems:
        print("BUDGET:", p)
    sys.exit(1 if problems else 0)

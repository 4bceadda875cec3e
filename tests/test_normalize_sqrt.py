"""normalize3's length (trace.h): vec3.c:22 takes (float)sqrt((double)sq); the
kernels take the correctly rounded binary32 root instead, which is the same
number (double rounding through 53 >= 2 * 24 + 2 bits is innocuous for a square
root). On the GPU the kernels' own spelling is compared with the binary64 form
on every non-negative finite float in one launch; on the CPU numpy's two forms
on 10^7 random patterns and on every subnormal with its neighbours."""
import numpy as np
import pytest


@pytest.mark.gpu
def test_binary32_root_equals_the_binary64_form_on_every_float(gpu):
    bad, first = gpu.sqrt_form_sweep()
    assert bad == 0, f"{bad} of the 0x7f800000 non-negative finite floats differ, the least 0x{first:08x}"
    assert first == 0xFFFFFFFF


def _same(bits):
    x = bits.view(np.float32)
    direct = np.sqrt(x)
    via64 = np.sqrt(x.astype(np.float64)).astype(np.float32)
    return direct.view(np.uint32) == via64.view(np.uint32)


def test_cpu_twin_random_patterns_and_subnormals():
    rng = np.random.default_rng(22)
    bits = rng.integers(0, 0x7F800000, size=10_000_000, dtype=np.uint32)
    assert _same(bits).all()
    # zero, every subnormal, the first normals; the largest finite floats and +inf
    assert _same(np.arange(0, (1 << 23) + 4, dtype=np.uint32)).all()
    assert _same(np.arange(0x7F800000 - 4, 0x7F800000 + 1, dtype=np.uint32)).all()

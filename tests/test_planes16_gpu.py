"""The two-plane fp16 format's scale rule at its boundaries on the MI355X (split16_planes_kernel, unaligned and aligned): scale and
inv bit-equal to the CPU build's, the planes equal to the CPU build's (tests/planes16_check.py)."""
import pytest

import planes16_check as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device("cuda:0")


@pytest.mark.parametrize("K", pc.WIDTHS)
def test_kernel_scales_and_planes_equal_the_cpu_builds(gpu, K):
    L, dev, stream = gpu
    pc.check_gpu_against_cpu_build(L, dev, stream, K)

"""mms_split_planes16_cat on the MI355X (split16_cat_kernel, csrc/split16_kernels.hip): byte-equal to mms_split_planes16_group on
the materialised concatenation at every layout -- aligned float4 pieces, the seam, the tail, pitched and unaligned sources --, the
guards around every output, rows = 0, and the error paths in the CPU build's words (tests/split16_cat_check.py)."""
import pytest

import split16_cat_check as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device("cuda:0")


@pytest.mark.parametrize("rows,K0,K1", sc.CASES)
def test_kernel_equals_split_of_the_concatenation(gpu, rows, K0, K1):
    L, dev, stream = gpu
    sc.check_case(L, dev, stream, "cuda:0", rows, K0, K1)


def test_rows_zero(gpu):
    L, dev, stream = gpu
    sc.check_rows_zero(L, dev, stream, "cuda:0")


def test_abi_errors_in_the_cpu_builds_words(gpu):
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = gpu
    hip = sc.error_paths(L, dev, stream, "cuda:0")
    cpu = sc.error_paths(_lib.lib_cpu(), -1, None, "cpu")
    assert hip == cpu
    assert L.mms_split_planes16_cat(-1, 0, 1, 0, None, 1, 0, None, None, None, None, 0, 0, None, None, None, None) != 0
    assert "no CPU path" in _lib.last_error(None, L)

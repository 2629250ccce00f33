"""The weight-refresh kernels per output on the MI355X (tests/refresh_kernels_check.py): fold_planes16_kernel<true> and <false>,
fold_scales16_kernel, split16_planes_kernel<true> and <false> in per-group mode, chain_refresh16_kernel and split_planes_kernel<false>
with three groups, against float64 and, where the two builds must agree bit for bit (the output scales, l1, the bound chain), against
the CPU build.  The launch's composition alone selects the instantiation (all groups K % 4 == 0 and 16-byte aligned operands: <true>; a
K = 5 group or a buffer 4 bytes off: <false>); no dispatch override is read or set.  Gates: the module docstring of the check list, with
the HIP build's D = 8 ceil(pieces / 64) + 6 additions per term."""
import pytest

import refresh_kernels_check as rk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu():
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _lib.for_device("cuda:0")
    return L, dev, stream, "cuda"


def _cpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.lib_cpu(), -1, None, "cpu"


def test_fold_planes_aligned_set_three_arrangements(torch_cuda):
    rk.check_fold_aligned_paths(*_gpu())


def test_fold_planes_unaligned_widths(torch_cuda):
    rk.check_fold_unaligned(*_gpu())


def test_fold_planes_heads_shaped(torch_cuda):
    rk.check_fold_heads_shaped(*_gpu())


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("which", sorted(rk.FOLD_OPTIONAL))
def test_fold_planes_optional_arguments(torch_cuda, which, aligned):
    rk.check_fold_optional(*_gpu(), which, aligned)


def test_fold_planes_boundary_rows(torch_cuda):
    rk.check_fold_boundary_rows(*_gpu())


@pytest.mark.parametrize("K", [100, 388])
@pytest.mark.parametrize("mutation", ["element", "tail"])
def test_fold_gates_see_a_dropped_element_or_tail(torch_cuda, mutation, K):
    rk.check_fold_gates_see_mutations(*_gpu(), mutation, K)


def test_fold_scales(torch_cuda):
    """... and equal to the CPU build's, bit for bit"""
    got, ref = rk.check_fold_scales(*_gpu()), rk.check_fold_scales(*_cpu())
    for M in rk.SCALES_M:
        for k in ("scale1", "ysc", "yinv"):
            assert torch_cuda.equal(got[M][k].view(torch_cuda.int32), ref[M][k].view(torch_cuda.int32)), (M, k)


def test_zero_network_layer(torch_cuda):
    rk.check_zero_network_layer(*_gpu())


def test_weight_planes_per_group(torch_cuda):
    """... and l1 equal to the CPU build's bit for bit: it follows the kernel's lane order, so that every hidden activation's scale is
    the same number on both builds (test_gpu_parity relies on it)"""
    got, ref = rk.check_weight_planes(*_gpu()), rk.check_weight_planes(*_cpu())
    assert sorted(got) == sorted(ref)
    for key in got:
        assert torch_cuda.equal(got[key].view(torch_cuda.int32), ref[key].view(torch_cuda.int32)), ("l1 differs between the builds", key)


def test_chain_refresh(torch_cuda):
    """... and every launch's chain, chain_scale and chain_inv equal to the CPU build's bit for bit"""
    got, ref = rk.check_chain_refresh(*_gpu()), rk.check_chain_refresh(*_cpu())
    assert sorted(got) == sorted(ref)
    for tag in got:
        for a, b in zip(got[tag], ref[tag]):
            assert torch_cuda.equal(a.view(torch_cuda.int32), b.view(torch_cuda.int32)), ("the builds differ", tag)


def test_split_planes_group_three_groups(torch_cuda):
    rk.check_split_planes_group(*_gpu())

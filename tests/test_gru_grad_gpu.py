"""The GRU gate backward (mms_gru_gates_grad_group, csrc/gru_grad_kernels.hip) entry by entry (tests/gru_grad_check.py) on the MI355X,
against float64 per output and against the CPU build.  tests/gru_grad_check.py's docstring says which edge of the kernel each shape hits."""
import pytest

import gru_grad_check as gc

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


@pytest.mark.parametrize("H,M", gc.SHAPES)
def test_against_float64(torch_cuda, H, M):
    gc.check_against_f64(*_gpu(), H, M, layout=gc.LAYOUTS[(H // 4 + M) % 3])


def test_against_float64_32_networks(torch_cuda):
    gc.check_against_f64(*_gpu(), 36, 7, G=32, layout="agents")


def test_no_rows(torch_cuda):
    gc.check_empty(*_gpu())


def test_masks_and_null_operands(torch_cuda):
    gc.check_masks(*_gpu())


def test_rows_independent_and_deterministic(torch_cuda):
    gc.check_rows_independent(*_gpu())


def test_layouts_and_writes(torch_cuda):
    gc.check_layouts(*_gpu())


def test_contract(torch_cuda):
    gc.check_contract(*_gpu())


def test_against_cpu_build(torch_cuda):
    """Every shape on both builds, the one past the chunk cap included: the difference is at most the sum of the two per-element bounds"""
    import parity
    worst = {}
    for H, M, G in [s + (3,) for s in gc.SHAPES] + [gc.BIG + (1,)]:
        worst["H%d_M%d" % (H, M)] = gc.builds_agree(gc.check_against_f64(*_gpu(), H, M, G=G), gc.check_against_f64(*_cpu(), H, M, G=G))
    print("gpu against cpu build, worst difference / (sum of the bounds):", worst)
    parity.record("gpu/gru_grad_against_cpu_build", **worst)

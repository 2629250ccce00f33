"""The unfused GRU gate step (mms_gru_gates_group, csrc/gru_gates_kernels.hip) entry by entry (tests/gru_gates_check.py) on the MI355X,
against float64 per output and against the CPU build.  The shapes cover the kernel's edges: one item per row (H = 4), a last workgroup
that is not full, more than one workgroup along the rows and along the hidden units, 32 networks in one launch."""
import pytest

import gru_gates_check as gg

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


@pytest.mark.parametrize("H,M", gg.SHAPES)
def test_against_float64(torch_cuda, H, M):
    gg.check_against_f64(*_gpu(), H, M, layout=gg.LAYOUTS[(H // 4 + M) % 3])


def test_no_rows(torch_cuda):
    gg.check_empty(*_gpu())


def test_layouts(torch_cuda):
    gg.check_layouts(*_gpu())


def test_masks(torch_cuda):
    gg.check_masks(*_gpu())


def test_rows_independent_and_deterministic(torch_cuda):
    gg.check_rows_independent(*_gpu())


def test_contract(torch_cuda):
    gg.check_contract(*_gpu())


def test_against_cpu_build(torch_cuda):
    """Every shape on both builds: the difference is at most the sum of the two per-element bounds"""
    import parity
    worst = {}
    for H, M in gg.SHAPES:
        worst["H%d_M%d" % (H, M)] = gg.builds_agree(gg.check_against_f64(*_gpu(), H, M), gg.check_against_f64(*_cpu(), H, M))
    print("gpu against cpu build, worst difference / (sum of the bounds):", worst)
    parity.record("gpu/gru_gates_against_cpu_build", **worst)

"""The grouped GRU cell step (mms_gru_group, csrc/gru_kernels.hip: gru_group_kernel) entry by entry (tests/gru_check.py) on the MI355X,
against float64 per output and against the CPU build.  The shapes cover the kernel's edges: a partial unit tile (H = 4), 32 + 4 units,
rows under and over the 128-row tile, a last k-slice of 4 (K = 36, 100, 388), 32 networks in one launch."""
import pytest

import gru_check as gk

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


@pytest.mark.parametrize("M", [1, 7, 130])
@pytest.mark.parametrize("H", [4, 36, 64, 100, 512])
def test_against_float64(torch_cuda, H, M):
    gk.check_against_f64(*_gpu(), H, M, layout=gk.LAYOUTS[(H // 4 + M) % 3])


@pytest.mark.parametrize("K,H", [(48, 64), (36, 64), (388, 36)])
def test_input_width_differs_from_hidden(torch_cuda, K, H):
    gk.check_against_f64(*_gpu(), H, 33, K=K)


def test_thirty_two_groups(torch_cuda):
    gk.check_against_f64(*_gpu(), 36, 33, G=32, layout="agents")


def test_no_rows(torch_cuda):
    gk.check_empty(*_gpu())


def test_masks(torch_cuda):
    gk.check_masks(*_gpu())


def test_pitches(torch_cuda):
    gk.check_pitches(*_gpu())


def test_rows_independent_and_deterministic(torch_cuda):
    gk.check_rows_independent(*_gpu())


@pytest.mark.parametrize("M,N,K", [(7, 64, 388), (130, 100, 36), (33, 128, 64)])
def test_layers_blocked_summation(torch_cuda, M, N, K):
    """mms_linear_group_act with act + 16, what the recurrent route's layers ask for: the 388-wide critic rows, ragged M and N, one slice"""
    gk.check_linear_blocked(*_gpu(), M, N, K)


def test_contract(torch_cuda):
    gk.check_contract(*_gpu())


def test_against_cpu_build(torch_cuda):
    """Three shapes on both builds: the difference is at most the sum of the two per-element bounds"""
    import parity
    worst = {}
    for H, M in ((36, 7), (100, 130), (512, 33)):
        worst["H%d_M%d" % (H, M)] = gk.builds_agree(gk.check_against_f64(*_gpu(), H, M), gk.check_against_f64(*_cpu(), H, M))
    print("gpu against cpu build, worst difference / (sum of the bounds):", worst)
    parity.record("gpu/gru_against_cpu_build", **worst)

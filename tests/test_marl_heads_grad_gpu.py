"""The update's output-head entries (mms_marl_heads_fwd_group, mms_marl_heads_grad_group, csrc/marl_heads_grad_kernels.hip) entry by entry
(tests/marl_heads_grad_check.py) on the MI355X, against float64 per network and output and against the CPU build.
tests/marl_heads_grad_check.py's docstring says which edge of the kernels each shape hits."""
import pytest

import marl_heads_grad_check as hc

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


@pytest.mark.parametrize("H,M,spec", hc.SHAPES)
def test_against_float64(torch_cuda, H, M, spec):
    hc.check_against_f64(*_gpu(), H, M, spec)


def test_against_float64_32_networks(torch_cuda):
    hc.check_against_f64(*_gpu(), *hc.WIDE)


@pytest.mark.parametrize("H,M,spec", hc.SHAPES[1:] + (hc.WIDE,))
def test_every_group_equals_the_single_group_call(torch_cuda, H, M, spec):
    hc.check_groups_equal_single(*_gpu(), H, M, spec)


@pytest.mark.parametrize("H", [36, 64, 512])
def test_groups_and_rows_independent(torch_cuda, H):
    hc.check_groups_independent(*_gpu(), H)


def test_null_outputs(torch_cuda):
    hc.check_null_outputs(*_gpu())


def test_no_rows(torch_cuda):
    hc.check_empty(*_gpu())


def test_contract(torch_cuda):
    hc.check_contract(*_gpu())


def test_against_cpu_build(torch_cuda):
    import parity
    worst = {}
    for H, M, spec in hc.SHAPES:
        nets = hc.make_data(H, M, spec, 7 * H + M)
        worst["H%d_M%d" % (H, M)] = hc.builds_agree(hc.check_against_f64(*_gpu(), H, M, spec), hc.check_against_f64(*_cpu(), H, M, spec), nets)
    print("gpu against cpu build, worst difference / (sum of the two errors):", worst)
    parity.record("gpu/marl_heads_against_cpu_build", **worst)


def test_graph_replay_equals_eager(torch_cuda):
    hc.check_graph_replay()

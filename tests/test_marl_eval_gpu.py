"""mms_marl_heads_eval (csrc/marl_eval_kernels.hip) entry by entry (tests/marl_eval_check.py) on the MI355X, against float64 per network
and output, against the CPU build, and replayed from a captured graph.  tests/marl_eval_check.py's docstring says which edge of the
kernel each shape hits."""
import pytest

import marl_eval_check as mc

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


@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("H,A,M", mc.SHAPES)
def test_against_float64(torch_cuda, H, A, M, G, ln):
    mc.check_against_f64(*_gpu(), H, A, M, G=G, ln=ln)


@pytest.mark.parametrize("ln", [True, False])
def test_against_float64_32_networks(torch_cuda, ln):
    mc.check_against_f64(*_gpu(), 36, 5, 7, G=32, ln=ln)


def test_factor_forms(torch_cuda):
    mc.check_factor_forms(*_gpu())


@pytest.mark.parametrize("H,A", [(512, 8), (100, 1)])
def test_rows_independent_and_deterministic(torch_cuda, H, A):
    mc.check_rows_independent(*_gpu(), H, A)


def test_contract(torch_cuda):
    mc.check_contract(*_gpu())


def test_against_cpu_build(torch_cuda):
    import parity
    worst = {}
    for H, A, M in mc.SHAPES:
        d = mc.make_data(3, M, H, A, True, 7 * H + 3 * M + A)
        worst["H%d_A%d_M%d" % (H, A, M)] = mc.builds_agree(mc.check_against_f64(*_gpu(), H, A, M), mc.check_against_f64(*_cpu(), H, A, M), d["truth"])
    print("gpu against cpu build, worst difference / (sum of the two errors):", worst)
    parity.record("gpu/marl_eval_against_cpu_build", **worst)


def test_graph_replay_equals_eager(torch_cuda):
    mc.check_graph_replay()

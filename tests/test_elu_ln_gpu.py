"""The ELU + LayerNorm block entries (mms_elu_ln_group, mms_elu_ln_grad_group, csrc/elu_ln_kernels.hip) entry by entry
(tests/elu_ln_check.py) on the MI355X, against float64 per network and output and against the CPU build.  tests/elu_ln_check.py's
docstring says which edge of the kernels each shape hits."""
import pytest

import elu_ln_check as ec

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


@pytest.mark.parametrize("H,M", ec.SHAPES)
def test_against_float64(torch_cuda, H, M):
    ec.check_against_f64(*_gpu(), H, M)


def test_against_float64_32_networks(torch_cuda):
    ec.check_against_f64(*_gpu(), 36, 7, G=32)


def test_no_rows(torch_cuda):
    ec.check_empty(*_gpu())


def test_null_dparams(torch_cuda):
    ec.check_null_params(*_gpu())


@pytest.mark.parametrize("H", [100, 64, 512])
def test_rows_independent_and_deterministic(torch_cuda, H):
    ec.check_rows_independent(*_gpu(), H)


def test_contract(torch_cuda):
    ec.check_contract(*_gpu())


def test_against_cpu_build(torch_cuda):
    """Every shape on both builds, the one past the chunk cap included (its float64 gate on the HIP build is this test's)"""
    import parity
    worst = {}
    for H, M, G in [s + (3,) for s in ec.SHAPES] + [ec.BIG + (1,)]:
        truth = ec.closed_form(ec.make_data(G, M, H, 7 * H + M))
        norms = {k: [float(truth[k][g].norm()) for g in range(G)] for k in ec.OUTS}
        worst["H%d_M%d" % (H, M)] = ec.builds_agree(ec.check_against_f64(*_gpu(), H, M, G=G), ec.check_against_f64(*_cpu(), H, M, G=G), norms)
    print("gpu against cpu build, worst difference / (sum of the two errors):", worst)
    parity.record("gpu/elu_ln_against_cpu_build", **worst)


def test_graph_replay_equals_eager(torch_cuda):
    ec.check_graph_replay()

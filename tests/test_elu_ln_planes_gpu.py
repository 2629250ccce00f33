"""mms_elu_ln_planes16_group (csrc/elu_ln_kernels.hip: elu_ln_planes_kernel) entry by entry (tests/elu_ln_planes_check.py) on the MI355X:
the bits of mms_elu_ln_group and the bytes of mms_split_planes16_group on the same device."""
import pytest

import elu_ln_check as ec
import elu_ln_planes_check as pc

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


@pytest.mark.parametrize("H,M", ec.SHAPES)
def test_equals_the_composition(torch_cuda, H, M):
    pc.check_composition(*_gpu(), H, M)


def test_equals_the_composition_at_the_widest_row(torch_cuda):
    pc.check_composition(*_gpu(), *ec.BIG, G=1)


def test_equals_the_composition_32_networks(torch_cuda):
    pc.check_composition(*_gpu(), 36, 7, G=32)


def test_zero_rows_and_a_bound_at_a_power_of_two(torch_cuda):
    pc.check_adversarial_rows(*_gpu())


@pytest.mark.parametrize("H", [100, 64, 512])
def test_rows_independent_and_deterministic(torch_cuda, H):
    pc.check_rows_independent(*_gpu(), H)


def test_no_rows_and_null_scale_entries(torch_cuda):
    pc.check_empty_and_null_entries(*_gpu())


def test_contract(torch_cuda):
    pc.check_contract(*_gpu())


def test_graph_replay_equals_eager(torch_cuda):
    pc.check_graph_replay()

"""The recurrent policies' plane route (GroupedPolicyInference(..., rnn_format="f16x2"); tests/marl_rnn16_check.py) on the MI355X: the
base blocks and both GRU products through split16_kernels.hip's layer kernel with fp32 output, the gates through
gru_gates_kernels.hip, the states read from and written into their slots."""
import pytest

import marl_rnn16_check as rk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return "cuda"


@pytest.mark.parametrize("M,hidden,recurrent_N", rk.SHAPES)
def test_three_agents_against_float64(cuda, M, hidden, recurrent_N):
    rk.check_three_agents(cuda, M, hidden, recurrent_N)


def test_fallback_is_the_fp32_route(cuda):
    rk.check_fallback(cuda)


def test_fallback_on_the_reference_fixture(cuda):
    rk.check_fallback_fixture(cuda)


def test_feed_forward_group_ignores_the_keyword(cuda):
    rk.check_feed_forward_ignores_the_keyword(cuda)


def test_masks_behind_the_product(cuda):
    rk.check_masks(cuda)


def test_collect_into_writes_the_next_slot_in_place(cuda):
    rk.check_collect_into(cuda)


def test_refresh_after_an_optimizer_step(cuda):
    rk.check_refresh(cuda)


def test_get_values_is_get_actions_values(cuda):
    rk.check_get_values(cuda)


def test_unknown_format_is_refused(cuda):
    rk.check_value_error(cuda)

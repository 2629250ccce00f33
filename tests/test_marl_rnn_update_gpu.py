"""The MAPPO / HAPPO trainers' opt-in `fused_rnn_update` route (tests/marl_rnn_update_check.py) on the MI355X: gru_sequence through
mms_gru_gates_group and mms_gru_gates_grad_group of the HIP build, against the default route on the same device."""
import pytest

import marl_rnn_update_check as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return "cuda"


@pytest.mark.parametrize("algo", ["MAPPO", "HAPPO"])
def test_update_against_float64(cuda, algo):
    uc.check_update(cuda, algo)


def test_update_actor_false_leaves_the_actor_without_gradients(cuda):
    uc.check_actor_frozen(cuda)


def test_naive_recurrent_generator(cuda):
    uc.check_naive_generator(cuda)


def test_default_route_is_unchanged(cuda):
    uc.check_default_unchanged(cuda)


def test_refusals(cuda):
    uc.check_refusals(cuda)

"""The MAPPO / HAPPO trainers' opt-in `fused_rnn_update` route (tests/marl_rnn_update_check.py) on torch device "cpu": gru_sequence
through the CPU build.  tests/test_marl_rnn_update_gpu.py runs the same list on the HIP build."""
import pytest

import marl_rnn_update_check as uc


@pytest.mark.parametrize("algo", ["MAPPO", "HAPPO"])
def test_update_against_float64(algo):
    uc.check_update("cpu", algo)


def test_update_actor_false_leaves_the_actor_without_gradients():
    uc.check_actor_frozen("cpu")


def test_naive_recurrent_generator():
    uc.check_naive_generator("cpu")


def test_default_route_is_unchanged():
    uc.check_default_unchanged("cpu")


def test_refusals():
    uc.check_refusals("cpu")

"""Recurrent MAPPO / HAPPO policies (tests/marl_rnn_check.py) on the MI355X: GroupedPolicyInference through the HIP build (mms_gru_group's
gru_group_kernel between mms_layernorm_group and mms_marl_heads_act; M = 128 with hidden 128 through the LayerNorm-fold layers), the
trainers' recurrent updates on the device."""
import pytest

import marl_rnn_check as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return "cuda"


def test_fixture_through_the_grouped_path(cuda):
    rc.check_fixture_grouped(cuda)


@pytest.mark.parametrize("M", [7, 128])
@pytest.mark.parametrize("recurrent_N", [1, 2])
@pytest.mark.parametrize("hidden", [64, 128])
def test_three_agents_against_float64(cuda, hidden, recurrent_N, M):
    rc.check_three_agents(cuda, hidden, recurrent_N, M)


@pytest.mark.parametrize("M,hidden,rnn_format", [(24, 64, "fp32"), (128, 128, "fp32"), (128, 128, "f16x2")])
def test_get_values_repeats_get_actions(cuda, M, hidden, rnn_format):
    rc.check_get_values_repeats_get_actions(cuda, M, hidden, rnn_format)


def test_collect_steps_with_a_done_env(cuda):
    rc.check_collect(cuda)


def test_collect_into_writes_the_next_slot_in_place(cuda):
    rc.check_collect_into(cuda)


def test_insert_step_zeroes_done_envs(cuda):
    rc.check_insert_step_zeroes_done_envs(cuda)


@pytest.mark.parametrize("algo", ["MAPPO", "HAPPO"])
def test_trainer_update(cuda, algo):
    rc.check_trainer_update(cuda, algo)


def test_update_forward_is_the_fixture(cuda):
    rc.check_update_forward_is_the_fixture(cuda)


@pytest.mark.parametrize("algo,naive", [("MAPPO", False), ("MAPPO", True), ("HAPPO", True)])
def test_train_runs(cuda, algo, naive):
    rc.check_train_runs(cuda, algo, naive)

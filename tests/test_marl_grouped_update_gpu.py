"""The lockstep MAPPO update (trainer.MAPPO.train_group, over mms_marl_ppo_loss_group) and Runner's `grouped_update` on the MI355X:
both routes from equal states end in the same bits (marl_grouped_update_check.py) under every normaliser, both mask flags, FusedAdam and
torch.optim.Adam, both block_products, update_actor=False, 3, 17 and 33 agents; the entries' call counts; the refusals; Runner.train()
with the key on and off, shared_buffers and fused_factor on and off."""
import pytest

import marl_grouped_update_check as gu

DEV = "cuda:0"

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


CASES = {
    "popart": dict(),
    "valuenorm": dict(use_popart=False, use_valuenorm=True),
    "no_normaliser": dict(use_popart=False, use_valuenorm=False),
    "both_mask_flags": dict(use_policy_active_masks=True, use_value_active_masks=True),
    "f16x2": dict(block_products="f16x2"),
    "no_clip": dict(use_max_grad_norm=False),
}


# every case with FusedAdam; torch.optim.Adam with and without a clip and without a normaliser (the steps differ there, nothing else)
PAIRS = [(case, True) for case in sorted(CASES)] + [("popart", False), ("no_clip", False), ("no_normaliser", False)]


@pytest.mark.parametrize("case,fused_adam", PAIRS)
def test_group_equals_the_sequential_loop(torch_cuda, case, fused_adam):
    gu.routes(DEV, 3, gu.config(**CASES[case]), fused_adam=fused_adam)


def test_update_actor_false(torch_cuda):
    gu.routes(DEV, 3, gu.config(), update_actor=False)
    gu.routes(DEV, 2, gu.config(hidden=8, T=4, N=8), update_actor=False, fused_adam=False)


def test_seventeen_agents_cross_the_chunk_of_mlp_base(torch_cuda):
    gu.routes(DEV, 17, gu.config(hidden=8, T=4, N=8))


def test_thirty_three_agents_cross_the_chunk_of_the_loss_entry(torch_cuda):
    gu.routes(DEV, 33, gu.config(hidden=4, T=2, N=8), order=list(range(32, -1, -1)))


def test_elu_ln_calls_do_not_grow_with_the_agents(torch_cuda):
    gu.check_elu_ln_count_does_not_grow(DEV)


def test_refusals_change_nothing(torch_cuda):
    gu.check_refusals(DEV)


@pytest.mark.parametrize("shared,fused_factor", [(False, True), (True, True), (False, False), (True, False)])
def test_runner_train_equals_the_agent_loop(torch_cuda, shared, fused_factor):
    gu.check_runner("cuda", shared, fused_factor)

"""heads.update_heads and the MAPPO / HAPPO trainers' `fused_head_update` route (tests/marl_head_update_check.py) on the MI355X: the HIP
build of mms_marl_heads_fwd_group / mms_marl_heads_grad_group (csrc/marl_heads_grad_kernels.hip).  tests/test_marl_head_update.py runs
the same list on the CPU build."""
import pytest

import marl_block_update_check as bu
import marl_head_update_check as hu

DEVICE = "cuda:0"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


@pytest.mark.parametrize("hidden", [36, 128])
def test_update_heads_matches_the_modules(torch_cuda, hidden):
    hu.check_update_heads(DEVICE, hidden)


def test_33_agents_run_in_chunks(torch_cuda):
    hu.check_chunks(DEVICE)


def test_a_network_without_a_gradient_gets_none(torch_cuda):
    hu.check_no_grad_networks(DEVICE)


def test_check_heads_refuses_what_the_entries_do_not_take(torch_cuda):
    hu.check_refusals(DEVICE)


@pytest.mark.parametrize("algo,route,hidden", bu.UPDATE_CASES)
def test_ppo_update_gradients(torch_cuda, algo, route, hidden):
    hu.check_update(DEVICE, algo, route, hidden)


@pytest.mark.parametrize("route", bu.ROUTES)
def test_update_actor_false_leaves_the_actor(torch_cuda, route):
    hu.check_actor_frozen(DEVICE, route)


@pytest.mark.parametrize("G,hidden", [(3, 128), (17, 8)])
def test_train_group_equals_the_agent_loop(torch_cuda, G, hidden):
    hu.check_group_routes(DEVICE, G, hidden)


def test_train_group_without_the_actor(torch_cuda):
    hu.check_group_routes(DEVICE, 2, 8, update_actor=False)


def test_heads_calls_do_not_grow_with_the_agents(torch_cuda):
    hu.check_call_counts(DEVICE)

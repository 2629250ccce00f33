"""The PPO and TRPO learners on the MI355X (onpolicy_learner_check.py): the opt-in routes -- mms_ppo_loss and mms_param_step under PPO;
mms_trpo_heads, mms_mlp_grad, mms_mlp_grad_rop and mms_param_step under TRPO -- against the default route and a float64 replay, at the
fixture's size and at 256 rows per minibatch over (128, 128); the direct curvature product against the float64 double backward; the
contract; run(2) on an engine; and a graph capture of the fused PPO minibatch up to the schedule's read."""
import pytest

import onpolicy_learner_check as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


@pytest.mark.parametrize("size", ["small", "tiles"])
@pytest.mark.parametrize("algo", ["ppo", "trpo"])
def test_opt_in_routes_against_the_default_route(torch_cuda, algo, size):
    oc.route_errors(algo, "cuda:0", size=size)


def test_trpo_routes_when_the_line_search_backtracks(torch_cuda):
    oc.route_errors("trpo", "cuda:0", step_fraction=1.0, max_kl=0.05, accept_ratio=0.9)


def test_direct_curvature_product(torch_cuda):
    oc.check_direct_product("cuda:0")
    oc.check_direct_product("cuda:0", rows=1000, hidden=(256, 128), seed=1)


@pytest.mark.parametrize("algo", ["ppo", "trpo"])
def test_contract(torch_cuda, algo):
    oc.check_contract(algo, "cuda:0")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("algo", ["ppo", "trpo"])
def test_run(torch_cuda, algo, fused):
    oc.check_run(algo, "cuda", fused)


def test_fused_ppo_minibatch_in_a_graph(torch_cuda):
    oc.check_graph_capture()

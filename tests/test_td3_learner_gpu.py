"""The TD3 and DDPG learners on the MI355X: td3_learner_check.py's checks on the HIP build -- the fused route (mms_det_heads_act /
mms_det_heads_grad, mms_q_heads_backup, mms_q_heads_loss, mms_param_step) against the default route and a float64 replay, one fused
step captured in a graph, the contract, and run(2) on a small engine on both routes."""
import pytest

import td3_learner_check as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")


@pytest.mark.parametrize("algo,freeze,skip", [("td3", False, False), ("td3", True, False), ("td3", False, True), ("ddpg", False, False), ("ddpg", True, False)])
def test_fused_route_against_default_route(algo, freeze, skip):
    tc.route_errors(algo, "cuda:0", freeze=freeze, skip=skip)


@pytest.mark.parametrize("algo", ["td3", "ddpg"])
def test_graph_capture_of_a_fused_step(algo):
    tc.check_graph_capture(algo)


@pytest.mark.parametrize("algo", ["td3", "ddpg"])
def test_contract(algo):
    tc.check_contract(algo, "cuda:0")


@pytest.mark.parametrize("algo", ["td3", "ddpg"])
@pytest.mark.parametrize("fused", [False, True])
def test_run_on_a_small_engine(algo, fused):
    tc.check_run(algo, "cuda", fused)

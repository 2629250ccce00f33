"""The TD3 and DDPG learners (algorithms/rl/td3/td3.py, ddpg/ddpg.py) without a GPU: the default route against the reference's own
update (tests/golden/td3_update.npz, ddpg_update.npz), the fused route against the default route through the CPU build, the learners'
contract and run(2) on a small CPU engine.  The checks are td3_learner_check.py's, shared with test_td3_learner_gpu.py."""
import pytest

import td3_learner_check as tc


@pytest.mark.parametrize("algo,variant", tc.VARIANTS)
def test_default_route_is_the_references_update(algo, variant):
    tc.fixture_update(algo, variant)


@pytest.mark.parametrize("algo,freeze,skip", [("td3", False, False), ("td3", True, False), ("td3", False, True), ("ddpg", False, False), ("ddpg", True, False)])
def test_fused_route_against_default_route(algo, freeze, skip):
    tc.route_errors(algo, "cpu", freeze=freeze, skip=skip)


@pytest.mark.parametrize("algo", ["td3", "ddpg"])
def test_contract(algo):
    tc.check_contract(algo, "cpu")


@pytest.mark.parametrize("algo", ["td3", "ddpg"])
@pytest.mark.parametrize("fused", [False, True])
def test_run_on_a_small_engine(algo, fused):
    tc.check_run(algo, "cpu", fused)

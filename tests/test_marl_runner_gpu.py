"""The on-policy MARL drop-in and GroupedPolicyInference.evaluate_actions on the MI355X (tests/marl_runner_check.py): the list of
tests/test_marl_runner.py on the HIP build, and the grouping invariance on the two-plane fp16 route as well."""
import pytest

import marl_runner_check as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def test_evaluate_actions_against_the_fixture(torch_cuda):
    rc.check_evaluate_against_fixture("cuda:0")


def test_single_agent_call_equals_grouped_call(torch_cuda):
    rc.check_grouping_invariance("cuda:0")


def test_single_agent_call_equals_grouped_call_on_the_plane_route(torch_cuda):
    rc.check_grouping_invariance("cuda:0", M=256, H=128, n=2, route="f16x2")


def test_more_than_sixteen_agents(torch_cuda):
    rc.check_chunks("cuda:0")


def test_eval(torch_cuda):
    rc.check_eval("cuda:0")


def test_refresh_after_an_optimizer_step(torch_cuda):
    rc.check_refresh("cuda:0")


def test_factor_loop_against_float64(torch_cuda, monkeypatch):
    rc.check_factor_loop("cuda:0", monkeypatch)


def test_noop_update_leaves_the_factor_at_one(torch_cuda):
    rc.check_noop_update("cuda:0")


def test_route_call_counts(torch_cuda, monkeypatch):
    from massive_marl_benchmark_amd import _lib
    rc.check_call_counts("cuda:0", _lib.lib(), monkeypatch)


def test_fused_and_module_routes_agree(torch_cuda):
    rc.check_routes_agree("cuda:0")


@pytest.mark.parametrize("algo,shared", [("mappo", False), ("happo", False), ("hatrpo", False), ("happo", True)])
def test_end_to_end(torch_cuda, algo, shared):
    rc.check_end_to_end("cuda", algo, shared)

"""blocks.mlp_base and the MAPPO / HAPPO trainers' opt-in `fused_block_update` route (tests/marl_block_update_check.py) on torch device
"cpu": mms_elu_ln_group and mms_elu_ln_grad_group of the CPU build.  tests/test_marl_block_update_gpu.py runs the same list on the HIP
build."""
import pytest

import marl_block_update_check as bc


@pytest.mark.parametrize("hidden", [32, 36])
def test_mlp_base_against_float64(hidden):
    bc.check_mlp_base("cpu", hidden)


@pytest.mark.parametrize("algo,route,hidden", bc.UPDATE_CASES)
def test_update_against_float64(algo, route, hidden):
    bc.check_update("cpu", algo, route, hidden)


@pytest.mark.parametrize("route", bc.ROUTES)
def test_update_actor_false_leaves_the_actor_untouched(route):
    bc.check_actor_frozen("cpu", route)


def test_default_route_is_unchanged_and_the_key_calls_mlp_base():
    bc.check_default_unchanged("cpu")


def test_refusals():
    bc.check_refusals("cpu")

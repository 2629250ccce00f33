"""blocks.mlp_base and the MAPPO / HAPPO trainers' opt-in `fused_block_update` route (tests/marl_block_update_check.py) on the MI355X:
mms_elu_ln_group and mms_elu_ln_grad_group of the HIP build, against the default route on the same device."""
import pytest

import marl_block_update_check as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return "cuda"


@pytest.mark.parametrize("hidden", [32, 36])
def test_mlp_base_against_float64(cuda, hidden):
    bc.check_mlp_base(cuda, hidden)


@pytest.mark.parametrize("algo,route,hidden", bc.UPDATE_CASES)
def test_update_against_float64(cuda, algo, route, hidden):
    bc.check_update(cuda, algo, route, hidden)


@pytest.mark.parametrize("route", bc.ROUTES)
def test_update_actor_false_leaves_the_actor_untouched(cuda, route):
    bc.check_actor_frozen(cuda, route)


def test_default_route_is_unchanged_and_the_key_calls_mlp_base(cuda):
    bc.check_default_unchanged(cuda)


def test_refusals(cuda):
    bc.check_refusals(cuda)

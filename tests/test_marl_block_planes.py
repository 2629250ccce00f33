"""blocks.mlp_base(products="f16x2") and the MAPPO / HAPPO trainers' `block_products` key (tests/marl_block_planes_check.py) on torch
"cpu": the CPU build of mms_weight_planes16_group, mms_split_planes16_group, mms_linear_group_act_split16 and
mms_elu_ln_planes16_group.  tests/test_marl_block_planes_gpu.py runs the same list on the HIP build."""
import pytest

import marl_block_planes_check as bc


@pytest.mark.parametrize("M", [128, 256])
def test_mlp_base_on_the_plane_products(M):
    bc.check_mlp_base("cpu", M)


def test_library_products_are_the_default_call():
    bc.check_default_path("cpu")


@pytest.mark.parametrize("algo,route", bc.UPDATE_CASES)
def test_ppo_update_on_the_plane_products(algo, route):
    bc.check_update("cpu", algo, route)


def test_refusals():
    bc.check_refusals("cpu")

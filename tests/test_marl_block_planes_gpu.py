"""blocks.mlp_base(products="f16x2") and the MAPPO / HAPPO trainers' `block_products` key (tests/marl_block_planes_check.py) on the
MI355X: the HIP build's plane products and mms_elu_ln_planes16_group against the default torch route on the same device."""
import pytest

import marl_block_planes_check as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


@pytest.mark.parametrize("M", [128, 256])
def test_mlp_base_on_the_plane_products(torch_cuda, M):
    bc.check_mlp_base("cuda", M)


def test_library_products_are_the_default_call(torch_cuda):
    bc.check_default_path("cuda")


@pytest.mark.parametrize("algo,route", bc.UPDATE_CASES)
def test_ppo_update_on_the_plane_products(torch_cuda, algo, route):
    bc.check_update("cuda", algo, route)


def test_refusals(torch_cuda):
    bc.check_refusals("cuda")

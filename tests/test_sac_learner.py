"""The SAC learner (algorithms/rl/sac/sac.py), its loss heads (loss.py, MLPActorCritic.q_loss / pi_loss) and the fixture of the
reference's own update (tests/golden/sac_update.npz) without a GPU: everything on torch's "cpu" device through the CPU build.  The
checks are sac_learner_check.py's, shared with test_sac_learner_gpu.py."""
import pytest
import torch

import sac_learner_check as lc

CPU = torch.device("cpu")


@pytest.mark.parametrize("freeze", [False, True])
def test_default_route_is_the_references_update(freeze):
    lc.fixture_update(freeze)


@pytest.fixture(scope="module")
def head_ratios():
    ratios = {H: lc.loss_head_ratios(CPU, H) for H in (64, 128)}
    lc.record_head_ratios("cpu", ratios)
    return ratios


@pytest.mark.parametrize("head", ["q_loss", "pi_loss head"])
@pytest.mark.parametrize("H", [64, 128])
def test_loss_heads_against_float64(head_ratios, H, head):
    """Fused error against float64 at most 2 x the fp32 torch expression's, per tensor (the loss, every parameter and input gradient)."""
    lc.assert_head_rule({H: head_ratios[H]}, head)


def test_loss_heads_fallback_and_frozen_critics():
    lc.check_fallback(CPU)


@pytest.mark.parametrize("freeze", [False, True])
def test_fused_route_against_default_route(freeze):
    lc.route_errors(CPU, freeze)


def test_learner_contract():
    lc.check_contract(CPU)


@pytest.mark.parametrize("fused", [False, True])
def test_run_on_a_small_engine(fused):
    lc.check_run("cpu", fused)

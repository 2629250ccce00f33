"""The SAC learner and its loss heads on the MI355X: q_loss / pi_loss through mms_q_heads_loss against float64, the fused route
against the default route on the same draws, one fused minibatch captured in a graph (no host read inside it), the learner's
contract and run(2) on a small engine.  The checks are sac_learner_check.py's, shared with test_sac_learner.py."""
import pytest

import sac_learner_check as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def head_ratios(dev):
    ratios = {H: lc.loss_head_ratios(dev, H) for H in (64, 128)}
    lc.record_head_ratios("hip", ratios)
    return ratios


@pytest.mark.parametrize("head", ["q_loss", "pi_loss head"])
@pytest.mark.parametrize("H", [64, 128])
def test_loss_heads_against_float64(head_ratios, H, head):
    """Fused error against float64 at most 2 x the fp32 torch expression's, per tensor (the loss, every parameter and input gradient)."""
    lc.assert_head_rule({H: head_ratios[H]}, head)


def test_loss_heads_fallback_and_frozen_critics(dev):
    lc.check_fallback(dev)


@pytest.mark.parametrize("freeze", [False, True])
def test_fused_route_against_default_route(dev, freeze):
    lc.route_errors(dev, freeze)


def test_fused_minibatch_is_graph_capturable(dev):
    lc.check_graph_capture()


def test_learner_contract(dev):
    lc.check_contract(dev)


@pytest.mark.parametrize("fused", [False, True])
def test_run_on_a_small_engine(dev, fused):
    lc.check_run("cuda", fused)

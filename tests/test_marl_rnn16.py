"""The recurrent policies' plane route (GroupedPolicyInference(..., rnn_format="f16x2"); tests/marl_rnn16_check.py) on the CPU build of
the C ABI.  tests/test_marl_rnn16_gpu.py runs the same list on the HIP build."""
import pytest

import marl_rnn16_check as rk


@pytest.mark.parametrize("M,hidden,recurrent_N", rk.SHAPES)
def test_three_agents_against_float64(M, hidden, recurrent_N):
    rk.check_three_agents("cpu", M, hidden, recurrent_N)


def test_fallback_is_the_fp32_route():
    rk.check_fallback("cpu")


def test_fallback_on_the_reference_fixture():
    rk.check_fallback_fixture("cpu")


def test_feed_forward_group_ignores_the_keyword():
    rk.check_feed_forward_ignores_the_keyword("cpu")


def test_masks_behind_the_product():
    rk.check_masks("cpu")


def test_collect_into_writes_the_next_slot_in_place():
    rk.check_collect_into("cpu")


def test_refresh_after_an_optimizer_step():
    rk.check_refresh("cpu")


def test_get_values_is_get_actions_values():
    rk.check_get_values("cpu")


def test_unknown_format_is_refused():
    rk.check_value_error("cpu")

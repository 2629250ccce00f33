"""gru_sequence (algorithms/marl/rnn_seq.py) against RNNLayer (tests/rnn_seq_check.py) on torch device "cpu": the CPU build of
mms_gru_gates_group and mms_gru_gates_grad_group.  tests/test_rnn_seq_gpu.py runs the same list on the HIP build."""
import pytest

import rnn_seq_check as rs


@pytest.mark.parametrize("T,N,H,R,kind", rs.CASES)
def test_against_rnn_layer_in_float64(T, N, H, R, kind):
    rs.check_against_f64("cpu", T, N, H, R, kind)


def test_grouped_call_equals_single_calls():
    rs.check_grouped_equals_single("cpu")


def test_backward_is_deterministic():
    rs.check_deterministic("cpu")


def test_refusals():
    rs.check_refusals("cpu")

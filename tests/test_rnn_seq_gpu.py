"""gru_sequence (algorithms/marl/rnn_seq.py) against RNNLayer (tests/rnn_seq_check.py) on the MI355X: mms_gru_gates_group forward,
mms_gru_gates_grad_group (csrc/gru_grad_kernels.hip) backward, and no host synchronisation in either."""
import pytest

import rnn_seq_check as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return "cuda"


@pytest.mark.parametrize("T,N,H,R,kind", rs.CASES)
def test_against_rnn_layer_in_float64(cuda, T, N, H, R, kind):
    rs.check_against_f64(cuda, T, N, H, R, kind)


def test_grouped_call_equals_single_calls(cuda):
    rs.check_grouped_equals_single(cuda)


def test_backward_is_deterministic(cuda):
    rs.check_deterministic(cuda)


def test_no_host_synchronisation(cuda):
    rs.check_no_host_sync(cuda)


def test_refusals(cuda):
    rs.check_refusals(cuda)

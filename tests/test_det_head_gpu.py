"""mms_det_heads_act / mms_det_heads_grad (csrc/maddpg_kernels.hip, csrc/det_head_kernels.hip) and the `fused_grad=True` path of DDPG's /
TD3's modules on the MI355X: det_head_check.py's checks on the HIP build -- every forward case against the grouped entry's bits and
against float64, the backward on its three load paths against the CPU build's bits, the bias sums, the error paths, and the modules on
the device against float64 autograd."""
import pytest

import det_head_check as dc
import sac_learner_check as sl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return dc.build("cuda:0")


def test_forward(gpu):
    ratios = dc.forward_ratios(gpu)
    dc.record_ratios("cuda", {"forward": ratios})
    sl.assert_head_rule(ratios, "forward")


def test_backward(gpu):
    dc.record_ratios("cuda", {"backward": dc.backward_ratios(gpu)})
    for N, A in dc.grad_cases():
        assert dc.ws_bytes(gpu, N, A) % 256 == 0 and dc.ws_bytes(gpu, N, A) >= (2 if N == dc.two_partials(A) else 1) * A * 8


def test_backward_against_cpu_build(gpu):
    """dy has the same bits in both builds; each build's dbias is one rounding of its own double sum, so the two differ by at most one
    fp32 ulp of the sum's magnitude bound."""
    import torch
    cpu = dc.build("cpu")
    for N, A in dc.grad_cases():
        t, g = dc.grad_problem(N, A, gpu[3])
        d_gpu, b_gpu = dc.grad(gpu, t, g)
        d_cpu, b_cpu = dc.grad(cpu, t.cpu(), g.cpu())
        assert torch.equal(d_gpu.cpu(), d_cpu), (N, A)
        dc.check_bias(b_gpu, d_cpu, (N, A))


def test_abi_errors(gpu):
    dc.check_abi_errors(gpu)


def test_module_gradients_against_float64(gpu):
    ratios = {H: dc.module_gradient_ratios(gpu, H) for H in (64, 128)}
    dc.record_ratios("cuda", {"module": ratios})
    sl.assert_head_rule(ratios, "pi_loss")


def test_module_semantics(gpu):
    dc.check_module_semantics(gpu)


def test_fallback_is_the_torch_path(gpu):
    dc.check_fallback("cuda:0")


def test_default_path_is_unchanged(gpu):
    """fused_grad=False is the code as it was: the same launches, the same bits as an actor built without the keyword, and torch's
    generator is where the reference's constructor leaves it."""
    import torch
    from massive_marl_benchmark_amd.algorithms.rl.td3.module import MLPActorCritic
    outs = []
    for kw in ({}, {"fused_grad": False}):
        torch.manual_seed(8)
        ac = dc.make_ac(MLPActorCritic, 32, 6, (128, 128), "cuda:0", **kw)
        o = torch.randn(500, 32, device="cuda")
        outs.append((ac.pi(o).detach(), ac.act(o), ac.act(o, deterministic=False), torch.rand(3)))
        assert ac.pi._counters is None
    assert all(torch.equal(p, q) for p, q in zip(*outs))

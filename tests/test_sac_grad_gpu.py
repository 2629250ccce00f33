"""The backward of SAC's fused head (mms_sac_heads_grad, csrc/sac_grad_kernels.hip) and the actor's `fused_grad=True` path on the
MI355X: sac_grad_check.py's checks on the HIP build -- the kernels against float64 per element, the bias sums, row independence,
determinism, the scalar path, the grid-stride wrap, the error paths -- the kernel against the CPU build, and the module on the
device against float64 autograd."""
import numpy as np
import pytest

import sac_grad_check as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return gc.build("cuda:0")


@pytest.mark.parametrize("N,H,A,limit,det", gc.ENTRY_SHAPES)
def test_kernel_against_float64(gpu, N, H, A, limit, det):
    gc.check_entry(gpu, N, H, A, limit, det)


def test_structure(gpu):
    gc.check_structure(gpu)


def test_abi_errors(gpu):
    gc.check_abi_errors(gpu)
    assert gc.ws_bytes(gpu, 70001, 6) >= 417 * 12 * 8 and gc.ws_bytes(gpu, 70001, 6) % 256 == 0


def test_kernel_against_cpu_build(gpu):
    """The same saved tensors through both builds: each is within the gate of float64, so they are within two gates of each other;
    the masks agree exactly."""
    import torch
    N, H, A, limit, det = gc.ENTRY_SHAPES[0]
    o = gc.forward(gpu, N, H, A, limit, det)
    host = {k: o[k].cpu() for k in ("u", "mu", "log_std", "ga", "gl")}
    d_gpu, b_gpu = gc.grad(gpu, o["u"], o["mu"], o["log_std"], o["ga"], o["gl"], limit)
    d_cpu, b_cpu = gc.grad(gc.build("cpu"), host["u"], host["mu"], host["log_std"], host["ga"], host["gl"], limit)
    _, _, gate_mu, gate_ls, inside = gc.f64_formula(o["u"], o["mu"], o["log_std"], o["ga"], o["gl"], limit, 1e-6)
    diff = np.abs(d_gpu.double().cpu().numpy() - d_cpu.double().numpy())
    assert (diff[:, :A] <= 2 * gate_mu).all() and (diff[:, A:] <= 2 * gate_ls).all()
    assert torch.equal(d_gpu.cpu()[:, A:] == 0, d_cpu[:, A:] == 0)


def test_module_gradients_against_float64(gpu):
    gc.module_gradient_ratios(gpu)


def test_module_semantics(gpu):
    gc.check_module_semantics(gpu)


def test_fallback_is_the_torch_path(gpu):
    gc.check_fallback("cuda:0")


def test_policy_loss_leaves_frozen_critics_alone(gpu):
    gc.check_policy_loss("cuda:0")


def test_no_grad_path_is_unchanged(gpu):
    """fused_grad=True changes nothing where no gradient is wanted: the same launches, the same bits as fused_grad=False."""
    import torch
    outs = []
    for flag in (True, False):
        torch.manual_seed(8)
        ac = gc.make_ac(32, 6, (128, 128), seed=4, fused_grad=flag).cuda()
        o = torch.randn(500, 32, device="cuda")
        with torch.no_grad():
            a, logp = ac.pi(o)
        outs.append((a, logp, ac.act(o), ac.pi._counters.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))

"""mms_param_step on the MI355X (csrc/param_step_kernels.hip), FusedAdam on "cuda" and the opt-in wiring of MADDPG / MAPPO through
it.  The checks are param_step_check.py's, shared with test_param_step.py."""
import pytest

import param_step_check as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device("cuda:0")


@pytest.mark.parametrize("hp", range(len(pc.HP)))
@pytest.mark.parametrize("tensors", range(len(pc.TENSOR_SETS)), ids=[s[0] for s in pc.TENSOR_SETS])
def test_against_float64(torch_cuda, tensors, hp):
    pc.check_against_float64(*_gpu(), "cuda", tensors, hp)


def test_polyak_is_bit_identical_to_the_reference_statements(torch_cuda):
    pc.check_polyak_bits(*_gpu(), "cuda")


def test_norm_semantics(torch_cuda):
    pc.check_norm_semantics(*_gpu(), "cuda")


def test_determinism_and_independence(torch_cuda):
    pc.check_determinism(*_gpu(), "cuda")


def test_nonfinite_gradient(torch_cuda):
    pc.check_nonfinite(*_gpu(), "cuda")


def test_error_paths(torch_cuda):
    pc.check_error_paths(*_gpu(), "cuda", other_device=-1)


def test_kernel_against_cpu_build(torch_cuda):
    """The two builds share param_step_lane.h: on the same inputs the element results are bit-identical wherever the clip coefficient
    is 1, and the norms agree to an fp32 rounding (the partial sums are added in another order, in double)."""
    import torch
    from massive_marl_benchmark_amd import _lib
    hp = pc.HP[2]
    name, numels, offs = pc.TENSOR_SETS[1]
    outs = []
    for lib3, dev in ((_gpu(), "cuda"), ((_lib.lib_cpu(), -1, None), "cpu")):
        pr = pc.Problem(numels, offs, dev, 1.0, hp["wd"], seed=29)
        outs.append(pc.run_once(*lib3, pr, hp, pr.g[0], step=2))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert all(torch.equal(x.cpu(), y) for x, y in zip(a, b))
    assert abs(float(outs[0][4]) - float(outs[1][4])) <= 2.0 ** -23 * float(outs[1][4])


def test_fused_adam(torch_cuda):
    pc.check_fused_adam(torch_cuda.device("cuda:0"))


def test_maddpg_wiring(torch_cuda):
    pc.check_maddpg_wiring("cuda:0")


@pytest.mark.parametrize("algo", ["MAPPO", "HAPPO"])
def test_mappo_wiring(torch_cuda, algo):
    pc.check_mappo_wiring("cuda:0", algo)

"""The critics' loss heads with a gradient (mms_q_heads_loss, csrc/q_loss_kernels.hip) on the MI355X: the kernel against
mms_q_heads_backup's q bit for bit and against float64 from its own q_out, ties, row independence, NULL outputs, the contract, and
the CPU build bit for bit where q is equal (q_loss_check.py's docstring says why that is the exact problem)."""
import pytest

import q_loss_check as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    from massive_marl_benchmark_amd import _lib
    L, device, stream = _lib.for_device("cuda:0")
    return L, device, stream, torch.device("cuda:0")


@pytest.mark.parametrize("M,H,G", lc.SHAPES + [lc.MULTI])
def test_kernel_against_float64(gpu, M, H, G):
    L, device, stream, dev = gpu
    lc.check_shape(L, device, stream, dev, M, H, G, "gpu")


@pytest.fixture
def no_dispatch_override():
    import os
    found = [v for v in lc.qc.DISPATCH_ENV if v in os.environ]
    if found:
        pytest.fail("%s set in the environment: not the shipped dispatch; unset to run these tests" % ", ".join(found))


@pytest.mark.parametrize("M,H,G", lc.NEW_SHAPES)
def test_kernel_table(gpu, no_dispatch_override, M, H, G):
    """One shape per q_heads_loss_kernel<G, NJ> with every chunk live, and one with chunks guarded out (lc.expected_kernel)."""
    L, device, stream, dev = gpu
    lc.check_shape(L, device, stream, dev, M, H, G, "gpu")


@pytest.mark.parametrize("mutation", ["chunk", "last"])
def test_gates_see_a_dropped_chunk_or_element(gpu, no_dispatch_override, mutation):
    """test_q_loss.py's on the device."""
    L, device, stream, dev = gpu
    worst = lc.check_shape(L, device, stream, dev, 33, 1024, 2, "gpu", mutation=mutation)
    assert sorted(worst) == ["dh0", "dh1", "dw0", "dw1"] and min(worst.values()) >= 10, worst


def test_null_outputs_one_network(gpu, no_dispatch_override):
    lc.check_null_outputs(*gpu, M=17, H=320, G=1)


def test_ties_and_strict_rows(gpu):
    lc.check_ties_and_strict(*gpu)


def test_rows_do_not_depend_on_their_place(gpu):
    lc.check_row_independence(*gpu)


def test_null_outputs(gpu):
    lc.check_null_outputs(*gpu)


def test_contract(gpu):
    L, device, stream, dev = gpu
    lc.check_contract(L, device, stream, -1)


@pytest.mark.parametrize("M,H", [(389, 1024), (2100, 128), (lc.MULTI[0], 64)])
def test_cpu_build_bit_for_bit(gpu, M, H):
    """The builds share the partition and the order of every double sum: equal q (the exact problem) gives equal bits everywhere."""
    import torch
    from massive_marl_benchmark_amd import _lib
    L, device, stream, dev = gpu
    for mode in (0, 1):
        a = lc.run_exact(L, device, stream, dev, M, H, mode)
        b = lc.run_exact(_lib.lib_cpu(), -1, None, torch.device("cpu"), M, H, mode)
        assert lc.same_bits(a, b) is None, (mode, lc.same_bits(a, b))

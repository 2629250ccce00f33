"""The head of TRPO's policy step (mms_trpo_heads, csrc/trpo_loss_kernels.hip) on the MI355X: the kernels against float64 next to torch
fp32 at the shapes of test_trpo_heads.py (trpo_heads_check.SHAPES: among them 66 row blocks with a ragged last one) in every index and
old_logp mode, with every output subset's bits; the exact properties, which include the element-wise path at bases 4 bytes past a
16-byte boundary; the error paths in the CPU build's words; gkl and gn bit for bit against the CPU build; mms_ppo_loss's numbers; and a
graph replay of the Python call."""
import pytest

import trpo_heads_check as tc

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


@pytest.mark.parametrize("dense_old_logp", [False, True])
@pytest.mark.parametrize("index_mode", [None, "perm", "repeat"])
@pytest.mark.parametrize("M,A", tc.SHAPES)
def test_kernel_against_float64(torch_cuda, M, A, index_mode, dense_old_logp):
    L, dev, stream = _gpu()
    tc.check(L, dev, stream, M, A, index_mode, dense_old_logp)


def test_exact_properties(torch_cuda):
    L, dev, stream = _gpu()
    tc.exact_properties(L, dev, stream, 1000, 80)
    tc.exact_properties(L, dev, stream, 600, 6)
    tc.exact_properties(L, dev, stream, 8321, 8)


def test_abi_errors_in_the_cpu_build_s_words(torch_cuda):
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    gpu, cpu = [], []
    tc.check_error_paths(L, dev, stream, other_device=-1, messages=gpu)
    tc.check_error_paths(_lib.lib_cpu(), -1, None, other_device=0, messages=cpu)
    differ = ("the wrong device", "a short workspace")                   # each build's own device rule; the CPU build needs no bytes
    assert [m for m in gpu if m[0] not in differ] == [m for m in cpu if m[0] not in differ]
    assert "a short workspace" in [m[0] for m in gpu]


@pytest.mark.parametrize("M,A", [(1000, 80), (257, 3), (8321, 8)])
def test_gkl_and_gn_have_the_cpu_build_s_bits(torch_cuda, M, A):
    """trpo_loss_lane.h states which outputs the two builds share bit for bit: gkl and gn.  The others agree inside the gates."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    pr = tc.problem(M, A, 6)
    c = tc.run(_lib.lib_cpu(), -1, None, pr)["out"]
    g = tc.run(L, dev, stream, {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in pr.items()})["out"]
    for k in ("gkl", "gn"):
        assert torch.equal(c[k], g[k].cpu()), k
    fails, _ = tc.gates(pr, {k: t.cpu() for k, t in g.items()})
    assert not fails, fails


def test_a_loss_kl_and_gsur_are_mms_ppo_loss_s(torch_cuda):
    """The two HIP entries are compiled with different floating-point flags, so here the three agree to the gates' floor, 1e-6 of their
    scale on top of twice fp32 rounding, not bit for bit (test_trpo_heads.py holds the exact form on the CPU build)."""
    L, dev, stream = _gpu()
    for name, (mine, theirs, scale) in tc.logp_equals_ppo_loss(L, dev, stream).items():
        a, b = mine.double().cpu(), theirs.double().cpu()
        assert float((a - b).pow(2).mean().sqrt()) <= (2.0 ** -22 + 1e-6) * scale, name


def test_graph_replay_equals_the_eager_call(torch_cuda):
    """The Python call captured once (two launches, no host synchronisation); mu and the stored fields then change in place: the replay
    equals the eager call bit for bit."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.trpo.heads import StoredRows, trpo_heads
    M, A, B = 1000, 80, 1500
    store, other = tc.problem(B, A, 7, "cuda:0"), tc.problem(B, A, 8, "cuda:0")
    idx = torch.randint(0, B, (M,), generator=torch.Generator().manual_seed(0)).cuda()

    class Rows(StoredRows):
        def __init__(self):
            self.indices, self.rows = idx, M
            self.actions, self.old_mu, self.old_sigma, self.old_logp, self.adv = (store[k] for k in ("actions", "old_mu", "old_sigma", "old_logp", "adv"))

    mu, rmu = store["mu"][idx].clone(), store["rmu"][idx].clone()
    step = lambda: trpo_heads(store["log_std"], mu=mu, rmu=rmu, stored=Rows(), want=tc.OUTPUTS)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                        # warm-up: the workspace exists before the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = step()
        g.replay()
        s.synchronize()
        first = {k: t.clone() for k, t in out.items()}
        assert tc.same(first, step())
        with torch.no_grad():
            mu.copy_(other["mu"][idx])
            for k in tc.STORED:
                store[k].copy_(other[k])
        g.replay()
        s.synchronize()
        second = {k: t.clone() for k, t in out.items()}
        assert tc.same(second, step())
        assert not any(torch.equal(first[k], second[k]) for k in ("out", "logp", "gsur", "gkl"))
    torch.cuda.current_stream().wait_stream(s)

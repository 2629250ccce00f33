"""The grouped loss head of the MAPPO update (mms_marl_ppo_loss_group, csrc/marl_loss_kernels.hip; loss.marl_ppo_loss_group) on the
MI355X: the checks of test_marl_loss_group.py on the HIP build -- every group bit for bit the single entry's kernels on its arguments,
float64 through marl_loss_check.gates, independence, mixed per-group options over one shared block, guard bytes, the error paths in
the CPU build's words, the autograd function -- and a captured graph of the grouped call replayed after the inputs changed."""
import pytest

import marl_loss_group_check as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device(DEV)


@pytest.mark.parametrize("G,M,A", gc.shapes())
def test_every_group_equals_the_single_entry(torch_cuda, G, M, A):
    gc.check_shape(*_gpu(), G, M, A)


def test_shipped_flags(torch_cuda):
    gc.check_shape(*_gpu(), 3, 300, 8, c=gc.mc.cfg(**gc.mc.SHIPPED))
    gc.check_shape(*_gpu(), 2, 300, 6, c=gc.mc.cfg())


def test_groups_are_independent(torch_cuda):
    gc.independence(*_gpu())


def test_mixed_options_over_one_shared_block(torch_cuda):
    gc.mixed_options(*_gpu())


def test_error_paths_in_the_cpu_build_s_words(torch_cuda):
    from massive_marl_benchmark_amd import _lib
    gpu, cpu = [], []
    gc.check_error_paths(*_gpu(), messages=gpu)
    gc.check_error_paths(_lib.lib_cpu(), -1, None, messages=cpu)
    assert [m for m in gpu if m[0] != "a short workspace"] == cpu


@pytest.mark.parametrize("G,M,A", [(3, 200, 6), (33, 20, 3)])
def test_python_layer_equals_the_single_call_per_agent(torch_cuda, G, M, A):
    gc.python_layer(DEV, G, M, A)


def test_graph_replay_equals_the_eager_call(torch_cuda):
    """Forward and backward of three agents captured once on a side stream; the inputs then change in place: the replay equals the
    eager call bit for bit (the table travels in the kernel arguments: nothing of it is read from the host at replay)."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.marl.loss import marl_ppo_loss_group
    G, M, A = 3, 500, 8
    c = gc.ALL
    prs = [gc.mc.problem(M, A, seed=41 + g, device=DEV) for g in range(G)]
    other = [gc.mc.problem(M, A, seed=51 + g, device=DEV) for g in range(G)]
    mus = [pr["mu"].clone().requires_grad_(True) for pr in prs]
    stds = [pr["std"].clone().requires_grad_(True) for pr in prs]
    values = [pr["value"].clone().view(-1, 1).requires_grad_(True) for pr in prs]
    fields = [tuple(pr[k] for k in gc.mc.FIELDS) for pr in prs]
    norms = [(pr["norm_mean"], pr["norm_var"]) for pr in prs]

    def step():
        objs, info = marl_ppo_loss_group(mus, stds, values, fields, norms=norms, row_logp=True, **gc.mc.loss_kwargs(c))
        return tuple(objs) + (info["ratio"], info["value_loss"]) + tuple(info["row_logp"]) + torch.autograd.grad(sum(objs), mus + stds + values)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                        # warm-up: the workspace exists before the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = step()
        g.replay()
        s.synchronize()
        first = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(first, step()))
        with torch.no_grad():
            for gi in range(G):
                mus[gi].copy_(other[gi]["mu"])
                values[gi].copy_(other[gi]["value"].view(-1, 1))
                for k, t in zip(gc.mc.FIELDS, fields[gi]):
                    t.copy_(other[gi][k])
        g.replay()
        s.synchronize()
        second = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(second, step()))
        assert not any(torch.equal(a, b) for a, b in zip(first, second))
    torch.cuda.current_stream().wait_stream(s)

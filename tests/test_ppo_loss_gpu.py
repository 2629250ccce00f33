"""The PPO update's loss head (mms_ppo_loss, csrc/ppo_loss_kernels.hip; loss.ppo_loss; ActorCritic.ppo_loss) on the MI355X: the kernels
against float64 next to torch fp32 at the shapes of test_ppo_loss.py and two more, the exact properties and error paths, the selection
sets against the CPU build's, graph replay, and the module path against the torch chain.

Shapes beyond the CPU file's: (8321, 8) -- two lanes per row, 128 rows per step of a block, so 66 row blocks: more than the 64 partials
the finish pass adds in one sweep of a wave's lanes (kPlMaxBlocks = 1024 keeps a block at one step here), with a last block of one
row -- and (8192, 80), the headline minibatch: 1024 row blocks, 16 sweeps."""
import pytest

import ppo_loss_check as pc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 8), (257, 1), (1000, 80), (4099, 8), (333, pc.MAX_A), (8321, 8), (8192, 80)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device("cuda:0")


@pytest.mark.parametrize("clipped_value", [0, 1])
@pytest.mark.parametrize("M,A", SHAPES)
def test_kernel_against_float64(torch_cuda, M, A, clipped_value):
    import parity
    L, dev, stream = _gpu()
    pr = pc.problem(M, A, seed=1, device="cuda:0")
    stats = {}
    res = pc.check(L, dev, stream, pr, clipped_value=clipped_value, stats=stats)
    parity.record("gpu/ppo_loss/M%d_A%d_cv%d" % (M, A, clipped_value), **{k + "_e_over_et": v["e_over_et"] for k, v in stats.items()},
                  **{k + "_e_over_scale": v["e_over_scale"] for k, v in stats.items()})


def test_scalar_rows_path(torch_cuda):
    """A not a multiple of 4, and a mu that starts 4 bytes past a 16-byte boundary: the rows as scalar loads, the same gates."""
    torch = torch_cuda
    L, dev, stream = _gpu()
    pc.check(L, dev, stream, pc.problem(1000, 6, seed=2, device="cuda:0"))
    pr = pc.problem(1000, 8, seed=2, device="cuda:0")
    aligned = pc.run(L, dev, stream, pr, 1, 0.7, 0.01)
    shifted = torch.zeros(1000 * 8 + 1, device="cuda:0")[1:].view(1000, 8)
    shifted.copy_(pr["mu"])
    assert shifted.data_ptr() % 16 == 4
    res = pc.run(L, dev, stream, dict(pr, mu=shifted), 1, 0.7, 0.01)
    assert res["guards"] and pc.same(res["out"], aligned["out"])          # the lane roles, and so every sum's order, depend on A alone


def test_exact_properties(torch_cuda):
    L, dev, stream = _gpu()
    pc.exact_properties(L, dev, stream, 1000, 80)
    pc.exact_properties(L, dev, stream, 600, 6)
    pc.exact_properties(L, dev, stream, 8321, 8)


def test_abi_errors_in_the_cpu_build_s_words(torch_cuda):
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    gpu, cpu = [], []
    pc.check_error_paths(L, dev, stream, other_device=-1, messages=gpu)
    pc.check_error_paths(_lib.lib_cpu(), -1, None, other_device=0, messages=cpu)
    differ = ("the wrong device", "a short workspace")                   # each build's own device rule; the byte counts
    assert [m for m in gpu if m[0] not in differ] == [m for m in cpu if m[0] not in differ]
    assert [m[0] for m in gpu] == [m[0] for m in cpu]


@pytest.mark.parametrize("M,A", [(1000, 80), (4099, 8), (257, 1)])
def test_selection_sets_equal_the_cpu_build_s(torch_cuda, M, A):
    """Rows with a zero dmu / dvalue, outside the bands: the same set on both builds (a problem as drawn, rows in the bands kept)."""
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    pr = pc.problem(M, A, seed=6, clean=False)
    prg = {k: (t.cuda() if hasattr(t, "cuda") else t) for k, t in pr.items()}
    c = pc.run(_lib.lib_cpu(), -1, None, pr, 1, 0.7, 0.01)["out"]
    g = pc.run(L, dev, stream, prg, 1, 0.7, 0.01)["out"]
    in_r, in_v = pc.bands(pr)
    assert int(in_r.sum()) + int(in_v.sum()) <= pc.BAND_CAP * M
    zc, zg = (c["dmu"] == 0).all(-1), (g["dmu"].cpu() == 0).all(-1)
    assert bool((zc == zg)[~in_r].all()) and int(zc.sum()) > M // 8
    assert bool(((c["dvalue"] == 0) == (g["dvalue"].cpu() == 0))[~in_v].all())
    assert not pc.gates(prg, g, 1, 0.7, 0.01, sums=False)


def test_graph_replay_equals_the_eager_call(torch_cuda):
    """Forward and backward captured once; mu, value and the stored fields then change in place: the replay equals the eager call
    bit for bit."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.loss import ppo_loss
    M, A, B = 1000, 80, 1500
    store = pc.problem(B, A, seed=7, device="cuda:0")
    other = pc.problem(B, A, seed=8, device="cuda:0")
    idx = torch.randint(0, B, (M,), generator=torch.Generator().manual_seed(0)).cuda()
    mu = store["mu"][idx].clone().requires_grad_(True)
    value = store["value"][idx].clone().view(-1, 1).requires_grad_(True)
    log_std = store["log_std"].clone().requires_grad_(True)
    fields = [store[k] for k in pc.FIELDS]

    def step():
        loss, info = ppo_loss(mu, log_std, value, *fields, pc.CLIP, 0.7, 0.01, True, indices=idx)
        return (loss, info["kl"]) + torch.autograd.grad(loss, (mu, log_std, value))

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
            mu.copy_(other["mu"][idx])
            value.copy_(other["value"][idx].view(-1, 1))
            for k, t in zip(pc.FIELDS, fields):
                t.copy_(other[k])
        g.replay()
        s.synchronize()
        second = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(second, step()))
        assert not any(torch.equal(a, b) for a, b in zip(first, second))
    torch.cuda.current_stream().wait_stream(s)


def test_module_path_on_the_device(torch_cuda):
    """ActorCritic.ppo_loss against the torch chain: loss, kl and every parameter's gradient inside the gate; a list of indices gives
    the tensor's bits; the HIP entry ran."""
    torch = torch_cuda
    L, _, _ = _gpu()
    calls = []
    real = L.mms_ppo_loss
    L.mms_ppo_loss = lambda *a: (calls.append(1), real(*a))[1]
    try:
        ac, st = pc.storage_problem(8, 256, 48, 8, seed=3, device="cuda:0")
        batches = list(st.mini_batch_generator(4))
        la, ia, ga = pc.module_check(ac, st, batches[2])
        assert len(calls) == 2                                        # a size query and a launch
        lb, ib, gb = pc.module_check(ac, st, torch.tensor(batches[2], device="cuda:0"))
        assert torch.equal(la, lb) and all(torch.equal(ia[k], ib[k]) for k in ia) and all(torch.equal(a, b) for a, b in zip(ga, gb))
        perm = torch.randperm(2048, generator=torch.Generator().manual_seed(1))[:700].cuda()
        pc.module_check(ac, st, perm, clipped_value=False)
    finally:
        L.mms_ppo_loss = real

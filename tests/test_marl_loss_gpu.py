"""The MAPPO / HAPPO update's loss head (mms_marl_ppo_loss, csrc/marl_loss_kernels.hip; loss.marl_ppo_loss; trainer.MAPPO / HAPPO) on the
MI355X: the kernels against float64 next to torch fp32 at the shapes of test_marl_loss.py and two more, every flag set, the exact
properties, pitched storage and error paths, the selection sets against the CPU build's, graph replay, the autograd function, the
fallbacks and the trainers on both buffer classes.

Shapes beyond the CPU file's (the geometry is ppo_loss_kernels.hip's, see marl_loss_check.py): (8321, 8) -- two lanes per row, 128 rows
per step of a block, so 66 row blocks: more than the 64 partials the finish pass adds in one sweep of a wave's lanes, with a last block
of one row -- and (32768, 8), the workload's minibatch (episode_length 8 x 4096 envs): 256 row blocks, four sweeps, and the mask pass's
64 blocks with two rows per thread.

MMS_MARL_LOSS_RECORD=<path> makes test_kernel_against_float64 write the e / et it measured there (profiles/marl_loss_error.json)."""
import os

import pytest

import marl_loss_check as mc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 8), (257, 1), (1000, 80), (4099, 8), (333, mc.MAX_A), (1000, 6), (8321, 8), (32768, 8)]
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


@pytest.mark.parametrize("flags", ["shipped", "all"])
@pytest.mark.parametrize("M,A", SHAPES)
def test_kernel_against_float64(torch_cuda, M, A, flags):
    import parity
    L, dev, stream = _gpu()
    pr = mc.problem(M, A, seed=1, device=DEV)
    stats = {}
    mc.check(L, dev, stream, pr, dict(mc.FLAG_SETS)[flags], stats=stats)
    name = "M%d_A%d_%s" % (M, A, flags)
    parity.record("gpu/marl_loss/" + name, **{k + "_e_over_et": v["e_over_et"] for k, v in stats.items()},
                  **{k + "_e_over_scale": v["e_over_scale"] for k, v in stats.items()})
    mc.STATS[name] = stats
    mc.write_error_record(os.environ.get("MMS_MARL_LOSS_RECORD"),
                          "mms_marl_ppo_loss on one MI355X (tests/test_marl_loss_gpu.py::test_kernel_against_float64): per output, e / et = rms error "
                          "against float64 over torch fp32 autograd's on the same inputs, and e / scale (scale: the same reduction over absolute values; "
                          "rms of the truth for dmu, dvalue and row_logp). Gate: e <= 1.25 et, or e <= 2 et + 1e-6 scale where et <= 2^-22 scale "
                          "(tests/marl_loss_check.py).")


@pytest.mark.parametrize("flags", [name for name, _ in mc.FLAG_SETS])
def test_each_flag_and_the_shipped_combinations(torch_cuda, flags):
    L, dev, stream = _gpu()
    mc.check(L, dev, stream, mc.problem(1000, 8, seed=2, device=DEV), dict(mc.FLAG_SETS)[flags])


def test_exact_properties(torch_cuda):
    L, dev, stream = _gpu()
    mc.exact_properties(L, dev, stream, 1000, 80)
    mc.exact_properties(L, dev, stream, 600, 6, c=mc.cfg(**mc.SHIPPED))
    mc.exact_properties(L, dev, stream, 8321, 8)


def test_pitched_storage_of_a_shared_block(torch_cuda):
    L, dev, stream = _gpu()
    mc.pitched_storage(L, dev, stream)
    mc.pitched_storage(L, dev, stream, A=6, c=mc.cfg(**mc.SHIPPED))
    mc.pitched_storage(L, dev, stream, T=8, N=600, c=mc.cfg(**mc.SHIPPED))


def test_abi_errors_in_the_cpu_build_s_words(torch_cuda):
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    gpu, cpu = [], []
    mc.check_error_paths(L, dev, stream, other_device=-1, messages=gpu)
    mc.check_error_paths(_lib.lib_cpu(), -1, None, other_device=0, messages=cpu)
    differ = ("the wrong device", "a short workspace")                   # each build's own device rule; the byte counts
    assert [m for m in gpu if m[0] not in differ] == [m for m in cpu if m[0] not in differ]
    assert [m[0] for m in gpu] == [m[0] for m in cpu]


@pytest.mark.parametrize("M,A", [(1000, 80), (4099, 8), (257, 1)])
def test_selection_sets_equal_the_cpu_build_s(torch_cuda, M, A):
    """Rows with a zero dmu / dvalue, outside the bands: the same set on both builds (a problem as drawn, rows in the bands kept)."""
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    c = mc.cfg(huber=1, clipped=1, pm=1, vm=1, norm=1, factor=1)
    pr = mc.problem(M, A, seed=6, clean=False)
    prg = {k: (t.cuda() if hasattr(t, "cuda") else t) for k, t in pr.items()}
    o = mc.run(_lib.lib_cpu(), -1, None, pr, c)["out"]
    g = mc.run(L, dev, stream, prg, c)["out"]
    in_r, in_v = mc.bands(pr)
    assert int(in_r.sum()) + int(in_v.sum()) <= mc.BAND_CAP * M
    zc, zg = (o["dmu"] == 0).all(-1), (g["dmu"].cpu() == 0).all(-1)
    assert bool((zc == zg)[~in_r].all()) and int(zc.sum()) > M // 8
    assert bool(((o["dvalue"] == 0) == (g["dvalue"].cpu() == 0))[~in_v].all())
    assert not mc.gates(prg, g, c, sums=False)


def test_graph_replay_equals_the_eager_call(torch_cuda):
    """Forward and backward captured once on a side stream; mu, value and the stored fields then change in place: each replay equals the
    eager call bit for bit."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.marl.loss import marl_ppo_loss
    M, A, B = 1000, 8, 1500
    c = mc.cfg(huber=1, clipped=1, pm=1, vm=1, norm=1, factor=1)
    store = mc.problem(B, A, seed=7, device=DEV)
    other = mc.problem(B, A, seed=8, device=DEV)
    idx = torch.randint(0, B, (M,), generator=torch.Generator().manual_seed(0)).cuda()
    mu = store["mu"][idx].clone().requires_grad_(True)
    value = store["value"][idx].clone().view(-1, 1).requires_grad_(True)
    std = store["std"].clone().requires_grad_(True)
    fields = [store[k] for k in mc.FIELDS]

    def step():
        obj, info = marl_ppo_loss(mu, std, value, *fields, **mc.loss_kwargs(c, store, indices=idx, row_logp=True))
        return (obj, info["ratio"], info["value_loss"], info["row_logp"]) + torch.autograd.grad(obj, (mu, std, value))

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
            for k, t in zip(mc.FIELDS, fields):
                t.copy_(other[k])
        g.replay()
        s.synchronize()
        second = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(second, step()))
        assert not any(torch.equal(a, b) for a, b in zip(first, second))
    torch.cuda.current_stream().wait_stream(s)


@pytest.mark.parametrize("flags", ["shipped_happo", "all"])
def test_autograd_function_against_torch(torch_cuda, flags):
    mc.autograd_function(DEV, dict(mc.FLAG_SETS)[flags], M=3000, A=8)


def test_inputs_the_entry_does_not_take_fall_back_to_torch(torch_cuda):
    mc.fallbacks(DEV)


@pytest.mark.parametrize("algo,kind,over", [("MAPPO", "shared", {}), ("HAPPO", "separated", dict(use_policy_active_masks=True, use_value_active_masks=True))])
def test_train_equals_a_loop_of_ppo_update(torch_cuda, algo, kind, over):
    mc.train_equals_update_loop(DEV, algo, kind, **over)


@pytest.mark.parametrize("algo,over", [("MAPPO", {}), ("HAPPO", {}), ("MAPPO", dict(use_popart=False, use_valuenorm=True))])
def test_ppo_update_against_the_reference_s_sequence(torch_cuda, algo, over):
    trainer, _ = mc.trainer_update_against_reference(DEV, algo, **over)
    if trainer.value_normalizer is not None:
        assert trainer.value_normalizer.running_mean.device.type == "cuda"

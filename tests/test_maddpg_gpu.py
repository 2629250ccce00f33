"""MADDPG on the MI355X: the two HIP entries mms_det_heads_act_group and mms_q_heads_backup_group (csrc/maddpg_kernels.hip) per
case, against the CPU build, and the modules of algorithms/marl/maddpg through the fused paths.  The checks are maddpg_check.py's,
shared with test_maddpg.py."""
import pytest

import maddpg_check as mc

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


@pytest.mark.parametrize("case", mc.HEAD_CASES, ids=lambda c: "M%d-H%d-A%d-G%d-a%d" % c)
def test_head_against_float64(torch_cuda, case):
    mc.check_head_case(*_gpu(), case, "cuda")


def test_head_exactness(torch_cuda):
    mc.check_head_exactness(*_gpu(), "cuda")


@pytest.mark.parametrize("case", [(7, 64, 3, 2, 0), (17, 512, 8, 10, 0), (333, 512, 16, 3, 2), (1000, 512, 8, 10, 5)], ids=lambda c: "M%d-H%d-A%d-G%d-a%d" % c)
def test_head_noise(torch_cuda, case):
    mc.check_head_noise(*_gpu(), case, "cuda")


def test_head_noise_statistics_and_cpu_build(torch_cuda):
    """The device's draws pass the statistics check and agree with the CPU build's for the same keys within 1e-5 (1 + |z|), the gate of
    test_sac_actor_gpu.py::test_kernel_against_cpu_build for this stream (the device's fast logf / cosf inside Box-Muller)."""
    from massive_marl_benchmark_amd import _lib
    zg = mc.check_head_statistics(*_gpu(), "cuda").cpu()
    zc = mc.zero_head_draws(_lib.lib_cpu(), -1, None, "cpu")
    err = ((zg - zc).abs() / (1 + zc.abs())).max()
    print("max |z_gpu - z_cpu| / (1 + |z|) = %.3g" % float(err))
    assert err <= 1e-5


def test_head_error_paths(torch_cuda):
    mc.check_head_error_paths(*_gpu(), other_device=-1)


@pytest.mark.parametrize("case", mc.Q_CASES, ids=lambda c: "M%d-H%d-G%d" % c)
def test_q_group_equals_ungrouped(torch_cuda, case):
    mc.check_q_case(*_gpu(), case, "cuda")


def test_q_group_error_paths(torch_cuda):
    mc.check_q_error_paths(*_gpu(), other_device=-1)


# ---- every det_heads_act_kernel<NCT, WAVES> and every part of the grouped Q kernel's k-loop (maddpg_check's docstring) ----

@pytest.fixture
def no_dispatch_override():
    import os
    found = [v for v in mc.qc.DISPATCH_ENV if v in os.environ]
    if found:
        pytest.fail("%s set in the environment: not the shipped dispatch; unset to run these tests" % ", ".join(found))


@pytest.mark.parametrize("case", mc.NEW_HEAD_CASES, ids=lambda c: "M%d-H%d-A%d-G%d-a%d" % c)
def test_head_kernel_table(torch_cuda, no_dispatch_override, case):
    """One case per det_heads_act_kernel<NCT, WAVES> (mc.expected_kernel): sigma = 0 against float64 in every destination layout, then
    sigma > 0 against mms_ppo_act's stream."""
    mc.check_head_case(*_gpu(), case, "cuda")
    mc.check_head_noise(*_gpu(), mc.noise_case(case), "cuda")


@pytest.mark.parametrize("mutation", ["tile", "last"])
def test_head_gate_sees_a_dropped_tile_or_column(torch_cuda, no_dispatch_override, mutation):
    """test_maddpg.py's, with the device's e_ref in the gate."""
    assert mc.check_head_case(*_gpu(), (33, 768, 113, 3, 0), "cuda", mutation=mutation) >= 10
    assert mc.check_head_case(*_gpu(), (1, 512, 128, 3, 2), "cuda", mutation=mutation) >= 10


@pytest.mark.parametrize("case", mc.NEW_Q_CASES, ids=lambda c: "M%d-H%d-G%d" % c)
def test_q_group_path_table(torch_cuda, no_dispatch_override, case):
    mc.check_q_case(*_gpu(), case, "cuda")


# ---- the modules through the fused paths on the device ----

def test_losses_at_initial_parameters(torch_cuda, monkeypatch):
    mc.check_losses("cuda:0", _gpu()[0], monkeypatch)


def test_ddpg_update_and_ordering(torch_cuda, monkeypatch):
    mc.check_update("cuda:0", _gpu()[0], monkeypatch)


def test_train_dicts(torch_cuda):
    mc.check_train("cuda:0")


def test_use_target_critic(torch_cuda, monkeypatch):
    mc.check_target_critic("cuda:0", _gpu()[0], monkeypatch)


def test_storage_on_device(torch_cuda):
    mc.check_storage("cuda:0")


def test_act_all_33_agents_padded_rows(torch_cuda, monkeypatch):
    mc.check_act_all("cuda:0", _gpu()[0], monkeypatch)


def test_graph_replay_follows_the_parameters(torch_cuda):
    """act_all and a target pass captured in one graph; after a polyak write into every actor and target actor a replay equals eager
    and differs from the first replay (nothing derived from the parameters is kept between calls); a captured noisy act_all draws
    fresh normals on every replay (the counters live on the device)."""
    torch = torch_cuda
    config, policies, trainer = mc.make_trainer(3, 10, 12, 2, (64, 64), "cuda:0", seed=4)
    _, other, _ = mc.make_trainer(3, 10, 12, 2, (64, 64), "cuda:0", seed=5)
    M = 48
    obs = [torch.randn(M, 10, device="cuda") for _ in range(3)]
    data = [{"obs2": torch.randn(4, 12, 10, device="cuda"), "sobs2": torch.randn(4, 12, 12, device="cuda")} for _ in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        trainer.act_all(obs, deterministic=True)                    # warm-up
        trainer.act_all(obs, deterministic=False)
        trainer._target_inputs(data)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _, joint = trainer.act_all(obs, deterministic=True)
            _, noisy = trainer.act_all(obs, deterministic=False)
            xin = trainer._target_inputs(data)["xin"][:, 12:]        # the joint-action columns (the left ones wait for share_obs2)
        g.replay()
        s.synchronize()
        first, first_x, first_noisy = joint.clone(), xin.clone(), noisy.clone()
        assert torch.equal(first, trainer.act_all(obs, deterministic=True)[1]) and torch.equal(first_x, trainer._target_inputs(data)["xin"][:, 12:])
        g.replay()
        s.synchronize()
        assert torch.equal(joint, first) and not torch.equal(noisy, first_noisy)
        with torch.no_grad():
            for po, ot in zip(policies, other):
                for net, onet in ((po.actor, ot.actor), (po.actor_targ, ot.actor_targ)):
                    for p_targ, p in zip(net.parameters(), onet.parameters()):
                        p_targ.data.mul_(0.5)
                        p_targ.data.add_(0.5 * p.data)
        g.replay()
        s.synchronize()
        second, second_x = joint.clone(), xin.clone()
        assert torch.equal(second, trainer.act_all(obs, deterministic=True)[1]) and torch.equal(second_x, trainer._target_inputs(data)["xin"][:, 12:])
        assert not torch.equal(first, second) and not torch.equal(first_x, second_x)
    torch.cuda.current_stream().wait_stream(s)


def test_runner_ten_ant(torch_cuda, monkeypatch, tmp_path):
    mc.check_runner("cuda", _gpu()[0], monkeypatch, tmp_path)

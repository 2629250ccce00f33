"""The off-policy Q target (mms_q_heads_backup, algorithms/rl/{ddpg,td3,sac}/module.py: fused_q_forward, fused_q_backup, q_backup)
without a GPU: the reference's compute_loss_q fixture through the torch path, the CPU build of the kernel against float64, its exact
properties and error paths, and the modules' semantics."""
import copy
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn

import q_check as qc
from conftest import load_golden
from massive_marl_benchmark_amd import _lib, spaces
from massive_marl_benchmark_amd.algorithms.rl.ddpg import module as ddpg_module
from massive_marl_benchmark_amd.algorithms.rl.sac import module as sac_module
from massive_marl_benchmark_amd.algorithms.rl.td3 import module as td3_module


def boxes(W, A):
    return spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-np.ones(A), np.ones(A))


def make_ac(algo, W, A, hidden, device="cpu", **kw):
    ob, ac = boxes(W, A)
    if algo == "sac":
        return sac_module.MLPActorCritic(ob, ac, hidden_sizes=hidden, **kw).to(device)
    mod = td3_module if algo == "td3" else ddpg_module
    return mod.MLPActorCritic(ob, ac, 0.1, device, hidden_sizes=hidden, **kw).to(device)


def fixture_target(g, algo, device="cpu", **kw):
    """This build's actor-critic with the fixture's target parameters (stored as the upper halves of their fp32 words, key order)."""
    W, A, *hidden = (int(x) for x in g["shape"])
    targ = make_ac(algo, W, A, tuple(hidden), **kw)
    sd = targ.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[algo + "_targ_keys"]]
    flat = torch.from_numpy((g[algo + "_targ_bf16"].astype(np.uint32) << 16).view(np.float32).copy())
    assert flat.numel() == sum(v.numel() for v in sd.values())
    at = 0
    for k, v in sd.items():
        sd[k] = flat[at:at + v.numel()].view(v.shape)
        at += v.numel()
    targ.load_state_dict(sd)
    return targ.to(device)


def fixture_loss(g, algo, targ, device="cpu"):
    t = lambda k: torch.from_numpy(g["%s_%s" % (algo, k)]).to(device)
    gamma, alpha = float(g["gamma"]), float(g["alpha"])
    if algo == "sac":
        backup = targ.q_backup(t("obs2"), t("a2"), t("r"), t("done"), gamma, alpha, t("logp_a2"))
    else:
        backup = targ.q_backup(t("obs2"), t("a2"), t("r"), t("done"), gamma)
    assert backup.shape == (4, 16, 1) and not backup.requires_grad
    loss = ((t("q1") - backup) ** 2).mean() + ((t("q2") - backup) ** 2).mean()
    return float(loss), float(g[algo + "_loss_q"])


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_reference_fixture_through_torch_path(algo):
    g = load_golden("q_target")
    assert g["sac_done"].dtype == np.uint8 and g["sac_done"].min() == 0 and g["sac_done"].max() == 1 and g["sac_r"].shape == (4, 16, 1)
    loss, stored = fixture_loss(g, algo, fixture_target(g, algo, fused_q=True))
    print("loss_q %.9g stored %.9g" % (loss, stored))
    assert abs(loss - stored) <= 1e-6 * abs(stored)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("with_logp", [True, False])
@pytest.mark.parametrize("M,H", [(1, 64), (37, 192), (200, 1024), (37, 64), (1, 1024), (300, 192), (37, 4096)])
def test_cpu_build_against_float64(M, H, G, with_logp):
    L = _lib.lib_cpu()
    pr = qc.problem(M, H, G, seed=3)
    q, backup = qc.run(L, -1, None, pr, with_logp=with_logp)
    for g in range(G):
        q64, s = qc.f64_q(pr, g)
        err = np.abs(q[g].double().numpy() - q64) / s
        print("M %d H %d g %d: max |q - q64| / s = %.3g" % (M, H, g, err.max()))
        assert (err <= 1e-6).all()
        qc.note("cpu", "q_heads_backup", "old", err.max() / 1e-6)
    qc.check_backup(q, backup, pr, with_logp, 0.99, 0.2, "cpu M %d H %d G %d" % (M, H, G))


def test_case_table_reaches_every_path():
    """Both kernels with each part of the k-loop; the shapes that ran before the table never ran both parts in one call."""
    assert qc.coverage() == qc.REACHABLE and len(qc.REACHABLE) == 6
    assert {qc.expected_path(H) for H in qc.OLD_H} == {"remainder", "unrolled"}
    assert [qc.expected_path(H) for H in (64, 192, 256, 320, 448, 576, 4096)] == ["remainder", "remainder", "unrolled", "both", "both", "both", "unrolled"]


@pytest.mark.parametrize("M,H,G", qc.CASES)
def test_path_table(M, H, G):
    qc.check_case(_lib.lib_cpu(), -1, None, "cpu", M, H, G)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("mutation", ["chunk", "last"])
def test_gate_sees_a_dropped_chunk_or_element(mutation, G):
    """The float64 side without the last 64 k, or without the last k, at nj = 9: the gate is missed at least ten times over."""
    assert qc.check_case(_lib.lib_cpu(), -1, None, "cpu", 33, 576, G, mutation=mutation) >= 10


def test_exact_properties_cpu_build():
    qc.exact_properties(_lib.lib_cpu(), -1, None, qc.problem(1000, 128, 2, seed=9))


def test_abi_errors_cpu_build():
    qc.check_error_paths(_lib.lib_cpu(), -1, None, other_device=0)


def test_symbol_is_exported_by_both_libraries():
    assert "mms_q_heads_backup" in _lib.SYMBOLS
    assert hasattr(_lib.lib_cpu(), "mms_q_heads_backup")
    import ctypes
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mms_q_heads_backup")


@pytest.mark.parametrize("algo", ["ddpg", "td3", "sac"])
def test_module_semantics(algo):
    mod = {"ddpg": ddpg_module, "td3": td3_module, "sac": sac_module}[algo]
    params = list(inspect.signature(mod.MLPActorCritic.__init__).parameters)
    assert params[-1] == "fused_q"                                     # last keyword: the reference's positional order is kept
    ob, ac_space = boxes(12, 4)
    if algo == "sac":
        ac = mod.MLPActorCritic(ob, ac_space, (64, 64), nn.ELU)        # positional, as the reference constructs it
    else:
        ac = mod.MLPActorCritic(ob, ac_space, 0.1, "cpu", (64, 64), nn.ReLU)
    critics = [ac.q] if algo == "ddpg" else [ac.q1, ac.q2]
    assert ac.fused_q is True and all(q.fused_q is True for q in critics)
    off = make_ac(algo, 12, 4, (64, 64), fused_q=False)
    assert off.fused_q is False and all(q.fused_q is False for q in ([off.q] if algo == "ddpg" else [off.q1, off.q2]))
    keys = list(ac.state_dict().keys())
    names = ("pi", "q") if algo == "ddpg" else ("pi", "q1", "q2")
    assert all(k.split(".")[0] in names for k in keys) and not any("fused" in k for k in keys) and not list(ac.buffers())
    n_q = 1 if algo == "ddpg" else 2
    assert sum(k.startswith("q") for k in keys) == 6 * n_q            # three Linears per critic, weight + bias: the reference's keys
    twin = copy.deepcopy(ac)
    assert list(twin.state_dict().keys()) == keys and twin.fused_q is True
    assert list(ac.to(torch.float64).state_dict().keys()) == keys
    ac = ac.float()
    # grad enabled, parameters requiring grad: the torch path, differentiable (compute_loss_q's online critics)
    o, a = torch.randn(3, 5, 12), torch.randn(3, 5, 4)
    q = critics[0](o, a)
    assert q.requires_grad and q.shape == (3, 5, 1)
    q.sum().backward()
    assert critics[0].q[0].weight.grad is not None
    # q_backup on CPU tensors is the literal expression
    r, d = torch.randn(3, 5, 1), (torch.rand(3, 5, 1) < 0.4)
    logp = torch.randn(3, 5, 1)
    with torch.no_grad():
        qmin = critics[0](o, a) if n_q == 1 else torch.min(critics[0](o, a), critics[1](o, a))
        df = d.float()
        want = r + 0.99 * (1 - df) * (qmin - 0.2 * logp)
        want_plain = r + 0.99 * (1 - df) * qmin
    for dd in (d, d.to(torch.uint8), df):
        got = ac.q_backup(o, a, r, dd, 0.99, 0.2, logp)
        assert torch.equal(got, want) and not got.requires_grad and got.shape == r.shape
        assert torch.equal(ac.q_backup(o, a, r, dd, 0.99), want_plain)
    assert torch.equal(got[d], r[d])
    with pytest.raises(ValueError):
        ac.q_backup(o, a, r, d, 0.99, alpha=0.2)
    # the fused functions decline CPU tensors instead of doing part of the work
    assert ddpg_module.fused_q_forward(critics, o, a) is None

"""TRPO's ActorCritic (massive_marl_benchmark_amd/algorithms/rl/trpo) on the CPU build: the import contract, mms_mlp_grad /
mms_mlp_grad_rop through `evaluate` and the two autograd calls of kl_hessian_times_vector against float64 torch autograd, the fallbacks,
determinism and the ABI's error paths."""
import copy
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from massive_marl_benchmark_amd import _lib  # noqa: E402
from trpo_check import hvp_parts, make_actor, rms, within_torch  # noqa: E402

SMALL = {"pi_hid_sizes": [32, 24, 16], "vf_hid_sizes": [32, 24, 16], "activation": "elu"}
ODD = {"pi_hid_sizes": [36, 20, 12], "vf_hid_sizes": [36, 20, 12], "activation": "elu"}    # widths not multiples of 32


def test_module_contract():
    from massive_marl_benchmark_amd.algorithms.rl import trpo
    from massive_marl_benchmark_amd.algorithms.rl.ppo import module as ppo_module
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage as PPOStorage
    assert trpo.RolloutStorage is PPOStorage
    assert issubclass(trpo.ActorCritic, ppo_module.ActorCritic)
    ac = trpo.ActorCritic((20,), (20,), (6,), 0.8, SMALL)
    ppo = ppo_module.ActorCritic((20,), (20,), (6,), 0.8, SMALL)
    assert list(ac.state_dict().keys()) == list(ppo.state_dict().keys())
    assert not ac.fused_grad and trpo.ActorCritic((20,), (20,), (6,), 0.8, SMALL, fused_grad=True).fused_grad   # opt-in
    assert trpo.ActorCritic.evaluate is not ppo_module.ActorCritic.evaluate
    for name in ("act", "act_inference"):
        assert getattr(trpo.ActorCritic, name) is getattr(ppo_module.ActorCritic, name)


def _against_float64(ac, obs, act, old_mu, v):
    t32 = copy.deepcopy(ac)
    t32.fused_grad = False
    ref = copy.deepcopy(ac).double()
    ref.fused_grad = False
    a = hvp_parts(ac, obs, act, old_mu, v)
    b = hvp_parts(ref, obs.double(), act.double(), old_mu.double(), v.double())
    c = hvp_parts(t32, obs, act, old_mu, v)
    return [(rms(x.double() - y), rms(z.double() - y), rms(y)) for x, y, z in zip(a, b, c)]


@pytest.mark.parametrize("cfg", [SMALL, ODD], ids=["32-24-16", "36-20-12"])
@pytest.mark.parametrize("moved", [False, True], ids=["mu==old_mu", "mu!=old_mu"])
def test_cpu_build_against_float64(cfg, moved):
    ac, obs, act, old_mu, v = make_actor((20,), 6, cfg, 40, torch.device("cpu"), moved)
    assert within_torch(_against_float64(ac, obs, act, old_mu, v)) == []


def test_curvature_term_matters():
    """With mu != old_mu the HVP has the term sum_rows g . (d2 mu) v; the Gauss-Newton part alone would be off by far more than
    rounding -- the fused HVP matches float64 only because the R-op supplies it."""
    ac, obs, act, old_mu, v = make_actor((20,), 6, SMALL, 40, torch.device("cpu"), True)
    with torch.no_grad():
        old_mu = old_mu + 0.5 * torch.randn(old_mu.shape, generator=torch.Generator().manual_seed(9))
    ref = copy.deepcopy(ac).double()
    ref.fused_grad = False
    full = hvp_parts(ref, obs.double(), act.double(), old_mu.double(), v.double())[3]
    # the Gauss-Newton part: J^T (d2 KL / d mu2) J v, with d2 KL / d mu2 = 1 / (N sigma^2) per element
    params = list(ref.actor.parameters())
    mu = ref.actor(obs.double())
    sig2 = torch.exp(ref.log_std.detach()) ** 2
    vs, i = [], 0
    for p in params:
        vs.append(v.double()[i:i + p.numel()].view(p.shape))
        i += p.numel()
    jv = torch.autograd.functional.jvp(lambda *ps: torch.func.functional_call(ref.actor, {n: q for (n, _), q in zip(ref.actor.named_parameters(), ps)},
                                                                              (obs.double(),)), tuple(p.detach() for p in params), tuple(vs))[1]
    gn = torch.autograd.grad(mu, params, jv / (mu.shape[0] * sig2))
    gn = torch.cat([t.reshape(-1) for t in gn])
    fused = hvp_parts(ac, obs, act, old_mu, v)[3].double()
    assert rms(full - gn) > 100 * rms(fused - full)


@pytest.mark.parametrize("case", ["relu", "fused_grad_off", "obs_requires_grad"])
def test_fallbacks_equal_ppo_evaluate(case):
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic as PPO
    cfg = dict(SMALL, activation="relu") if case == "relu" else SMALL
    torch.manual_seed(0)
    ac = __import__("massive_marl_benchmark_amd.algorithms.rl.trpo", fromlist=["ActorCritic"]).ActorCritic((20,), (20,), (6,), 0.8, cfg,
                                                                                                          fused_grad=case != "fused_grad_off")
    assert case != "fused_grad_off" or not ac.fused_grad
    ppo = PPO((20,), (20,), (6,), 0.8, cfg)
    ppo.load_state_dict(ac.state_dict())
    obs = torch.randn(40, 20, requires_grad=case == "obs_requires_grad")
    act = torch.randn(40, 6)
    assert not ac._grad_path_qualifies(obs)
    for x, y in zip(ac.evaluate(obs, None, act), ppo.evaluate(obs, None, act)):
        assert torch.equal(x, y)
        assert (x.grad_fn is None) == (y.grad_fn is None)


def test_qualifying_actor_takes_the_kernels():
    ac, obs, act, old_mu, v = make_actor((20,), 6, SMALL, 40, torch.device("cpu"), False)
    assert ac._grad_path_qualifies(obs)
    mean = ac.evaluate(obs, None, act)[3]
    assert type(mean.grad_fn).__name__ == "_ActorMLPBackward"


def test_hvp_deterministic():
    ac, obs, act, old_mu, v = make_actor((20,), 6, ODD, 40, torch.device("cpu"), True)
    a = hvp_parts(ac, obs, act, old_mu, v)
    b = hvp_parts(ac, obs, act, old_mu, v)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_abi_errors():
    L = _lib.lib_cpu()
    n = ctypes.c_int64(0)
    dims = (ctypes.c_int32 * 3)(8, 4, 2)
    # wrong device, bad layer count, bad widths: non-zero with a message
    assert L.mms_mlp_grad(0, 2, 4, dims, *([None] * 8), None, ctypes.byref(n), None) != 0
    assert b"device must be -1" in L.mms_last_error(None)
    assert L.mms_mlp_grad(-1, 1, 4, dims, *([None] * 8), None, ctypes.byref(n), None) != 0
    assert b"bad arguments" in L.mms_last_error(None)
    bad = (ctypes.c_int32 * 3)(8, 0, 2)
    assert L.mms_mlp_grad_rop(-1, 2, 4, bad, *([None] * 11), None, ctypes.byref(n), None) != 0
    assert b"bad arguments" in L.mms_last_error(None)
    assert L.mms_mlp_grad(-1, 2, 4, dims, *([None] * 8), None, None, None) != 0          # ws_bytes is required
    # size query, then null data pointers
    assert L.mms_mlp_grad(-1, 2, 4, dims, *([None] * 8), None, ctypes.byref(n), None) == 0 and n.value == 0
    ws = torch.empty(256, dtype=torch.uint8)
    n = ctypes.c_int64(256)
    assert L.mms_mlp_grad(-1, 2, 4, dims, *([None] * 8), ctypes.c_void_p(ws.data_ptr()), ctypes.byref(n), None) != 0
    assert b"null pointer" in L.mms_last_error(None)
    assert L.mms_mlp_grad_rop(-1, 2, 4, dims, *([None] * 11), ctypes.c_void_p(ws.data_ptr()), ctypes.byref(n), None) != 0
    assert b"null pointer" in L.mms_last_error(None)
    for sym in ("mms_mlp_grad", "mms_mlp_grad_rop"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym)


def test_reference_fixture_replay():
    """tests/golden/trpo_update.npz: the reference's own trpo.py (kl_hessian_times_vector, conjugate_gradient, line_search) on one
    minibatch with mu != old_mu, replayed with this build's ActorCritic(fused_grad=True) on the CPU build.  The reference ran torch fp32
    autograd through MultivariateNormal; this build's torch path (fused_grad=False) lands 1.4e-6 .. 2.4e-6 (relative rms) from it on
    flat_g / step_dir / full_step, so 1e-5 bounds both paths with room and would not hold for a wrong HVP."""
    from massive_marl_benchmark_amd.algorithms.rl.trpo import ActorCritic
    from trpo_check import minibatch_sequence
    import numpy as np
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trpo_update.npz"))
    shape, hy = [int(x) for x in f["shape"]], f["hyper"]
    cfg = {"pi_hid_sizes": shape[1:-1], "vf_hid_sizes": shape[1:-1], "activation": "elu"}
    ac = ActorCritic((shape[0],), (shape[0],), (shape[-1],), float(hy[0]), cfg, fused_grad=True)
    keys = [str(k) for k in f["keys"]]
    assert keys == list(ac.state_dict().keys())
    ac.load_state_dict({k: torch.from_numpy(f["sd%d" % i]) for i, k in enumerate(keys)})
    T = lambda k: torch.from_numpy(f[k])                                  # noqa: E731
    assert ac._grad_path_qualifies(T("obs"))
    out = minibatch_sequence(ac, T("obs"), T("actions"), T("advantages"), T("old_logp"), T("old_mu"), T("old_sigma"), T("v"), float(hy[1]),
                             int(hy[2]), float(hy[3]), int(hy[4]), float(hy[5]), float(hy[6]))
    for k in ("flat_g", "hv", "step_dir", "full_step"):
        assert rms(out[k] - T(k)) <= 1e-5 * rms(T(k)), k
    assert out["success"] == bool(f["success"])
    assert rms(out["params_after"] - T("params_after")) <= 1e-5 * rms(T("full_step"))

"""SAC's actor-critic (algorithms/rl/sac/module.py) and its fused head mms_sac_heads_act, without a GPU: the reference fixture through
the torch path, the CPU build of the head against float64, the counter-based draws, module semantics and the ABI's error paths."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import sac_check as sc
from conftest import load_golden
from massive_marl_benchmark_amd import _lib, spaces
from massive_marl_benchmark_amd.algorithms.rl.sac import MLPActorCritic, ReplayBuffer
from massive_marl_benchmark_amd.algorithms.rl.ddpg.storage import ReplayBuffer as DDPGReplayBuffer


def _ac(W, A, hidden, limit=1.0, **kw):
    return MLPActorCritic(spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-limit * np.ones(A), limit * np.ones(A)),
                          hidden_sizes=hidden, **kw)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_fixture_through_torch_path(tag):
    g = load_golden("sac_actor")
    W, A, *hidden = (int(x) for x in g[tag + "_shape"])
    keys = [str(k) for k in g[tag + "_keys"]]
    ref_sd = {k: torch.from_numpy(g["%s_sd%d" % (tag, i)]) for i, k in enumerate(keys)}
    torch.manual_seed(int(g[tag + "_seed"]))
    ac = _ac(W, A, hidden)
    sd = ac.state_dict()
    assert list(sd.keys()) == keys
    for k in keys:
        assert sd[k].shape == ref_sd[k].shape, k
        assert torch.equal(sd[k], ref_sd[k]), k                  # the seed draw comes after every layer: the reference's initialisation
    ac.load_state_dict(ref_sd)
    o = torch.from_numpy(g[tag + "_obs"])
    with torch.no_grad():
        a, logp = ac.pi(o, deterministic=True)
        q1, q2 = ac.q1(o, a), ac.q2(o, a)
    act = ac.act(o, deterministic=True)
    close = lambda x, ref: float((x.double() - torch.from_numpy(ref).double()).abs().max() / (1 + np.abs(ref).max()))
    assert logp.shape == (64, 1) and a.shape == (64, A)
    assert close(a, g[tag + "_action"]) <= 1e-6
    assert close(act, g[tag + "_act"]) <= 1e-6
    assert close(logp, g[tag + "_logp"]) <= 1e-6
    assert close(q1, g[tag + "_q1"]) <= 1e-6 and close(q2, g[tag + "_q2"]) <= 1e-6


@pytest.mark.parametrize("N,H,A,limit,det", [(200, 128, 24, 1.0, False), (100, 64, 128, 2.5, False), (37, 192, 3, 1.0, False),
                                             (64, 128, 17, 1.0, True)])
def test_cpu_build_against_float64(N, H, A, limit, det):
    L = _lib.lib_cpu()
    h, mw, mb, lw, lb = sc.problem(N, H, A, seed=N + A)
    counters = torch.arange(N, dtype=torch.int64) % 5
    z = torch.zeros(N, A) if det else sc.draws(L, -1, None, 77, counters, 3, N, A)
    out = sc.run(L, -1, None, h, mw, mb, lw, lb, act_limit=limit, deterministic=det, seed=77, counters=counters.clone(), row_offset=3)
    mu64, ls64, s_mu, _ = sc.f64_head(h, mw, mb, lw, lb)
    mu, ls = out["mu"].double().numpy(), out["log_std"].double().numpy()
    assert (np.abs(mu - mu64) <= 1e-6 * s_mu + 1e-30).all()      # an fmaf chain over k: <= H ulp of the row scale, far less in practice
    lo, hi = ls64 < -20.001, ls64 > 2.001
    assert lo.any() and hi.any()
    assert (ls[lo] == -20.0).all() and (ls[hi] == 2.0).all()      # the clamp is exact at both bounds
    assert (ls >= -20.0).all() and (ls <= 2.0).all()
    assert (np.abs(out["u"].numpy()).max(-1) >= 3).any()         # saturated rows are part of the check
    sc.check_epilogue(out, z, limit, 1e-6, det, "cpu")
    if det:
        assert torch.equal(out["u"], out["mu"])


def test_case_table_reaches_every_kernel():
    """The launcher's `switch` (NCT 2..16) times the WAVES its LDS clamp leaves, and both ways to 4 waves at NCT >= 10: an instantiation
    or a clamp changed there without a case fails here."""
    assert sc.coverage() == sc.REACHABLE and len(sc.REACHABLE) == 32 and len({k[:2] for k in sc.REACHABLE}) == 28
    assert sc.coverage(sc.OLD_SHAPES) == {(10, 4, True), (4, 8, False), (2, 4, False), (2, 1, False), (4, 2, False), (16, 1, False)}
    assert sc.expected_kernel(512, 128) == (16, 4, True) and sc.expected_kernel(256, 128) == (16, 4, False)
    assert sc.expected_kernel(512, 64) == (8, 8, False) and sc.expected_kernel(768, 113) == (16, 4, False)
    for t in range(1, 9):            # each NCT with a full last column tile per head and with one live column in it
        assert {A for _, _, A in sc.CASES if (A + 15) // 16 == t} >= {16 * t, 16 * (t - 1) + 1}


@pytest.mark.parametrize("N,H,A", sc.CASES)
def test_kernel_table(N, H, A):
    sc.check_case(_lib.lib_cpu(), -1, None, "cpu", N, H, A)


@pytest.mark.parametrize("mutation", ["tile", "last"])
def test_gate_sees_a_dropped_tile_or_column(mutation):
    """The float64 side without each head's last column tile, or without its last column, at NCT = 16: the gate of the products is
    missed at least ten times over."""
    L = _lib.lib_cpu()
    assert sc.check_kernel(L, -1, None, "cpu", 33, 768, 113, mutation=mutation) >= 10
    assert sc.check_kernel(L, -1, None, "cpu", 17, 256, 128, mutation=mutation) >= 10


def test_counters_and_draws():
    L = _lib.lib_cpu()
    N, H, A = 1000, 64, 9
    h, mw, mb, lw, lb = sc.problem(N, H, A, seed=3, scaled=False)
    c0 = (torch.arange(N, dtype=torch.int64) * 7) % 11
    c = c0.clone()
    first = sc.run(L, -1, None, h, mw, mb, lw, lb, seed=5, counters=c)
    assert torch.equal(c, c0 + 1)                                 # a sample call advances every row by exactly one
    sc.run(L, -1, None, h, mw, mb, lw, lb, seed=5, counters=c, deterministic=True)
    assert torch.equal(c, c0 + 1)                                 # deterministic calls draw nothing
    second = sc.run(L, -1, None, h, mw, mb, lw, lb, seed=5, counters=c)
    assert torch.equal(c, c0 + 2) and not torch.equal(first["u"], second["u"])
    # the first 64 rows of the 1000-row call equal a 64-row call with the same counters
    part = sc.run(L, -1, None, h[:64], mw, mb, lw, lb, seed=5, counters=c0[:64].clone())
    for k in ("u", "action", "logp"):
        assert torch.equal(part[k], first[k][:64]), k
    # equal (seed, row_offset + row, counter): equal draws, wherever the row sits in the call
    z = sc.draws(L, -1, None, 5, c0, 0, N, A)
    z_shift = sc.draws(L, -1, None, 5, c0[100:], 100, N - 100, A)
    assert torch.equal(z_shift, z[100:])
    assert not torch.equal(sc.draws(L, -1, None, 6, c0, 0, N, A), z)                     # another seed, another stream
    assert not torch.equal(sc.draws(L, -1, None, 5, c0[100:], 0, N - 100, A), z[100:])   # another global row, another stream


def test_module_semantics():
    ac = _ac(12, 4, (64, 64), seed=9)
    assert ac.pi.seed == 9 and ac.pi.row_offset == 0
    c = ac.pi.counters(10, "cpu")
    c += 3
    assert ac.pi.counters(4, "cpu") is c                          # large enough: kept
    grown = ac.pi.counters(20, "cpu")
    assert grown.numel() == 20 and (grown[:10] == 3).all() and (grown[10:] == 0).all()   # grown, what was drawn kept
    keys = list(ac.state_dict().keys())
    assert not any("counter" in k for k in keys) and all(k.split(".")[0] in ("pi", "q1", "q2") for k in keys)
    twin = copy.deepcopy(ac)                                      # sac.py: actor_critic_targ = deepcopy(actor_critic)
    assert torch.equal(twin.pi._counters, ac.pi._counters) and twin.pi._counters.data_ptr() != ac.pi._counters.data_ptr()
    assert list(twin.state_dict().keys()) == keys and twin.pi.seed == ac.pi.seed
    moved = ac.to("cpu").to(torch.float64)
    assert list(moved.state_dict().keys()) == keys and moved.pi.mu_layer.weight.dtype == torch.float64
    ac = _ac(12, 4, (64, 64)).float()
    o = torch.randn(3, 5, 12)
    a, logp = ac.pi(o)                                            # grad enabled: the torch path, differentiable
    assert a.requires_grad and logp.requires_grad and a.shape == (3, 5, 4) and logp.shape == (3, 5, 1)
    logp.sum().backward()
    assert ac.pi.mu_layer.weight.grad is not None
    a, logp = ac.pi(o, with_logprob=False)
    assert logp is None
    assert not ac.act(o).requires_grad and (ac.act(o).abs() <= 1).all()
    torch.manual_seed(4)
    s1 = _ac(12, 4, (64, 64)).pi.seed
    torch.manual_seed(4)
    assert _ac(12, 4, (64, 64)).pi.seed == s1                     # the default seed follows torch.manual_seed
    assert ReplayBuffer is DDPGReplayBuffer


def test_counters_keep_their_address_once_a_capture_holds_them():
    """A captured graph holds the counters' device address only: once pinned (what a capture does) they must never move."""
    pi = _ac(12, 4, (64, 64)).pi
    c = pi.counters(10, "cpu")
    c += 2
    ptr = c.data_ptr()
    assert pi.counters(5, "cpu").data_ptr() == ptr                # smaller calls use the same tensor
    c = pi.reserve_counters(80, "cpu")                            # not pinned yet: grows, keeps what was drawn
    assert c.numel() == 80 and (c[:10] == 2).all() and (c[10:] == 0).all()
    ptr = c.data_ptr()
    pi._counters_pinned = True                                    # set by _fused when it runs inside a graph capture
    assert pi.counters(80, "cpu").data_ptr() == ptr and pi.counters(3, "cpu").data_ptr() == ptr
    with pytest.raises(RuntimeError, match="reserve_counters"):
        pi.counters(81, "cpu")                                    # SAC's pi(o2) at 8 x num_envs after capturing act at num_envs
    assert pi._counters.data_ptr() == ptr and pi._counters.numel() == 80
    assert copy.deepcopy(pi)._counters_pinned                     # a copy keeps the rule (conservative)


def test_abi_errors_cpu_build():
    L = _lib.lib_cpu()
    N, H, A = 8, 64, 4
    h, mw, mb, lw, lb = sc.problem(N, H, A, scaled=False)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    dst = [torch.full((N, A), 7.0) for _ in range(5)] + [torch.full((N,), 7.0)]
    counters = torch.zeros(N, dtype=torch.int64)

    def call(hidden=h, H=H, mw=mw, mb=mb, lw=lw, lb=lb, det=0, counters=counters, A=A, N=N, device=-1):
        return L.mms_sac_heads_act(device, p(hidden), H, p(mw), p(mb), p(lw), p(lb), 1.0, 1e-6, det, 1, p(counters), 0, p(dst[0]), p(dst[1]),
                                   p(dst[5]), p(dst[2]), p(dst[3]), p(dst[4]), N, A, None)

    bad = [dict(A=0), dict(A=129), dict(H=96), dict(H=0), dict(hidden=None), dict(mw=None), dict(mb=None), dict(lw=None), dict(lb=None),
           dict(counters=None), dict(N=-1), dict(device=0), dict(hidden=torch.zeros(N * H + 1)[1:])]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0 and _lib.last_error(None, L), kw
        assert all((d == 7.0).all() for d in dst) and (counters == 0).all(), kw
    assert "multiple of 64" in (call(H=96), _lib.last_error(None, L))[1]
    assert "aligned" in (call(hidden=torch.zeros(N * H + 1)[1:]), _lib.last_error(None, L))[1]
    assert call(counters=None, det=1) == 0 and (counters == 0).all()     # deterministic: counters are not needed
    assert call() == 0 and (counters == 1).all() and not (dst[5] == 7.0).any()

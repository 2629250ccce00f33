"""Checks of mms_sac_heads_act (include/mms.h) shared by the CPU-build tests (test_sac_actor.py) and the GPU tests
(test_sac_actor_gpu.py): the launch through ctypes, the float64 evaluation of SAC's head formulae (agents/algorithms/rl/sac/
module.py:31-61) and the error gates.

Gates.  The epilogue (clamp, exp, rsample, tanh, log-probability) is checked against float64 evaluated from the call's own mu and
log_std, so that the GEMM's rounding is judged separately.  The log-probability's tanh correction log(1 - t^2 + eps) amplifies an
error dt of t = tanh(u) by 2|t| / (1 - t^2 + eps) -- large near |t| = 1, where the reference's fp32 evaluation has the same
cancellation -- so a row's logp gate is sum_j (1e-4 + 2|t_j| dt_j / (1 - t_j^2 + eps)) with dt = 8 ulp(1) + (1 - t^2) |du| (a few
ulp of tanh plus the propagated difference of u): 1e-4 A plus little on rows with max|u| < 3."""
import ctypes

import numpy as np
import torch

from massive_marl_benchmark_amd import _lib

LOG_2PI_HALF = 0.5 * np.log(2.0 * np.pi)
ULP1 = 2.0 ** -24


def run(L, device, stream, hidden, mu_w, mu_b, ls_w, ls_b, *, act_limit=1.0, epsilon=1e-6, deterministic=False, seed=1, counters=None,
        row_offset=0, with_logp=True):
    """One mms_sac_heads_act call with every destination; returns a dict of the outputs (tensors on hidden's device)."""
    N, H = hidden.shape
    A = mu_w.shape[0]
    dev = hidden.device
    out = {k: torch.full((N, A), float("nan"), device=dev) for k in ("action", "act_slot", "u", "mu", "log_std")}
    out["logp"] = torch.full((N,), float("nan"), device=dev) if with_logp else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(L.mms_sac_heads_act(device, p(hidden), H, p(mu_w), p(mu_b), p(ls_w), p(ls_b), float(act_limit), float(epsilon), int(deterministic),
                                   seed, p(counters), row_offset, p(out["action"]), p(out["act_slot"]), p(out["logp"]), p(out["u"]), p(out["mu"]),
                                   p(out["log_std"]), N, A, stream), None, "mms_sac_heads_act", L)
    return out


def draws(L, device, stream, seed, counters, row_offset, N, A):
    """The standard normals a sample call with these counters uses: the same call on mu = 0, log_std = 0, where u = 0 + 1 * z = z
    exactly.  `counters` is not advanced (a copy is)."""
    dev = counters.device
    z64 = torch.zeros(N, 64, device=dev)
    w, b = torch.zeros(A, 64, device=dev), torch.zeros(A, device=dev)
    return run(L, device, stream, z64, w, b, w, b, seed=seed, counters=counters[:N].clone(), row_offset=row_offset, with_logp=False)["u"]


def f64_head(hidden, mu_w, mu_b, ls_w, ls_b):
    """mu and the unclamped log_std in float64, with the row scale sum_k |h_k w_jk| + |b_j| of each product."""
    h, mw, mb, lw, lb = (np.asarray(t.detach().cpu(), np.float64) for t in (hidden, mu_w, mu_b, ls_w, ls_b))
    mu, ls = h @ mw.T + mb, h @ lw.T + lb
    s_mu, s_ls = np.abs(h) @ np.abs(mw).T + np.abs(mb), np.abs(h) @ np.abs(lw).T + np.abs(lb)
    return mu, ls, s_mu, s_ls


def f64_epilogue(mu, log_std, z, act_limit, epsilon, deterministic):
    """The sampling epilogue in float64 from (fp32) mu, clamped log_std and the draws z."""
    mu, ls, z = (np.asarray(t, np.float64) for t in (mu, log_std, z))
    if deterministic:
        z = np.zeros_like(mu)
    u = mu + np.exp(ls) * z
    t = np.tanh(u)
    logp = (-0.5 * z * z - ls - LOG_2PI_HALF - np.log(1.0 - t * t + epsilon)).sum(-1)
    return u, t, act_limit * t, logp


def logp_gate(t, du, epsilon):
    t = np.asarray(t, np.float64)
    dt = 8 * ULP1 + (1.0 - t * t) * np.abs(du)
    return (1e-4 + 2.0 * np.abs(t) * dt / (1.0 - t * t + epsilon)).sum(-1)


def check_epilogue(out, z, act_limit, epsilon, deterministic, what=""):
    """The call's u / action / logp against the float64 epilogue of its own mu and log_std; returns the worst logp error over its gate."""
    np_ = lambda k: out[k].detach().cpu().numpy().astype(np.float64)
    mu, ls, u_k, act, logp = np_("mu"), np_("log_std"), np_("u"), np_("action"), np_("logp")
    u, t, act64, logp64 = f64_epilogue(mu, ls, z.cpu().numpy(), act_limit, epsilon, deterministic)
    du = np.abs(u_k - u)
    # fma rounding of u, and expf: the device's fast exp2(x log2 e) is off by up to ~|x| 2^-24 relative (x = log_std >= -20)
    assert (du <= 2.4e-7 * np.abs(u) + 2e-6 * np.exp(ls) * np.abs(z.cpu().numpy()) + 1e-30).all(), (what, du.max())
    assert (np.abs(act) <= act_limit).all(), what
    assert (np.abs(act - act64) <= act_limit * (8 * ULP1 + (1 - t * t) * du)).all(), (what, np.abs(act - act64).max())
    assert np.array_equal(np_("act_slot"), act), what
    gate = logp_gate(t, du, epsilon)
    ratio = np.abs(logp - logp64) / gate
    assert (ratio <= 1.0).all(), (what, ratio.max(), np.argmax(ratio))
    return float(ratio.max())


def problem(N, H, A, seed=0, device="cpu", scaled=True):
    """hidden [N,H] (ELU outputs; with `scaled`, every 8th row x 30 and every 8th + 4 x 300: log_std past both clamp bounds, tanh
    saturated) and the two heads' parameters at nn.Linear's scale."""
    g = torch.Generator().manual_seed(seed)
    h = torch.nn.functional.elu(torch.randn(N, H, generator=g))
    if scaled:
        h[0::8] *= 30.0
        h[4::8] *= 300.0
    k = H ** -0.5
    mk = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).to(device)
    return h.to(device), mk(A, H), mk(A), mk(A, H), mk(A)

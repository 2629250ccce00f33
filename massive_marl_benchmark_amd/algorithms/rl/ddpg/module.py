"""MLPActorCritic of DDPG (agents/algorithms/rl/ddpg/module.py:5-61): deterministic tanh actor scaled to the action limit, one Q
network on cat(obs, act), Gaussian exploration noise clipped to the limit.  Same constructor, sub-module names (state_dict keys
`pi.pi.<i>.*`, `q.q.<i>.*`) and `act(obs, deterministic)` contract, so ddpg.py uses it unchanged.

On the HIP device the actor's layers run as `mms_linear2_act` launches (fp32 MFMA, bias + ReLU / tanh in the epilogue) when the
network qualifies (fp32, ReLU / ELU / Tanh / Identity activations, input width a multiple of 4) -- the collection loop of
BASELINE configs[2] is a chain of small kernels and the library path spends three launches per layer.  The exploration noise is
drawn on the device (the reference draws it on the host and copies it over, module.py:59); a different stream of normals,
same distribution.

The critics.  Under no_grad on the HIP device (the Q target of every update: ddpg.py:368-369, td3.py:370-373, sac.py:379-382) an
`MLPQFunction` runs as launches of this build too: one `torch.cat`, every hidden Linear + activation through `mms_linear2_act`
and the last Linear(H, 1) through `mms_q_heads_backup` (`fused_q_forward`).  `MLPActorCritic.q_backup` is the one-call form of the
whole target: both critics of TD3 / SAC per launch, and the min and the Bellman backup inside the last one (`fused_q_backup`).
Wherever a gradient is wanted (the online critics of compute_loss_q, compute_loss_pi), on the CPU, or with shapes the kernels do
not take, the critics are the plain torch modules.  `fused_q=False` in the constructor means torch always.
"""
import ctypes

import torch
import torch.nn as nn

from .... import _lib
from ....engine import current_stream_ptr

_ACT_CODES = {nn.Identity: 0, nn.ELU: 1, nn.ReLU: 2, nn.Tanh: 3}
_Q_MAX_H = 4096          # include/mms.h: MMS_Q_MAX_H


def _kernel_layout(t):
    return t.is_contiguous() and t.data_ptr() % 16 == 0


def mlp(sizes, activation, output_activation=nn.Identity):
    """Linear layers sizes[0] -> ... -> sizes[-1], `activation` between them and `output_activation` at the end (module.py:5-10)."""
    mods = []
    last = len(sizes) - 2
    for j, (fan_in, fan_out) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(fan_in, fan_out))
        mods.append((output_activation if j == last else activation)())
    return nn.Sequential(*mods)


def fused_mlp_forward(seq, x):
    """`seq(x)` through mms_linear2_act, one launch per Linear + activation pair; None if `seq` does not qualify."""
    mods = list(seq)
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or len(mods) % 2 or torch.is_grad_enabled() and any(p.requires_grad for p in seq.parameters()):
        return None
    pairs = list(zip(mods[0::2], mods[1::2]))
    for lin, act in pairs:
        if not isinstance(lin, nn.Linear) or type(act) not in _ACT_CODES or lin.bias is None or lin.in_features % 4 or lin.weight.dtype != torch.float32:
            return None
        if isinstance(act, nn.ELU) and act.alpha != 1.0:
            return None
    dev = x.device
    L, idx, stream = _lib.for_device(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    h = x.contiguous()
    for lin, act in pairs:
        y = torch.empty(h.shape[0], lin.out_features, device=dev)
        _lib.check(L.mms_linear2_act(idx, h.shape[0], lin.out_features, lin.in_features, p(h), p(lin.weight.detach()), p(lin.bias.detach()), p(y),
                                     None, None, None, None, _ACT_CODES[type(act)], stream), None, "mms_linear2_act", L)
        h = y
    return h


def _q_chain(qs, obs, act):
    """The hidden layers of one or two MLPQFunctions of the same shape on cat(obs, act), both networks per mms_linear2_act launch.
    Returns (hidden activations per network [M, H], the last Linears, leading shape), or None if anything does not qualify --
    decided before the first launch, so there is never a partial fallback."""
    if len(qs) not in (1, 2) or not all(getattr(q, "fused_q", True) for q in qs):
        return None
    if not (obs.is_cuda and act.is_cuda and obs.dtype == torch.float32 and act.dtype == torch.float32 and obs.dim() >= 1 and obs.shape[:-1] == act.shape[:-1] and act.device == obs.device):
        return None
    if torch.is_grad_enabled() and (obs.requires_grad or act.requires_grad or any(p.requires_grad for q in qs for p in q.parameters())):
        return None
    nets = [list(q.q) for q in qs]
    if any(len(m) != len(nets[0]) or len(m) % 2 or len(m) < 2 for m in nets):
        return None
    for m in nets:
        for i in range(0, len(m), 2):
            lin, fn, lin0, fn0 = m[i], m[i + 1], nets[0][i], nets[0][i + 1]
            if not isinstance(lin, nn.Linear) or lin.bias is None or lin.weight.dtype != torch.float32 or lin.weight.device != obs.device:
                return None
            if not _kernel_layout(lin.weight) or not lin.bias.is_contiguous() or lin.bias.device != obs.device or lin.bias.dtype != torch.float32:
                return None                  # (e.g. parameters that are views into a flat buffer: the kernels read dense, 16-byte aligned weight rows)
            if type(fn) is not type(fn0) or (lin.in_features, lin.out_features) != (lin0.in_features, lin0.out_features):
                return None
            if i == len(m) - 2:      # Linear(H, 1), identity output: mms_q_heads_backup
                if type(fn) is not nn.Identity or lin.out_features != 1 or lin.in_features % 64 or lin.in_features > _Q_MAX_H:
                    return None
            elif type(fn) not in _ACT_CODES or lin.in_features % 4 or (isinstance(fn, nn.ELU) and fn.alpha != 1.0):
                return None
    if nets[0][0].in_features != obs.shape[-1] + act.shape[-1]:
        return None
    dev = obs.device
    L, idx, stream = _lib.for_device(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = torch.cat([obs, act], dim=-1)                      # ONE cat, shared by both networks
    lead = x.shape[:-1]
    x = x.reshape(-1, x.shape[-1])
    M, two = x.shape[0], len(qs) == 2
    hs = [x] * len(qs)
    for i in range(0, len(nets[0]) - 2, 2):
        lins = [m[i] for m in nets]
        ys = [torch.empty(M, lin.out_features, device=dev) for lin in lins]
        _lib.check(L.mms_linear2_act(idx, M, lins[0].out_features, lins[0].in_features, p(hs[0]), p(lins[0].weight.detach()), p(lins[0].bias.detach()),
                                     p(ys[0]), p(hs[1]) if two else None, p(lins[1].weight.detach()) if two else None,
                                     p(lins[1].bias.detach()) if two else None, p(ys[1]) if two else None, _ACT_CODES[type(nets[0][i + 1])], stream),
                   None, "mms_linear2_act", L)
        hs = ys
    return hs, [m[-2] for m in nets], lead


def _q_tail(hs, last, q_out, r=None, d=None, logp=None, gamma=0.0, alpha=0.0, backup=None):
    """mms_q_heads_backup on the chain's hidden activations."""
    L, idx, stream = _lib.for_device(hs[0].device)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    two = len(hs) == 2
    _lib.check(L.mms_q_heads_backup(idx, hs[0].shape[0], hs[0].shape[1], p(hs[0]), p(last[0].weight.detach()), p(last[0].bias.detach()), p(q_out[0]),
                                    p(hs[1]) if two else None, p(last[1].weight.detach()) if two else None, p(last[1].bias.detach()) if two else None,
                                    p(q_out[1]) if two else None, p(r), p(d), p(logp), float(gamma), float(alpha), p(backup), stream),
               None, "mms_q_heads_backup", L)


def fused_q_forward(qs, obs, act):
    """[q(obs, act) for q in qs] for one or two MLPQFunctions of the same shape, without torch's modules: one cat, one
    mms_linear2_act launch per hidden layer for both networks, one mms_q_heads_backup launch for the last layers.  For the HIP device,
    fp32, nothing wanting a gradient; returns None when anything does not qualify (the caller then runs the torch modules)."""
    chain = _q_chain(qs, obs, act)
    if chain is None:
        return None
    hs, last, lead = chain
    out = [torch.empty(hs[0].shape[0], device=hs[0].device) for _ in qs]
    _q_tail(hs, last, out)
    return [o.view(*lead, 1) for o in out]


@torch.no_grad()
def fused_q_backup(qs, obs, act, r, d, gamma, alpha=None, logp=None):
    """The Bellman backup r + gamma * (1 - d) * (min_g q_g(obs, act) - alpha * logp) in the shape of `r` (alpha / logp None: no
    entropy term -- TD3, DDPG), for the target critics `qs`.  On the HIP device the fused chain of fused_q_forward with the min and
    the backup inside its last launch; `d` as uint8 (what ReplayBuffer.dones holds) or bool is read as it is, any other dtype costs
    one ne(0).  Where the chain does not apply, the reference's expression in torch.  No gradient
    either way (the reference evaluates the target under no_grad)."""
    if (alpha is None) != (logp is None):
        raise ValueError("fused_q_backup: alpha and logp come together")
    M = r.numel()
    fits = r.is_cuda and r.dtype == torch.float32 and d.numel() == M and d.device == r.device and obs.shape[:-1].numel() == M and (
        logp is None or (logp.numel() == M and logp.dtype == torch.float32 and logp.device == r.device))
    chain = _q_chain(qs, obs, act) if fits else None
    if chain is None:
        q = qs[0](obs, act)
        for other in qs[1:]:
            q = torch.min(q, other(obs, act))
        if not d.is_floating_point():
            d = d.to(r.dtype)                  # torch has no `1 - bool`
        if logp is None:
            return r + gamma * (1 - d) * q
        return r + gamma * (1 - d) * (q - alpha * logp)
    hs, last, _ = chain
    if d.dtype not in (torch.uint8, torch.bool):
        d = d.ne(0)
    d8 = d.contiguous()
    d8 = d8.view(torch.uint8) if d8.dtype == torch.bool else d8
    backup = torch.empty(r.shape, device=r.device)
    _q_tail(hs, last, [None] * len(qs), r.contiguous(), d8, None if logp is None else logp.contiguous(), gamma, 0.0 if alpha is None else alpha, backup)
    return backup


class MLPActor(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit):
        super().__init__()
        self.pi = mlp([obs_dim, *hidden_sizes, act_dim], activation, nn.Tanh)
        self.act_limit = act_limit

    def forward(self, obs):
        out = fused_mlp_forward(self.pi, obs)
        if out is None:
            out = self.pi(obs)
        return out if self.act_limit == 1.0 else self.act_limit * out       # x 1.0 is exact: one launch less for the ant / helicopter tasks


class MLPQFunction(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, fused_q=True):
        super().__init__()
        self.q = mlp([obs_dim + act_dim, *hidden_sizes, 1], activation)
        self.fused_q = bool(fused_q)       # False: torch always

    def forward(self, obs, act):
        out = fused_q_forward([self], obs, act) if self.fused_q else None
        if out is not None:
            return out[0]
        return self.q(torch.cat([obs, act], dim=-1))      # [..., 1], as the reference returns it


class MLPActorCritic(nn.Module):
    def __init__(self, observation_space, action_space, act_noise, device, hidden_sizes=(256, 256), activation=nn.ReLU, fused_q=True):
        super().__init__()
        self.fused_q = bool(fused_q)
        obs_dim, act_dim = observation_space.shape[0], action_space.shape[0]
        self.act_limit = action_space.high[0]
        self.act_noise = act_noise
        self.device = device
        self.pi = MLPActor(obs_dim, act_dim, hidden_sizes, activation, self.act_limit)
        self._build_q(obs_dim, act_dim, hidden_sizes, activation)

    def _build_q(self, obs_dim, act_dim, hidden_sizes, activation):
        self.q = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q)

    def _critics(self):
        return [self.q]

    def q_backup(self, o2, a2, r, d, gamma, alpha=None, logp=None):
        """r + gamma * (1 - d) * (min over this network's critics of q(o2, a2) - alpha * logp), no gradient: called on the target
        copy it is ddpg.py:368-369 / td3.py:370-373 in one line (see fused_q_backup)."""
        return fused_q_backup(self._critics(), o2, a2, r, d, gamma, alpha, logp)

    def act(self, obs, deterministic=True):
        with torch.no_grad():
            a = self.pi(obs)
            if not deterministic:
                if a.is_cuda:      # mean + std * N(0, 1) in one launch, clamp in place (the collection loop is launch bound)
                    a = torch.normal(a, float(self.act_noise)).clamp_(-self.act_limit, self.act_limit)
                else:
                    a = torch.clamp(a + self.act_noise * torch.randn_like(a), -self.act_limit, self.act_limit)
        return a

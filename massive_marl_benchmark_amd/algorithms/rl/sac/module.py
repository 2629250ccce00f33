"""MLPActorCritic of SAC (agents/algorithms/rl/sac/module.py:23-99): a squashed-Gaussian actor (`pi`: `net`, `mu_layer`,
`log_std_layer`) and twin Q networks (`q1`, `q2`).  Same constructor, sub-module names (state_dict keys `pi.net.<i>.*`,
`pi.mu_layer.*`, `pi.log_std_layer.*`, `q1.q.<i>.*`, `q2.q.<i>.*`), `act_limit` attribute and `forward(obs, deterministic,
with_logprob, epsilon)` / `act(obs, deterministic)` contracts, so sac.py uses it unchanged.

When no gradient is wanted on the HIP device (the collection's `act`, sac.py:166, and the Q target's `pi(o2)` under no_grad,
sac.py:374-376), the actor runs as launches of this build: the hidden layers through `mms_linear2_act` (ddpg.module.fused_mlp_forward)
and the head -- mu_layer, log_std_layer, clamp, rsample, the tanh-corrected log-probability and the scaled action -- as ONE
`mms_sac_heads_act` launch.  Anything else (autograd for compute_loss_pi, the CPU, other dtypes, shapes the kernels do not take)
is plain torch with the same formulae.  The critics under no_grad run fused as well (`MLPQFunction.forward`, `q_backup`: see
ddpg.module); `fused_q=False` keeps them on torch.

`layers="f16x2"` (constructor keyword of SquashedGaussianMLPActor, MLPQFunction and MLPActorCritic, which hands it down; default
"fp32" = everything above, launch for launch and bit for bit): the hidden layers of those fused paths -- `net` in front of
`mms_sac_heads_act`, the critics' hidden layers in front of `mms_q_heads_backup`, on (obs, act) without the cat -- run on the two-plane
fp16 kernel through ddpg.module.split16_hidden.  include/mms.h on what that trades: "the operand is kept to 2^-22 |x| (worst case;
4e-8 rms) instead of exactly", relative to its row's bound.  The weights' planes are rebuilt on every call, so in-place parameter
updates (optimizer, polyak) are always followed; shapes the kernel does not take run the "fp32" chain.  The heads, the sampling and
the per-row counters are the same launches either way.

The noise of the fused path is this build's counter-based generator (seed, global row = row_offset + row, per-row draw counter),
not torch's Philox: sampled actions differ from the reference's draw for the same torch seed, their distribution and
log-probabilities do not.  The per-row counters are a plain device tensor (not a buffer: state_dict keys stay the reference's),
grown to the largest row count seen.  A captured graph holds only the counters' device address, so once a graph capture has used
them they are pinned: a call that would need more rows (or another device) raises instead of moving them.  Before capturing, size
them for every row count the actor will see -- `pi.reserve_counters(8 * num_envs, device)` for SAC, whose Q target calls the same
actor on 8 ring rows x num_envs (sac.py:374-376).  `deepcopy` (sac.py's actor_critic_targ) copies seed and counters: a sampled call
of the copy draws the same noise as the original would (sac.py never samples from the target actor).
"""
import ctypes
import math

import torch
import torch.nn as nn

from .... import _lib
from ..ddpg.module import LAYERS, _Split16Owner, fused_mlp_forward, fused_q_backup, fused_q_forward, mlp, split16_hidden

LOG_STD_MAX = 2
LOG_STD_MIN = -20
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _draw_seed():
    """A noise-stream key from torch's default generator, so that torch.manual_seed makes runs reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class SquashedGaussianMLPActor(_Split16Owner, nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit, seed=None, row_offset=0, layers="fp32"):
        super().__init__()
        self._init_layers(layers)          # "f16x2": `net` through split16_hidden (module docstring)
        self.net = mlp([obs_dim] + list(hidden_sizes), activation, activation)
        self.mu_layer = nn.Linear(hidden_sizes[-1], act_dim)
        self.log_std_layer = nn.Linear(hidden_sizes[-1], act_dim)
        self.act_limit = act_limit
        self.seed = _draw_seed() if seed is None else int(seed)    # drawn after the layers: their initialisation is the reference's
        self.row_offset = int(row_offset)                           # global index of row 0 (data-parallel shards draw disjoint rows)
        self._counters = None
        self._counters_pinned = False      # a graph capture has used the counters: their address must not change

    def reserve_counters(self, n, device):
        """Size the per-row draw counters for n rows on `device` now (before a graph capture); returns them."""
        return self.counters(n, device)

    def counters(self, n, device):
        """The per-row draw counters on `device`, at least n of them (grown on demand; what was drawn so far is kept).  Once pinned
        by a graph capture they are never reallocated: a request they cannot serve raises."""
        c = self._counters
        if c is None or c.device != torch.device(device) or c.numel() < n:
            capturing = torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()
            if self._counters_pinned or capturing:     # (allocated inside a capture, the zero fill would replay with the graph)
                raise RuntimeError("SquashedGaussianMLPActor: %d rows on %s need new draw counters, but a graph capture holds or is recording the current "
                                   "ones (%s); call pi.reserve_counters(<largest row count>, device) before capturing"
                                   % (n, torch.device(device), "none" if c is None else "%d on %s" % (c.numel(), c.device)))
            old = None if c is None else c.to(device)
            c = torch.zeros(max(n, 0 if old is None else old.numel()), dtype=torch.int64, device=device)
            if old is not None:
                c[:old.numel()].copy_(old)
            self._counters = c
        return c

    def _fusable(self, obs):
        if not obs.is_cuda or obs.dtype != torch.float32 or obs.dim() < 1:
            return False
        if torch.is_grad_enabled() and (obs.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        H, A = self.mu_layer.in_features, self.mu_layer.out_features
        return H % 64 == 0 and 1 <= A <= 128 and all(p.dtype == torch.float32 and p.is_cuda
                                                       for p in (*self.mu_layer.parameters(), *self.log_std_layer.parameters()))

    def _fused(self, obs, deterministic, with_logprob, epsilon):
        """The forward through mms_linear2_act + mms_sac_heads_act; None where the hidden layers do not qualify."""
        lead = obs.shape[:-1]
        x = obs.reshape(-1, obs.shape[-1])
        hidden = None
        if self.layers == "f16x2":
            hs = split16_hidden([self.net], x, self._split16_scratch)
            hidden = None if hs is None else hs[0]
        if hidden is None:
            hidden = fused_mlp_forward(self.net, x)
        if hidden is None:
            return None
        N, A = hidden.shape[0], self.mu_layer.out_features
        dev = hidden.device
        L, idx, stream = _lib.for_device(dev)
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        act = torch.empty(N, A, device=dev)
        logp = torch.empty(N, device=dev) if with_logprob else None
        counters = None if deterministic else self.counters(N, dev)
        if counters is not None and torch.cuda.is_current_stream_capturing():
            self._counters_pinned = True
        _lib.check(L.mms_sac_heads_act(idx, p(hidden), hidden.shape[1], p(self.mu_layer.weight.detach()), p(self.mu_layer.bias.detach()),
                                       p(self.log_std_layer.weight.detach()), p(self.log_std_layer.bias.detach()), float(self.act_limit),
                                       float(epsilon), int(bool(deterministic)), self.seed, p(counters), self.row_offset, p(act), None, p(logp),
                                       None, None, None, N, A, stream), None, "mms_sac_heads_act", L)
        return act.view(*lead, A), (None if logp is None else logp.view(*lead, 1))

    def torch_forward(self, obs, deterministic=False, with_logprob=True, epsilon=1e-6, eps=None):
        """The forward in plain torch (module.py:31-61); `eps` (the standard normals of the rsample) is drawn by torch when None."""
        net_out = self.net(obs)
        mu = self.mu_layer(net_out)
        log_std = torch.clamp(self.log_std_layer(net_out), LOG_STD_MIN, LOG_STD_MAX)
        std = torch.exp(log_std)
        if deterministic:
            z = torch.zeros_like(mu)
            u = mu
        else:
            z = torch.randn_like(mu) if eps is None else eps
            u = mu + z * std
        logp = None
        if with_logprob:
            # Normal(mu, std).log_prob(u) with (u - mu) / std = z, and the tanh correction (SAC paper, appendix C)
            logp = (-0.5 * z * z - log_std - _HALF_LOG_2PI - torch.log(1 - torch.tanh(u).pow(2) + epsilon)).sum(dim=-1, keepdim=True)
        return self.act_limit * torch.tanh(u), logp

    def forward(self, obs, deterministic=False, with_logprob=True, epsilon=1e-6):
        if self._fusable(obs):
            out = self._fused(obs, deterministic, with_logprob, epsilon)
            if out is not None:
                return out
        return self.torch_forward(obs, deterministic, with_logprob, epsilon)


class MLPQFunction(_Split16Owner, nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, fused_q=True, layers="fp32"):
        super().__init__()
        self.q = mlp([obs_dim + act_dim] + list(hidden_sizes) + [1], activation)
        self.fused_q = bool(fused_q)       # False: torch always
        self._init_layers(layers)          # "f16x2": the fused paths' hidden layers through split16_hidden on (obs, act), no cat

    def forward(self, obs, act):
        out = fused_q_forward([self], obs, act) if self.fused_q else None      # no gradient wanted on the HIP device: ddpg.module
        if out is not None:
            return out[0]
        return self.q(torch.cat([obs, act], dim=-1))      # [..., 1], as the reference returns it


class MLPActorCritic(nn.Module):
    def __init__(self, observation_space, action_space, hidden_sizes=(256, 256), activation=nn.ELU, seed=None, row_offset=0, layers="fp32", fused_q=True):
        super().__init__()
        if layers not in LAYERS:
            raise ValueError("layers must be one of %s, not %r" % (LAYERS, layers))
        self.layers = layers               # handed down to the actor and both critics
        obs_dim, act_dim = observation_space.shape[0], action_space.shape[0]
        act_limit = action_space.high[0]
        self.pi = SquashedGaussianMLPActor(obs_dim, act_dim, hidden_sizes, activation, act_limit, seed=0, row_offset=row_offset, layers=layers)
        self.fused_q = bool(fused_q)
        self.q1 = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, layers)
        self.q2 = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, layers)
        self.pi.seed = _draw_seed() if seed is None else int(seed)  # after every layer: initialisation identical to the reference's

    def q_backup(self, o2, a2, r, d, gamma, alpha=None, logp=None):
        """r + gamma * (1 - d) * (min(q1(o2, a2), q2(o2, a2)) - alpha * logp), no gradient: called on the target copy it is
        sac.py:379-382 in one line -- both critics per launch, the min and the backup inside the last one (ddpg.module.fused_q_backup)."""
        return fused_q_backup([self.q1, self.q2], o2, a2, r, d, gamma, alpha, logp)

    def act(self, obs, deterministic=False):
        with torch.no_grad():
            a, _ = self.pi(obs, deterministic, False)
            return a.detach()

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

`fused_grad=True` (constructor keyword of SquashedGaussianMLPActor and MLPActorCritic, which hands it down; default False = everything
above): when a gradient IS wanted -- compute_loss_pi, sac.py:392-403 -- `net` still runs in torch, and the head behind it is one
`mms_sac_heads_act` launch forward and one `mms_sac_heads_grad` call plus three library products backward (`_SacHead`), on "cuda" and,
through the CPU build, on "cpu".  What it trades: the noise is the counter stream described below (torch_forward draws torch.randn),
counters advancing once per sampled call as in the no-grad path; and where log_std_layer's raw output EQUALS a clamp bound
torch.clamp passes the gradient while this gives none (a measure-zero tie, include/mms.h).  The backward is once-differentiable.  A
head that does not qualify (dtype, alignment, H % 64, A > 128) runs torch_forward exactly as with False.

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
from ..ddpg.module import LAYERS, _NoiseOwner, _Split16Owner, _draw_seed, fused_mlp_forward, fused_q_backup, fused_q_forward, mlp, split16_hidden
from .loss import q_heads_loss
from ..ppo.loss import _p, _workspace       # (the device's cached, 256-byte aligned workspace: one per process, calls run in stream order)

LOG_STD_MAX = 2
LOG_STD_MIN = -20
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class _SacHead(torch.autograd.Function):
    """The head behind `net` with a gradient (`fused_grad=True`): mms_sac_heads_act forward with u, mu and the clamped log_std kept,
    mms_sac_heads_grad + three library products backward.  Returns (action [N,A],) or (action, logp [N])."""

    @staticmethod
    def forward(ctx, hidden, mu_w, mu_b, ls_w, ls_b, act_limit, epsilon, deterministic, with_logprob, seed, counters, row_offset):
        N, H = hidden.shape
        A = mu_w.shape[0]
        dev = hidden.device
        L, idx, stream = _lib.for_device(dev)
        act, u, mu, ls = (torch.empty(N, A, device=dev) for _ in range(4))
        logp = torch.empty(N, device=dev) if with_logprob else None
        _lib.check(L.mms_sac_heads_act(idx, _p(hidden), H, _p(mu_w), _p(mu_b), _p(ls_w), _p(ls_b), act_limit, epsilon, int(deterministic), seed,
                                       _p(counters), row_offset, _p(act), None, _p(logp), _p(u), _p(mu), _p(ls), N, A, stream), None,
                   "mms_sac_heads_act", L)
        ctx.save_for_backward(hidden, mu_w, ls_w, u, mu, ls)
        ctx.scalars = (act_limit, epsilon)
        ctx.set_materialize_grads(False)           # an output the loss does not use arrives as None: the entry takes NULL for it
        return (act, logp) if with_logprob else (act,)

    @staticmethod
    def backward(ctx, g_act, g_logp=None):
        # once_differentiable alone raises only where an incoming gradient itself requires one; under create_graph=True with constant
        # incoming gradients it would hand back a silently constant head: refuse that as well
        if torch.is_grad_enabled():
            raise RuntimeError("SquashedGaussianMLPActor(fused_grad=True): the fused head is once differentiable (no create_graph=True)")
        return _SacHead._backward(ctx, g_act, g_logp)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _backward(ctx, g_act, g_logp):
        hidden, mu_w, ls_w, u, mu, ls = ctx.saved_tensors
        need = ctx.needs_input_grad
        if g_act is None and g_logp is None:
            return (None,) * 12
        N, A = u.shape
        dev = u.device
        # (a .mean() or .sum() upstream delivers a stride-0 expanded tensor)
        g_act = None if g_act is None else g_act.to(torch.float32).contiguous()
        g_logp = None if g_logp is None else g_logp.to(torch.float32).contiguous()
        L, idx, stream = _lib.for_device(dev)
        dy = torch.empty(N, 2 * A, device=dev)
        dbias = torch.empty(2 * A, device=dev) if (need[2] or need[4]) else None
        nbytes = ctypes.c_int64(-1)
        head = (idx, N, A, ctx.scalars[0], ctx.scalars[1], _p(u), _p(mu), _p(ls), _p(g_act), _p(g_logp), _p(dy), _p(dbias))
        _lib.check(L.mms_sac_heads_grad(*head, None, ctypes.byref(nbytes), stream), None, "mms_sac_heads_grad size query", L)
        ws = _workspace(nbytes.value, dev)
        _lib.check(L.mms_sac_heads_grad(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_sac_heads_grad", L)
        g_hidden = dy @ torch.cat([mu_w, ls_w], 0) if need[0] else None
        g_w = dy.t() @ hidden if (need[1] or need[3]) else None
        return (g_hidden, g_w[:A] if need[1] else None, dbias[:A] if need[2] else None, g_w[A:] if need[3] else None,
                dbias[A:] if need[4] else None) + (None,) * 7


class SquashedGaussianMLPActor(_NoiseOwner, _Split16Owner, nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit, seed=None, row_offset=0, fused_grad=False, layers="fp32"):
        super().__init__()
        self._init_layers(layers)          # "f16x2": `net` through split16_hidden (module docstring)
        self.fused_grad = bool(fused_grad)  # True: the head WITH a gradient through mms_sac_heads_act / mms_sac_heads_grad (module docstring)
        self.net = mlp([obs_dim] + list(hidden_sizes), activation, activation)
        self.mu_layer = nn.Linear(hidden_sizes[-1], act_dim)
        self.log_std_layer = nn.Linear(hidden_sizes[-1], act_dim)
        self.act_limit = act_limit
        # (ddpg.module._NoiseOwner: seed, row_offset, the per-row draw counters) drawn after the layers: their initialisation is the reference's
        self._init_noise(_draw_seed() if seed is None else seed, row_offset)

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

    def _grad_fusable(self, obs):
        """`fused_grad=True`, a gradient is wanted and the head qualifies for _SacHead: fp32, contiguous, 16-byte aligned mu_layer /
        log_std_layer on "cuda" or "cpu", H % 64 == 0, 1 <= A <= 128, a non-empty fp32 input on the parameters' device."""
        if not self.fused_grad or not torch.is_grad_enabled() or obs.dtype != torch.float32 or obs.dim() < 1 or obs.numel() == 0:
            return False
        if not (obs.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        head = (self.mu_layer.weight, self.mu_layer.bias, self.log_std_layer.weight, self.log_std_layer.bias)
        dev = head[0].device
        H, A = self.mu_layer.in_features, self.mu_layer.out_features
        return (dev.type in ("cuda", "cpu") and obs.device == dev and H % 64 == 0 and 1 <= A <= 128
                and all(p.dtype == torch.float32 and p.device == dev and p.is_contiguous() and p.data_ptr() % 16 == 0 for p in head))

    def _fused_with_grad(self, obs, deterministic, with_logprob, epsilon):
        """`net` in torch (autograd keeps it), the head through _SacHead; noise and counters as in _fused."""
        lead = obs.shape[:-1]
        hidden = self.net(obs.reshape(-1, obs.shape[-1])).contiguous()
        if hidden.data_ptr() % 16:
            hidden = hidden.clone()
        N, A = hidden.shape[0], self.mu_layer.out_features
        counters = None if deterministic else self.counters(N, hidden.device)
        if counters is not None and hidden.is_cuda and torch.cuda.is_current_stream_capturing():
            self._counters_pinned = True
        out = _SacHead.apply(hidden, self.mu_layer.weight, self.mu_layer.bias, self.log_std_layer.weight, self.log_std_layer.bias,
                             float(self.act_limit), float(epsilon), bool(deterministic), bool(with_logprob), self.seed, counters, self.row_offset)
        return out[0].view(*lead, A), (out[1].view(*lead, 1) if with_logprob else None)

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

    def forward(self, obs, deterministic=False, with_logprob=True, epsilon=1e-6, eps=None):
        if eps is not None:                # given standard normals (a recorded rsample): torch_forward's statements on them
            return self.torch_forward(obs, deterministic, with_logprob, epsilon, eps)
        if self._fusable(obs):
            out = self._fused(obs, deterministic, with_logprob, epsilon)
            if out is not None:
                return out
        if self._grad_fusable(obs):
            return self._fused_with_grad(obs, deterministic, with_logprob, epsilon)
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
    def __init__(self, observation_space, action_space, hidden_sizes=(256, 256), activation=nn.ELU, seed=None, row_offset=0, layers="fp32", fused_grad=False,
                 fused_q=True):
        super().__init__()
        if layers not in LAYERS:
            raise ValueError("layers must be one of %s, not %r" % (LAYERS, layers))
        self.layers = layers               # handed down to the actor and both critics
        obs_dim, act_dim = observation_space.shape[0], action_space.shape[0]
        act_limit = action_space.high[0]
        self.pi = SquashedGaussianMLPActor(obs_dim, act_dim, hidden_sizes, activation, act_limit, seed=0, row_offset=row_offset, layers=layers,
                                           fused_grad=fused_grad)
        self.fused_q = bool(fused_q)
        self.q1 = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, layers)
        self.q2 = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, layers)
        self.pi.seed = _draw_seed() if seed is None else int(seed)  # after every layer: initialisation identical to the reference's

    def q_backup(self, o2, a2, r, d, gamma, alpha=None, logp=None):
        """r + gamma * (1 - d) * (min(q1(o2, a2), q2(o2, a2)) - alpha * logp), no gradient: called on the target copy it is
        sac.py:379-382 in one line -- both critics per launch, the min and the backup inside the last one (ddpg.module.fused_q_backup)."""
        return fused_q_backup([self.q1, self.q2], o2, a2, r, d, gamma, alpha, logp)

    def q_loss(self, o, a, backup):
        """compute_loss_q's loss for a given Bellman backup (sac.py:370-371, 385-387): mean((q1 - backup)^2) + mean((q2 - backup)^2).
        The critics' hidden layers run in torch on cat(o, a) (autograd keeps them, their products stay with the library); both last
        layers, the loss and their backward are one mms_q_heads_loss call (loss.q_heads_loss)."""
        x = torch.cat([o, a], dim=-1)
        x = x.reshape(-1, x.shape[-1])
        return q_heads_loss([q.q[:-2](x) for q in (self.q1, self.q2)], [self.q1.q[-2], self.q2.q[-2]], target=backup, mode="mse")

    def pi_loss(self, o, alpha):
        """compute_loss_pi (sac.py:392-403): mean(alpha logp_pi - min(q1(o, pi), q2(o, pi))) with pi, logp_pi = self.pi(o).  The actor
        and the critics' hidden layers as in q_loss; the critics' last layers, the min, the mean and their backward are one
        mms_q_heads_loss call.  Critics whose parameters do not require a gradient get none computed."""
        pi, logp = self.pi(o)
        x = torch.cat([o, pi], dim=-1)
        x = x.reshape(-1, x.shape[-1])
        return q_heads_loss([q.q[:-2](x) for q in (self.q1, self.q2)], [self.q1.q[-2], self.q2.q[-2]], logp=logp.reshape(-1), alpha=alpha, mode="pi")

    def act(self, obs, deterministic=False):
        with torch.no_grad():
            a, _ = self.pi(obs, deterministic, False)
            return a.detach()

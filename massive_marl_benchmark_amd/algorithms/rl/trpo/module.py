"""ActorCritic for TRPO (agents/algorithms/rl/trpo/module.py, which is PPO's module.py) with the actor's first- and second-order
backward passes on this build's kernels.

Everything is PPO's ActorCritic (same constructor, state_dict keys, `act`, `act_inference`, fused rollout path) except `evaluate`:
when the actor qualifies, `mu` comes from `_ActorMLP`, an autograd Function whose forward runs the layers through mms_linear2_act and
whose backward is `_ActorMLPGrad` (mms_mlp_grad: J^T g).  `_ActorMLPGrad` is itself differentiable once, by the R-op mms_mlp_grad_rop,
so the reference's unmodified `kl_hessian_times_vector` (trpo.py:417-435) lands on the kernels:
  grad(kl, actor.parameters(), create_graph=True)  ->  _ActorMLP.backward  ->  _ActorMLPGrad (recorded, with d_l / e_l saved)
  grad(sum(flat_grad_kl * v), actor.parameters())  ->  _ActorMLPGrad.backward(v): J v as the gradient of g (torch carries it through
      the KL's elementwise graph and back into _ActorMLP.backward: the Gauss-Newton term) and sum_rows g . (d2 mu) v as the parameters'
      gradient (the curvature term, non-zero once mu != old_mu).
The sum is the exact Hessian-vector product of the reference's KL.  Log-probability, entropy, log_std and the critic stay the PPO
module's closed-form torch.  Anything the kernels do not take falls back to exactly PPO's `evaluate`.
"""
import ctypes
import math

import torch
import torch.nn as nn

from .... import _lib
from ..ppo.module import ActorCritic as _PPOActorCritic


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ptrs(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


class _Net:
    """The saved state of one actor forward: input, hidden activations, parameters, widths."""

    def __init__(self, x, hs, params, dims):
        self.x, self.hs, self.params, self.dims = x, hs, params, dims

    @property
    def L(self):
        return len(self.dims) - 1

    def workspace(self, which, L, idx, stream):
        fn = L.mms_mlp_grad if which == "grad" else L.mms_mlp_grad_rop
        dims = (ctypes.c_int32 * len(self.dims))(*self.dims)
        nbytes = ctypes.c_int64(0)
        nulls = [None] * (8 if which == "grad" else 11)               # the data pointers; workspace NULL = the size query
        _lib.check(fn(idx, self.L, self.x.shape[0], dims, *nulls, None, ctypes.byref(nbytes), stream), None, "%s size query" % fn.__name__, L)
        ws = torch.empty(max(int(nbytes.value), 256), dtype=torch.uint8, device=self.x.device)
        return dims, ws, ctypes.c_int64(ws.numel())


def _grad(net, g, save):
    """mms_mlp_grad: the parameters' gradients [dW_1, db_1, ...] for mu's gradient g; with save, also d_l and e_l (l < L)."""
    L, idx, stream = _lib.for_device(g.device)
    M, n = g.shape[0], net.dims
    W = net.params[0::2]
    dw = [torch.empty_like(w) for w in W]
    db = [torch.empty_like(b) for b in net.params[1::2]]
    d = [torch.empty(M, n[l], device=g.device) for l in range(1, net.L)] if save else None
    e = [torch.empty(M, n[l], device=g.device) for l in range(1, net.L)] if save else None
    dims, ws, nbytes = net.workspace("grad", L, idx, stream)
    _lib.check(L.mms_mlp_grad(idx, net.L, M, dims, _p(net.x), _ptrs(net.hs), _ptrs(W), _p(g), _ptrs(dw), _ptrs(db), _ptrs(d) if save else None,
                              _ptrs(e) if save else None, _p(ws), ctypes.byref(nbytes), stream), None, "mms_mlp_grad", L)
    out = []
    for a, b in zip(dw, db):
        out += [a, b]
    return out, d, e


def _rop(net, g, d, e, V, C):
    """mms_mlp_grad_rop: the R-op of J^T g along the parameters' direction (V weights, C biases), with the d_l / e_l of _grad(net, g, save=True).
    Returns (rmu = J v, [rdW_1, rdb_1, ...] = sum_rows g . (d2 mu) v)."""
    L, idx, stream = _lib.for_device(g.device)
    W = net.params[0::2]
    rmu = torch.empty_like(g)
    rdw = [torch.empty_like(w) for w in W]
    rdb = [torch.empty_like(b) for b in net.params[1::2]]
    dims, ws, nbytes = net.workspace("rop", L, idx, stream)
    _lib.check(L.mms_mlp_grad_rop(idx, net.L, g.shape[0], dims, _p(net.x), _ptrs(net.hs), _ptrs(W), _ptrs(V), _ptrs(C), _p(g), _ptrs(d),
                                  _ptrs(e), _p(rmu), _ptrs(rdw), _ptrs(rdb), _p(ws), ctypes.byref(nbytes), stream), None,
               "mms_mlp_grad_rop", L)
    out = []
    for a, b in zip(rdw, rdb):
        out += [a, b]
    return rmu, out


def _forward(x, params):
    """(mu, the saved state): hidden layers Linear + ELU and an identity output layer through mms_linear2_act, one launch per layer."""
    L, idx, stream = _lib.for_device(x.device)
    W, B = params[0::2], params[1::2]
    M, h, hs = x.shape[0], x, []
    for l, (w, b) in enumerate(zip(W, B)):
        y = torch.empty(M, w.shape[0], device=x.device)
        last = l == len(W) - 1
        _lib.check(L.mms_linear2_act(idx, M, w.shape[0], w.shape[1], _p(h), _p(w), _p(b), _p(y), None, None, None, None, 0 if last else 1,
                                     stream), None, "mms_linear2_act", L)
        if not last:
            hs.append(y)
        h = y
    return h, _Net(x, hs, list(params), [x.shape[1]] + [w.shape[0] for w in W])


class _ActorMLPGrad(torch.autograd.Function):
    """forward: J^T g (mms_mlp_grad).  backward: its R-op along the parameters' direction (mms_mlp_grad_rop)."""

    @staticmethod
    def forward(ctx, net, g, *params):
        g = g.contiguous()
        out, d, e = _grad(net, g, save=True)
        ctx.net, ctx.d, ctx.e = net, d, e
        ctx.save_for_backward(g)
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *vs):
        net, (g,) = ctx.net, ctx.saved_tensors
        rmu, out = _rop(net, g, ctx.d, ctx.e, [v.contiguous() for v in vs[0::2]], [c.contiguous() for c in vs[1::2]])
        return (None, rmu, *out)


class _ActorMLP(torch.autograd.Function):
    """mu = MLP(x): hidden layers Linear + ELU and an identity output layer through mms_linear2_act (exact fp32, bias and ELU fused),
    one launch per layer; saves every h_l (ELU's derivatives are read from h, a_l is not kept)."""

    @staticmethod
    def forward(ctx, x, *params):
        h, ctx.net = _forward(x, params)
        return h

    @staticmethod
    def backward(ctx, g):
        # torch.is_grad_enabled() here is create_graph of the caller's autograd.grad: record _ActorMLPGrad (and keep d_l / e_l) only then
        if torch.is_grad_enabled():
            grads = _ActorMLPGrad.apply(ctx.net, g, *ctx.net.params)
        else:
            grads, _, _ = _grad(ctx.net, g.contiguous(), save=False)
        return (None, *grads)


class ActorCritic(_PPOActorCritic):
    """PPO's ActorCritic; with fused_grad=True, `evaluate`'s mean goes through _ActorMLP (module docstring).

    fused_grad is off by default: at the shipped shape (8192 rows, 388 -> [1024, 1024, 512] -> 80) one HVP measured 3.89 ms on the
    kernels against 2.87 ms with torch autograd (profiles/trpo_update_bench.jsonl), so the default stays PPO's `evaluate` exactly."""

    def __init__(self, obs_shape, states_shape, actions_shape, initial_std, model_cfg, asymmetric=False, seed=0, row_offset=0, fused_grad=False):
        super().__init__(obs_shape, states_shape, actions_shape, initial_std, model_cfg, asymmetric=asymmetric, seed=seed, row_offset=row_offset)
        self.fused_grad = bool(fused_grad)

    def _grad_path_qualifies(self, obs):
        """Linear / ELU(alpha 1) pairs and a final Linear with biases, fp32 contiguous parameters, input widths multiples of 4
        (mms_linear2_act), 2..8 layers; obs fp32 contiguous on the actor's device and not requiring grad."""
        if not self.fused_grad or obs.requires_grad or obs.dtype != torch.float32 or obs.dim() != 2 or not obs.is_contiguous():
            return False
        mods = list(self.actor)
        if len(mods) < 3 or len(mods) % 2 == 0 or len(mods) > 15:
            return False
        for i, m in enumerate(mods):
            if i % 2 == 1:
                if not (isinstance(m, nn.ELU) and m.alpha == 1.0):
                    return False
            elif not (isinstance(m, nn.Linear) and m.bias is not None and m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32
                      and m.weight.is_contiguous() and m.bias.is_contiguous() and m.in_features % 4 == 0 and m.weight.device == obs.device):
                return False
        return obs.device.type in ("cuda", "cpu") and obs.shape[1] == mods[0].in_features and obs.shape[0] > 0

    def _actor_params(self):
        return [p for m in self.actor if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]

    def mean(self, observations):
        """The actor's mean as `evaluate` takes it: through _ActorMLP when the actor qualifies, the torch module otherwise."""
        if not self._grad_path_qualifies(observations):
            return self.actor(observations)
        return _ActorMLP.apply(observations, *self._actor_params())

    def mean_saved(self, observations):
        """Not in the reference: (mu, net) without an autograd graph -- _ActorMLP's forward with its saved state in hand, for a caller that
        takes the actor's derivatives itself (trpo.py: J^T g by `grad_flat`, the curvature product by `rop_flat`).  The actor must qualify."""
        if not self._grad_path_qualifies(observations):
            raise ValueError("ActorCritic.mean_saved: the actor does not qualify for the kernels' backward passes (fused_grad=True, fp32 "
                             "Linear / ELU layers with biases, input widths multiples of 4, contiguous fp32 observations on its device)")
        with torch.no_grad():
            return _forward(observations, [p.detach() for p in self._actor_params()])

    def mean_nograd(self, observations):
        """Not in the reference: the actor's mean without a graph, through the no-gradient layer route (`_hidden_one`: mms_linear2_act with
        bias and ELU in the epilogue, persistent activations) plus the last Linear where the actor is an fp32 ELU network; the torch
        module otherwise."""
        with torch.no_grad():
            if (observations.dtype == torch.float32 and observations.dim() == 2 and self._fp32_net_qualifies(self.actor)
                    and observations.device == self.actor[-1].weight.device):
                return self.actor[-1](self._hidden_one(self.actor, observations.contiguous()))
            return self.actor(observations)

    def evaluate(self, observations, states, actions):
        if not self._grad_path_qualifies(observations):
            return super().evaluate(observations, states, actions)
        mean = self.mean(observations)
        scale_log = 2.0 * self.log_std                               # as ppo/module.py's evaluate from here on
        z = (actions - mean) * torch.exp(-scale_log)
        log_prob = (-0.5 * z * z - scale_log - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + scale_log).sum(-1).expand(mean.shape[0])
        value = self.critic(states if self.asymmetric else observations)
        return log_prob, entropy, value, mean, self.log_std.repeat(mean.shape[0], 1)


def grad_flat(net, g):
    """J^T g over the actor's parameters in the flat layout of actor.parameters() (mms_mlp_grad)."""
    out, _, _ = _grad(net, g.contiguous(), save=False)
    return torch.cat([t.reshape(-1) for t in out])


def grad_saved(net, g):
    """The d_l / e_l of mms_mlp_grad(g, save): what rop_flat needs of the gradient g it differentiates."""
    _, d, e = _grad(net, g.contiguous(), save=True)
    return d, e


def rop_flat(net, g, d, e, v):
    """(J v, sum_rows g . (d2 mu / d theta2) v as a flat vector) along the flat direction v (mms_mlp_grad_rop)."""
    V, C, at = [], [], 0
    for w, b in zip(net.params[0::2], net.params[1::2]):
        V.append(v[at:at + w.numel()].view(w.shape).contiguous())
        at += w.numel()
        C.append(v[at:at + b.numel()].contiguous())
        at += b.numel()
    rmu, out = _rop(net, g, d, e, V, C)
    return rmu, torch.cat([t.reshape(-1) for t in out])

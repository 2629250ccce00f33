"""The output heads of a MAPPO / HAPPO update for a list of networks, forward and backward in HIP: `update_heads`, what the trainers run
with `fused_head_update` (trainer.py).

torch runs an actor's head as `DiagGaussian.fc_mean` (an addmm) and three element-wise kernels for
`std = sigmoid(log_std / std_x_coef) * std_y_coef`, a critic's as `v_out` (an addmm), and backward two products and a column sum per
Linear, the std expression's backward and autograd's accumulations -- per network, each a launch for a product that is 1 to 16 wide.
Here, for all networks of a call:
  forward   ONE mms_marl_heads_fwd_group call: out_g = b_g + w_g f_g for every head, std_g for every actor.
  backward  ONE mms_marl_heads_grad_group call for the networks that received a gradient: df_g, dw_g, db_g, dlog_std_g (sums in
            double in a fixed order; csrc/marl_heads_grad_kernels.hip).
More than 32 networks are chunked.  A grouped call gives network g the bits of a call on g alone, so a trainer that runs its two heads
here and MAPPO.train_group that runs all agents' heads here leave the same parameters.  Nothing synchronises with the host.  torch
"cpu" tensors go through the CPU build of the same entries (an explicit choice of device, not a fallback).  The backward is
once-differentiable.  What the entries do not take raises NotImplementedError (check_heads)."""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ... import _lib
from ..rl.ppo.loss import _workspace       # (the device's cached, 256-byte aligned workspace: one per process, calls run in stream order)

MAX_GROUPS = 32                             # include/mms.h: MMS_MAX_GROUPS
MAX_A, MAX_H = 16, 1024

_table = _lib.ptr_array                                        # HOST array of device addresses (None: NULL)


def _actor_head(actor):
    return getattr(getattr(actor, "act", None), "action_out", None)


def check_heads(actors, critics, who="update_heads"):
    """(hidden width, std_x_coef, std_y_coef) of the actors' DiagGaussian heads and the critics' v_out, or NotImplementedError for what
    update_heads does not cover.  The coefficients are None without actors."""
    actors, critics = list(actors), list(critics)
    if not actors and not critics:
        raise NotImplementedError("%s: at least one network" % who)
    widths, coefs = set(), set()

    def linear(lin, what, most):
        if not isinstance(lin, nn.Linear):
            raise NotImplementedError("%s: %s must be an nn.Linear, got %s" % (who, what, type(lin).__name__))
        if lin.bias is None:
            raise NotImplementedError("%s: %s has no bias" % (who, what))
        if lin.weight.dtype != torch.float32 or lin.bias.dtype != torch.float32:
            raise NotImplementedError("%s: fp32 parameters only (%s)" % (who, what))
        if not 1 <= lin.out_features <= most:
            raise NotImplementedError("%s: %s has %d outputs (1..%d are covered)" % (who, what, lin.out_features, most))
        widths.add(lin.in_features)

    for actor in actors:
        head = _actor_head(actor)
        if head is None or not (hasattr(head, "fc_mean") and hasattr(head, "log_std")):
            raise NotImplementedError("%s: only Box action spaces (ACTLayer.action_out = DiagGaussian) are covered" % who)
        linear(head.fc_mean, "fc_mean", MAX_A)
        if head.log_std.dtype != torch.float32 or tuple(head.log_std.shape) != (head.fc_mean.out_features,):
            raise NotImplementedError("%s: log_std must be an fp32 vector with one entry per action" % who)
        coefs.add((float(head.std_x_coef), float(head.std_y_coef)))
    for critic in critics:
        linear(getattr(critic, "v_out", None), "v_out", 1)
    if len(widths) != 1:
        raise NotImplementedError("%s: the networks of one call must have one hidden width, got %s" % (who, sorted(widths)))
    H = widths.pop()
    if H % 4 != 0 or not 4 <= H <= MAX_H:
        raise NotImplementedError("%s: hidden width %d is not covered (a multiple of 4 up to %d)" % (who, H, MAX_H))
    if len(coefs) > 1:
        raise NotImplementedError("%s: the actors must have one (std_x_coef, std_y_coef), got %s" % (who, sorted(coefs)))
    x_coef, y_coef = coefs.pop() if coefs else (None, None)
    if x_coef == 0.0:
        raise NotImplementedError("%s: std_x_coef must not be zero" % who)
    return H, x_coef, y_coef


class _Heads(torch.autograd.Function):
    """G heads of one M and H.  args: x_coef, y_coef, then per network f [M, H], weight [A, H], bias [A], log_std [A] (None: a critic).
    Returns out [M, A] per network, then std [A] per network that has a log_std.  A network none of whose inputs needs a gradient gets
    non-differentiable outputs."""

    @staticmethod
    def forward(ctx, x_coef, y_coef, *args):
        G = len(args) // 4
        nets = [args[4 * g:4 * g + 4] for g in range(G)]
        dev = nets[0][0].device
        M, H = nets[0][0].shape
        L, idx, stream = _lib.for_device(dev)
        A = [n[1].shape[0] for n in nets]
        out = [torch.empty(M, a, device=dev) for a in A]
        std = [None if n[3] is None else torch.empty(a, device=dev) for n, a in zip(nets, A)]
        for i in range(0, G, MAX_GROUPS):                             # (one launch up to 32 networks)
            sl = slice(i, min(i + MAX_GROUPS, G))
            n = sl.stop - i
            _lib.check(L.mms_marl_heads_fwd_group(idx, n, M, H, _table([t[0] for t in nets[sl]]), H, _table([t[1] for t in nets[sl]]),
                                                  _table([t[2] for t in nets[sl]]), (ctypes.c_int32 * n)(*A[sl]), _table([t[3] for t in nets[sl]]),
                                                  x_coef, y_coef, _table(out[sl]), _table(std[sl]), stream), None, "mms_marl_heads_fwd_group", L)
        ctx.save_for_backward(*args)
        ctx.coefs = (x_coef, y_coef)
        ctx.set_materialize_grads(False)                            # (an output nobody used arrives as None in backward, not as zeros)
        need = ctx.needs_input_grad[2:]
        ctx.mark_non_differentiable(*[t for g in range(G) if not any(need[4 * g:4 * g + 4]) for t in (out[g], std[g]) if t is not None])
        return tuple(out) + tuple(s for s in std if s is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        G = len(saved) // 4
        nets = [saved[4 * g:4 * g + 4] for g in range(G)]
        need = ctx.needs_input_grad[2:]
        x_coef, y_coef = ctx.coefs
        dev = nets[0][0].device
        M, H = nets[0][0].shape
        L, idx, stream = _lib.for_device(dev)
        dstd_of, k = {}, G
        for g in range(G):
            if nets[g][3] is not None:
                dstd_of[g] = grads[k]
                k += 1
        result = [None] * (4 * G)
        live = [g for g in range(G) if any(need[4 * g:4 * g + 4]) and (grads[g] is not None or dstd_of.get(g) is not None)]
        for i in range(0, len(live), MAX_GROUPS):
            gs = live[i:i + MAX_GROUPS]
            n = len(gs)
            A = [nets[g][1].shape[0] for g in gs]
            # (a .sum() upstream delivers a stride-0 expanded tensor; an output that only its std was used of: zeros)
            dout = [torch.zeros(M, a, device=dev) if grads[g] is None else grads[g].to(torch.float32).contiguous() for g, a in zip(gs, A)]
            dstd = [None if dstd_of.get(g) is None or not need[4 * g + 3] else dstd_of[g].to(torch.float32).contiguous() for g in gs]
            df = [torch.empty(M, H, device=dev) if need[4 * g] and grads[g] is not None else None for g in gs]
            sums = [(need[4 * g + 1] or need[4 * g + 2]) and grads[g] is not None for g in gs]
            dw = [torch.empty(a, H, device=dev) if s else None for s, a in zip(sums, A)]
            db = [torch.empty(a, device=dev) if s else None for s, a in zip(sums, A)]
            dls = [None if d is None else torch.empty(a, device=dev) for d, a in zip(dstd, A)]
            head = (idx, n, M, H, _table([nets[g][0] for g in gs]), H, _table([nets[g][1] for g in gs]), (ctypes.c_int32 * n)(*A), _table(dout),
                    _table([None if d is None else nets[g][3] for g, d in zip(gs, dstd)]), _table(dstd), x_coef, y_coef, _table(df), H, _table(dw), _table(db),
                    _table(dls))
            nbytes = ctypes.c_int64(-1)
            _lib.check(L.mms_marl_heads_grad_group(*head, None, ctypes.byref(nbytes), stream), None, "mms_marl_heads_grad_group size query", L)
            ws = ctypes.c_void_p(_workspace(nbytes.value, dev))
            _lib.check(L.mms_marl_heads_grad_group(*head, ws, ctypes.byref(nbytes), stream), None, "mms_marl_heads_grad_group", L)
            for j, g in enumerate(gs):
                for k, t in enumerate((df[j], dw[j], db[j], dls[j])):
                    if need[4 * g + k]:
                        result[4 * g + k] = t
        return (None, None) + tuple(result)


def update_heads(fa, fc, actors, critics, update_actor=True):
    """(mus, stds, values) of the actors' heads on the features fa[i] [M, H] and the critics' on fc[i] [M, H]: mus[i] [M, A_i], stds[i]
    [A_i], values[i] [M, 1] -- one forward call for all of them and, behind a loss, one backward call for those that got a gradient.
    Differentiable once in the features and the heads' parameters.  update_actor=False: the actors' inputs enter detached, so their
    outputs carry no gradient and they are left out of the backward call."""
    fa, fc, actors, critics = list(fa), list(fc), list(actors), list(critics)
    if len(fa) != len(actors) or len(fc) != len(critics):
        raise ValueError("update_heads: one feature tensor per network")
    H, x_coef, y_coef = check_heads(actors, critics)
    feats = fa + fc
    M = feats[0].shape[0]
    for f in feats:
        if f.dim() != 2 or tuple(f.shape) != (M, H):
            raise NotImplementedError("update_heads: every feature tensor must be [M, %d] with one M, got %s" % (H, tuple(f.shape)))
        if f.device != feats[0].device or f.dtype != torch.float32:
            raise NotImplementedError("update_heads: fp32 tensors on one device")
    keep = (lambda t: t) if update_actor else (lambda t: t.detach())
    args = []
    for f, actor in zip(fa, actors):
        head = _actor_head(actor)
        args += [keep(f.contiguous()), keep(head.fc_mean.weight), keep(head.fc_mean.bias), keep(head.log_std)]
    for f, critic in zip(fc, critics):
        args += [f.contiguous(), critic.v_out.weight, critic.v_out.bias, None]
    res = _Heads.apply(1.0 if x_coef is None else x_coef, 1.0 if y_coef is None else y_coef, *args)
    na, nc = len(actors), len(critics)
    return list(res[:na]), list(res[na + nc:]), list(res[na:na + nc])

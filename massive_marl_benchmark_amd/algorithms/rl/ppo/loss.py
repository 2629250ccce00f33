"""The loss head of PPO.update (agents/algorithms/rl/ppo/ppo.py:270-302) as one call: the KL of the adaptive schedule, the clipped
surrogate, the (clipped) value loss and the entropy term, with the gradients of the loss with respect to the networks' outputs
(`mms_ppo_loss`, include/mms.h: csrc/ppo_loss_kernels.hip on the GPU, the CPU build for CPU tensors).

    loss, info = ppo_loss(mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma,
                          clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, indices=None)

`mu` [M, A], `log_std` [A] and `value` [M] or [M, 1] are what the networks gave for the minibatch; the seven stored fields are read in
place: with `indices` (a list or an int64 tensor of M rows) they are the storage's flat views, without it they are the M gathered rows.
`loss` is differentiable with respect to mu, log_std and value (autograd carries three tensors into the two MLPs); `info` holds the
device scalars `surrogate`, `value_loss`, `entropy` and `kl`, none of them differentiable (ppo.py takes them with .item() or under
no_grad).  Inputs the entry does not take -- a dtype other than float32, more than MMS_PPO_LOSS_MAX_A actions, storage that is not
contiguous -- are evaluated by `ppo_loss_torch`, the same expression in torch ops; that is decided before anything is launched."""
import ctypes
import math

import torch

from .... import _lib

MAX_A = 128              # include/mms.h: MMS_PPO_LOSS_MAX_A

_workspaces = {}         # device -> uint8 tensor (grown on demand; every call on a device runs in stream order on the caller's stream)


def ppo_loss_torch(mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma, clip_param, value_loss_coef,
                   entropy_coef, use_clipped_value_loss, indices=None):
    """The expression of ppo.py:270-302 behind ActorCritic.evaluate in torch ops; returns (loss, info) like ppo_loss."""
    A = mu.shape[-1]
    take = (lambda t, *s: t.reshape(-1, *s)) if indices is None else (lambda t, *s: t.reshape(-1, *s)[indices])
    actions, old_mu, old_sigma = take(actions, A), take(old_mu, A), take(old_sigma, A)
    old_logp, adv, returns, target_values = take(old_logp), take(adv), take(returns), take(target_values)
    value = value.reshape(-1)
    scale_log = 2.0 * log_std
    z = (actions - mu) * torch.exp(-scale_log)
    logp = (-0.5 * z * z - scale_log - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + scale_log).sum(-1)
    with torch.no_grad():
        kl = torch.sum(log_std - old_sigma + (torch.square(old_sigma.exp()) + torch.square(old_mu - mu)) / (2.0 * torch.square(log_std.exp())) - 0.5,
                       dim=-1).mean()
    ratio = torch.exp(logp - old_logp)
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param)).mean()
    if use_clipped_value_loss:
        value_clipped = target_values + (value - target_values).clamp(-clip_param, clip_param)
        value_loss = torch.max((value - returns).pow(2), (value_clipped - returns).pow(2)).mean()
    else:
        value_loss = (returns - value).pow(2).mean()
    loss = surrogate + value_loss_coef * value_loss - entropy_coef * entropy
    return loss, {"surrogate": surrogate.detach(), "value_loss": value_loss.detach(), "entropy": entropy.detach(), "kl": kl}


def _workspace(nbytes, device):
    """A 256-byte aligned address with `nbytes` behind it, inside the device's cached buffer."""
    need = int(nbytes) + 256
    buf = _workspaces.get(device)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.uint8, device=device)
        _workspaces[device] = buf
    return buf.data_ptr() + (-buf.data_ptr()) % 256


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _PpoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, log_std, value, indices, actions, old_logp, adv, returns, target_values, old_mu, old_sigma, clip, value_coef, entropy_coef,
                clipped_value):
        M, A = mu.shape
        dev = mu.device
        L, idx, stream = _lib.for_device(dev)
        grads = any(ctx.needs_input_grad[:3])
        out = torch.empty(5, device=dev)
        dmu, dls, dv = (torch.empty_like(mu), torch.empty_like(log_std), torch.empty(M, device=dev)) if grads else (None, None, None)
        nbytes = ctypes.c_int64(-1)
        head = (idx, M, A, _p(mu), _p(log_std), _p(value), _p(indices), _p(actions), _p(old_logp), _p(adv), _p(returns), _p(target_values), _p(old_mu),
                _p(old_sigma), clip, value_coef, entropy_coef, clipped_value, _p(out), _p(dmu), _p(dls), _p(dv))
        _lib.check(L.mms_ppo_loss(*head, None, ctypes.byref(nbytes), stream), None, "mms_ppo_loss size query", L)
        ws = _workspace(nbytes.value, dev)
        _lib.check(L.mms_ppo_loss(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_ppo_loss", L)
        ctx.saved = (dmu, dls, dv, value.shape)
        terms = out.unbind(0)
        ctx.mark_non_differentiable(*terms[1:])
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *unused):
        dmu, dls, dv, vshape = ctx.saved
        need = ctx.needs_input_grad
        return (g * dmu if need[0] else None, g * dls if need[1] else None, (g * dv).view(vshape) if need[2] else None) + (None,) * 12


def ppo_loss(mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma, clip_param, value_loss_coef, entropy_coef,
             use_clipped_value_loss, indices=None):
    """(loss, info): see the module docstring."""
    args = (mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma)
    dev = mu.device
    if indices is not None and not torch.is_tensor(indices):
        indices = torch.as_tensor(indices, dtype=torch.int64, device=dev)           # a list of indices: one copy to the device
    fused = (mu.dim() == 2 and 1 <= mu.shape[1] <= MAX_A and mu.shape[0] >= 1 and all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in args)
             and (indices is None or (indices.dtype == torch.int64 and indices.is_contiguous() and indices.device == dev)))
    if not fused:
        return ppo_loss_torch(*args, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, indices)
    M, A = mu.shape
    rows = M if indices is None else indices.numel()
    if rows != M or value.numel() != M or log_std.numel() != A:
        raise ValueError("ppo_loss: mu is [%d, %d] but value has %d elements, log_std %d and the minibatch %d rows" % (M, A, value.numel(), log_std.numel(), rows))
    if indices is None and any(t.numel() != n for t, n in zip(args[3:], (M * A, M, M, M, M, M * A, M * A))):
        raise ValueError("ppo_loss: without indices the stored fields are the minibatch's own rows")
    loss, surrogate, value_loss, entropy, kl = _PpoLoss.apply(mu, log_std, value, indices, actions, old_logp, adv, returns, target_values, old_mu, old_sigma,
                                                             float(clip_param), float(value_loss_coef), float(entropy_coef), int(bool(use_clipped_value_loss)))
    return loss, {"surrogate": surrogate, "value_loss": value_loss, "entropy": entropy, "kl": kl}

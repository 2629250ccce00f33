"""The loss head of the MAPPO / HAPPO update (agents/algorithms/marl/mappo_trainer.py:63-179, happo_trainer.py:48-170, behind
ACTLayer.evaluate_actions for a Box space) as one call: the per-dimension Gaussian log-density, the clipped surrogate with HAPPO's
factor, the entropy term, the (PopArt-normalised, clipped, Huber) value loss and the active masks, with the gradients of the objective
with respect to the networks' outputs (`mms_marl_ppo_loss`, include/mms.h: csrc/marl_loss_kernels.hip on the GPU, the CPU build for
CPU tensors).

    objective, info = marl_ppo_loss(mu, std, value, actions, old_logp, adv, value_preds, returns, active_masks=None, factor=None,
                                    clip_param=.., value_loss_coef=.., entropy_coef=.., huber_delta=.., use_huber_loss=..,
                                    use_clipped_value_loss=.., use_policy_active_masks=False, use_value_active_masks=False,
                                    norm_mean=None, norm_var=None, indices=None, row_logp=False)
    objectives, info = marl_ppo_loss_group(mus, stds, values, fields, ...)       G independent agents (MAPPO) in one call: see there

`mu` [M, A], `std` [A] and `value` [M] or [M, 1] are what the networks gave for the minibatch.  The stored fields are taken as the
buffers hold them -- [T, N, A] / [T+1, N, 1] tensors of a SeparatedReplayBuffer, or one agent's strided views of SharedRolloutBuffers
(`actions[:, :, k]`, `value_preds[:, :, k:k+1]`) -- and read in place: the row pitch of each is derived here.  With `indices` (a list
or an int64 tensor of M flat rows t N + n) they are the buffer's tensors, without it the minibatch is their first M rows.
`objective` = policy_loss - entropy_coef dist_entropy + value_loss_coef value_loss is differentiable with respect to mu, std and value
(pass `mu.detach()` / `std.detach()` for update_actor=False); the reference backpropagates its two halves into the actor and the
critic separately, which is the same thing for disjoint parameter sets.  `info` holds the device scalars `policy_loss`, `value_loss`,
`dist_entropy` and `ratio` (mean_i r_i), and `row_logp` [M] = sum_j logp_ij when asked for; none of them differentiable.
Inputs the entry does not take -- a dtype other than float32, more than MMS_MARL_LOSS_MAX_A actions, fields whose rows are not dense
(a last dimension that is not contiguous, leading dimensions that do not collapse to one pitch) -- are evaluated by
`marl_ppo_loss_torch`, the same expression in torch ops; that is decided before anything is launched.

One stream per device: the per-block partials live in one cached workspace per device, so calls on the same device must be ordered
on one stream (the caller's current one, as the trainers run them).  Calls issued on two streams of a device at once would race on
it (rl/ppo/loss.py has the same limit)."""
import ctypes
import math

import torch

from ... import _lib
from ...model import MmsMarlLossFields, MmsMarlLossGroup, MmsRows

MAX_A = 128              # include/mms.h: MMS_MARL_LOSS_MAX_A
MAX_GROUPS = 32          # include/mms.h: MMS_MAX_GROUPS
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)

_workspaces = {}         # device -> uint8 tensor (grown on demand; every call on a device runs in stream order on the caller's stream)


def marl_ppo_loss_torch(mu, std, value, actions, old_logp, adv, value_preds, returns, active_masks=None, factor=None, *, clip_param,
                        value_loss_coef, entropy_coef, huber_delta, use_huber_loss, use_clipped_value_loss, use_policy_active_masks=False,
                        use_value_active_masks=False, norm_mean=None, norm_var=None, indices=None, row_logp=False):
    """The reference's expression in torch ops (the trainers' ppo_update and cal_value_loss, FixedNormal.log_probs, ACTLayer's entropy,
    huber_loss / mse_loss); returns (objective, info) like marl_ppo_loss."""
    M, A = mu.shape
    if indices is not None and not torch.is_tensor(indices):
        indices = torch.as_tensor(indices, dtype=torch.int64, device=mu.device)
    take = (lambda t, w: t.reshape(-1, w)[:M]) if indices is None else (lambda t, w: t.reshape(-1, w)[indices])
    a, olp = take(actions, A), take(old_logp, A)
    adv, vp, ret = take(adv, 1), take(value_preds, 1), take(returns, 1)
    masks = take(active_masks, 1) if (use_policy_active_masks or use_value_active_masks) else None
    values = value.reshape(-1, 1)
    logp = -((a - mu) ** 2) / (2 * std ** 2) - std.log() - HALF_LOG_2PI                       # torch.distributions.Normal.log_prob
    entropy = (0.5 + HALF_LOG_2PI + std.log()).expand(M, A)                                   # Normal.entropy
    imp_weights = torch.exp((logp - olp).sum(dim=-1, keepdim=True))
    surr = torch.min(imp_weights * adv, torch.clamp(imp_weights, 1.0 - clip_param, 1.0 + clip_param) * adv)
    if factor is not None:
        surr = take(factor, 1) * surr
    if use_policy_active_masks:
        policy_loss = (-torch.sum(surr, dim=-1, keepdim=True) * masks).sum() / masks.sum()
        dist_entropy = (entropy * masks).sum() / masks.sum()
    else:
        policy_loss = -torch.sum(surr, dim=-1, keepdim=True).mean()
        dist_entropy = entropy.mean()
    target = ret if norm_mean is None else (ret - norm_mean) / torch.sqrt(norm_var)
    clipped = vp + (values - vp).clamp(-clip_param, clip_param)
    e_c, e_o = target - clipped, target - values
    if use_huber_loss:
        h = lambda e: (abs(e) <= huber_delta).to(e.dtype) * e ** 2 / 2 + (e > huber_delta).to(e.dtype) * huber_delta * (abs(e) - huber_delta / 2)
    else:
        h = lambda e: e ** 2 / 2
    value_loss = torch.max(h(e_o), h(e_c)) if use_clipped_value_loss else h(e_o)
    value_loss = (value_loss * masks).sum() / masks.sum() if use_value_active_masks else value_loss.mean()
    objective = policy_loss - entropy_coef * dist_entropy + value_loss_coef * value_loss
    info = {"policy_loss": policy_loss.detach(), "value_loss": value_loss.detach(), "dist_entropy": dist_entropy.detach(),
            "ratio": imp_weights.detach().mean()}
    if row_logp:
        info["row_logp"] = logp.detach().sum(-1)
    return objective, info


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


def field_rows(t, width):
    """(pitch in floats, rows) of a stored field whose rows hold `width` floats, or None when its rows are not dense: the last
    dimension is the row (contiguous; a trailing [.., 1] of a one-float field is dropped) and the dimensions before it must collapse
    to one pitch, as the buffers' tensors and their per-agent views do."""
    shape, stride = list(t.shape), list(t.stride())
    if width > 1 or (len(shape) > 1 and shape[-1] == 1):
        if not shape or shape[-1] != width or (width > 1 and stride[-1] != 1):
            return None
        shape, stride = shape[:-1], stride[:-1]
    lead = [(n, s) for n, s in zip(shape, stride) if n != 1]
    if not lead:
        return width, 1
    for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != s1 * n1:
            return None
    pitch = lead[-1][1]
    if pitch < width:
        return None
    rows = 1
    for n, _ in lead:
        rows *= n
    return pitch, rows


class _MarlPpoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, std, value, indices, fields, pitches, scalars, flags, norm_mean, norm_var, want_row_logp):
        M, A = mu.shape
        dev = mu.device
        L, idx, stream = _lib.for_device(dev)
        grads = any(ctx.needs_input_grad[:3])
        out = torch.empty(5, device=dev)
        dmu, dstd, dv = (torch.empty_like(mu), torch.empty_like(std), torch.empty(M, device=dev)) if grads else (None, None, None)
        logp = torch.empty(M, device=dev) if want_row_logp else None
        f = MmsMarlLossFields()
        for name, t, pitch in zip(MmsMarlLossFields.NAMES, fields, pitches):
            if t is not None:
                setattr(f, name, MmsRows(t.data_ptr(), pitch))
        nbytes = ctypes.c_int64(-1)
        head = (idx, M, A, _p(mu), _p(std), _p(value), _p(indices), ctypes.addressof(f), *scalars, *flags, _p(norm_mean), _p(norm_var), _p(out), _p(dmu),
                _p(dstd), _p(dv), _p(logp))
        _lib.check(L.mms_marl_ppo_loss(*head, None, ctypes.byref(nbytes), stream), None, "mms_marl_ppo_loss size query", L)
        ws = _workspace(nbytes.value, dev)
        _lib.check(L.mms_marl_ppo_loss(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_marl_ppo_loss", L)
        ctx.saved = (dmu, dstd, dv, value.shape)
        terms = out.unbind(0) + ((logp,) if want_row_logp else ())
        ctx.mark_non_differentiable(*terms[1:])
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *unused):
        dmu, dstd, dv, vshape = ctx.saved
        need = ctx.needs_input_grad
        return (g * dmu if need[0] else None, g * dstd if need[1] else None, (g * dv).view(vshape) if need[2] else None) + (None,) * 8


def marl_ppo_loss(mu, std, value, actions, old_logp, adv, value_preds, returns, active_masks=None, factor=None, *, clip_param, value_loss_coef,
                  entropy_coef, huber_delta, use_huber_loss, use_clipped_value_loss, use_policy_active_masks=False, use_value_active_masks=False,
                  norm_mean=None, norm_var=None, indices=None, row_logp=False):
    """(objective, info): see the module docstring."""
    kw = dict(clip_param=clip_param, value_loss_coef=value_loss_coef, entropy_coef=entropy_coef, huber_delta=huber_delta, use_huber_loss=use_huber_loss,
              use_clipped_value_loss=use_clipped_value_loss, use_policy_active_masks=use_policy_active_masks, use_value_active_masks=use_value_active_masks,
              norm_mean=norm_mean, norm_var=norm_var, indices=indices, row_logp=row_logp)
    dev = mu.device
    masked = bool(use_policy_active_masks or use_value_active_masks)
    if masked and active_masks is None:
        raise ValueError("marl_ppo_loss: a mask flag is on but active_masks is None")
    if (norm_mean is None) != (norm_var is None):
        raise ValueError("marl_ppo_loss: norm_mean and norm_var go together")
    if indices is not None and not torch.is_tensor(indices):
        indices = kw["indices"] = torch.as_tensor(indices, dtype=torch.int64, device=dev)     # a list of indices: one copy to the device
    fields = (actions, old_logp, adv, value_preds, returns, active_masks if masked else None, factor)
    tensors = [t for t in (mu, std, value, norm_mean, norm_var) + fields if t is not None]
    fused = (mu.dim() == 2 and 1 <= mu.shape[1] <= MAX_A and mu.shape[0] >= 1 and all(t.dtype == torch.float32 and t.device == dev for t in tensors)
             and mu.is_contiguous() and std.is_contiguous() and value.is_contiguous()
             and (indices is None or (indices.dtype == torch.int64 and indices.is_contiguous() and indices.device == dev)))
    rows = None
    if fused:
        A = mu.shape[1]
        rows = [None if t is None else field_rows(t, A if i < 2 else 1) for i, t in enumerate(fields)]
        fused = all(r is not None for r, t in zip(rows, fields) if t is not None)
    if not fused:
        return marl_ppo_loss_torch(mu, std, value, actions, old_logp, adv, value_preds, returns, active_masks, factor, **kw)
    M, A = mu.shape
    n = M if indices is None else indices.numel()
    if n != M or value.numel() != M or std.numel() != A:
        raise ValueError("marl_ppo_loss: mu is [%d, %d] but value has %d elements, std %d and the minibatch %d rows" % (M, A, value.numel(), std.numel(), n))
    if indices is None and any(r[1] < M for r in rows if r is not None):
        raise ValueError("marl_ppo_loss: without indices the stored fields hold the minibatch's own rows first (a field has fewer than %d)" % M)
    scalars = (float(clip_param), float(value_loss_coef), float(entropy_coef), float(huber_delta))
    flags = (int(bool(use_huber_loss)), int(bool(use_clipped_value_loss)), int(bool(use_policy_active_masks)), int(bool(use_value_active_masks)),
             int(norm_mean is not None))
    out = _MarlPpoLoss.apply(mu, std, value, indices, fields, tuple(0 if r is None else r[0] for r in rows), scalars, flags, norm_mean, norm_var, bool(row_logp))
    info = {"policy_loss": out[1], "value_loss": out[2], "dist_entropy": out[3], "ratio": out[4]}
    if row_logp:
        info["row_logp"] = out[5]
    return out[0], info


# ---- every agent of a MAPPO run in one call (mms_marl_ppo_loss_group) ---------------------------------------------------------------

class _MarlPpoLossGroup(torch.autograd.Function):
    """forward(ctx, setup, mu_0, std_0, value_0, mu_1, ..): one entry call per MAX_GROUPS groups; returns the G objectives (0-d, the only
    differentiable outputs), the [G, 5] rows of the entry's `out` and, when asked for, the G row_logp vectors."""

    @staticmethod
    def forward(ctx, setup, *nets):
        indices, fields, pitches, scalars, flags, norms, want_row_logp = setup
        G = len(nets) // 3
        mus, stds, values = nets[0::3], nets[1::3], nets[2::3]
        M, A = mus[0].shape
        dev = mus[0].device
        L, idx, stream = _lib.for_device(dev)
        out = torch.empty(G, 5, device=dev)
        need = ctx.needs_input_grad
        grads = [any(need[1 + 3 * g:4 + 3 * g]) for g in range(G)]
        dmu = [torch.empty_like(mus[g]) if grads[g] else None for g in range(G)]
        dstd = [torch.empty_like(stds[g]) if grads[g] else None for g in range(G)]
        dv = [torch.empty(M, device=dev) if grads[g] else None for g in range(G)]
        logp = [torch.empty(M, device=dev) if want_row_logp else None for g in range(G)]
        ptr = lambda t: None if t is None else t.data_ptr()
        for lo in range(0, G, MAX_GROUPS):
            n = min(MAX_GROUPS, G - lo)
            table = (MmsMarlLossGroup * n)()
            for k in range(n):
                g, t = lo + k, table[k]
                t.mu, t.std, t.value, t.indices = ptr(mus[g]), ptr(stds[g]), ptr(values[g]), ptr(indices[g])
                for name, f, pitch in zip(MmsMarlLossFields.NAMES, fields[g], pitches[g]):
                    if f is not None:
                        setattr(t.fields, name, MmsRows(f.data_ptr(), pitch))
                t.norm_mean, t.norm_var = (ptr(norms[g][0]), ptr(norms[g][1])) if norms is not None else (None, None)
                t.out, t.dmu, t.dstd, t.dvalue, t.row_logp = out[g].data_ptr(), ptr(dmu[g]), ptr(dstd[g]), ptr(dv[g]), ptr(logp[g])
            nbytes = ctypes.c_int64(-1)
            head = (idx, n, M, A, ctypes.addressof(table), *scalars, *flags)
            _lib.check(L.mms_marl_ppo_loss_group(*head, None, ctypes.byref(nbytes), stream), None, "mms_marl_ppo_loss_group size query", L)
            ws = _workspace(nbytes.value, dev)
            _lib.check(L.mms_marl_ppo_loss_group(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_marl_ppo_loss_group", L)
        ctx.saved = (dmu, dstd, dv, [v.shape for v in values])
        objectives = out[:, 0].unbind(0)
        rest = (out,) + (tuple(logp) if want_row_logp else ())
        ctx.mark_non_differentiable(*rest)
        return objectives + rest

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        dmu, dstd, dv, vshapes = ctx.saved
        need = ctx.needs_input_grad
        res = [None]
        for g in range(len(dmu)):
            k = 1 + 3 * g
            res += [gs[g] * dmu[g] if need[k] else None, gs[g] * dstd[g] if need[k + 1] else None,
                    (gs[g] * dv[g]).view(vshapes[g]) if need[k + 2] else None]
        return tuple(res)


def marl_ppo_loss_group(mus, stds, values, fields, *, clip_param, value_loss_coef, entropy_coef, huber_delta, use_huber_loss, use_clipped_value_loss,
                        use_policy_active_masks=False, use_value_active_masks=False, norms=None, indices=None, row_logp=False):
    """marl_ppo_loss for G agents whose updates do not depend on each other (MAPPO's), one mms_marl_ppo_loss_group call per 32 of them.
    mus, stds, values: G tensors each, of one shape per kind; fields: G tuples (actions, old_logp, adv, value_preds, returns,
    active_masks, factor) as marl_ppo_loss takes them; norms: None, or G pairs (norm_mean, norm_var); indices: None, or G entries
    (None or an int64 device tensor of M rows).  The scalars and flags are shared.
    Returns (objectives, info): G 0-d tensors, objective g differentiable with respect to (mus[g], stds[g], values[g]) and equal, bit
    for bit, to marl_ppo_loss on agent g's arguments; info = {"policy_loss", "value_loss", "dist_entropy", "ratio"}: [G] device
    tensors, and "row_logp": G [M] tensors when asked for.  Nothing is read back to the host.
    Inputs the entry does not take (marl_ppo_loss's list) raise NotImplementedError: evaluate such agents one by one."""
    mus, stds, values, fields = list(mus), list(stds), list(values), [tuple(f) for f in fields]
    G = len(mus)
    if G < 1 or not (len(stds) == len(values) == len(fields) == G):
        raise ValueError("marl_ppo_loss_group: one std, value and tuple of fields per mu, at least one")
    indices = [None] * G if indices is None else list(indices)
    if len(indices) != G or (norms is not None and len(norms) != G):
        raise ValueError("marl_ppo_loss_group: indices and norms hold one entry per agent")
    masked = bool(use_policy_active_masks or use_value_active_masks)
    dev = mus[0].device
    if mus[0].dim() != 2:
        raise NotImplementedError("marl_ppo_loss_group: mu must be [M, A]")
    M, A = mus[0].shape
    if not (1 <= A <= MAX_A and M >= 1):
        raise NotImplementedError("marl_ppo_loss_group: 1 <= A <= %d and M >= 1" % MAX_A)
    pitches = []
    for g in range(G):
        f = fields[g]
        if len(f) != 7 or any(t is None for t in f[:5]) or (masked and f[5] is None):
            raise ValueError("marl_ppo_loss_group: fields are (actions, old_logp, adv, value_preds, returns, active_masks, factor); active_masks with a mask flag")
        f = fields[g] = tuple(t if (i != 5 or masked) else None for i, t in enumerate(f))      # (without a mask flag active_masks is not read)
        if tuple(mus[g].shape) != (M, A) or stds[g].numel() != A or values[g].numel() != M:
            raise ValueError("marl_ppo_loss_group: agent %d: mu [%d, %d], std [%d] and value [%d] expected" % (g, M, A, A, M))
        if indices[g] is not None and not torch.is_tensor(indices[g]):
            indices[g] = torch.as_tensor(indices[g], dtype=torch.int64, device=dev)
        norm = () if norms is None else tuple(norms[g])
        tensors = [t for t in (mus[g], stds[g], values[g]) + norm + f if t is not None]
        ok = (all(t.dtype == torch.float32 and t.device == dev for t in tensors) and mus[g].is_contiguous() and stds[g].is_contiguous()
              and values[g].is_contiguous() and len(norm) in (0, 2) and all(t is not None for t in norm)
              and (indices[g] is None or (indices[g].dtype == torch.int64 and indices[g].is_contiguous() and indices[g].device == dev
                                          and indices[g].numel() == M)))
        rows = [None if t is None else field_rows(t, A if i < 2 else 1) for i, t in enumerate(f)] if ok else None
        if not ok or any(r is None for r, t in zip(rows, f) if t is not None):
            raise NotImplementedError("marl_ppo_loss_group: agent %d: float32 tensors on one device, dense mu / std / value, stored fields with dense rows "
                                      "and int64 indices of M rows (marl_ppo_loss serves the rest, agent by agent)" % g)
        if indices[g] is None and any(r[1] < M for r in rows if r is not None):
            raise ValueError("marl_ppo_loss_group: agent %d: without indices the stored fields hold the minibatch's own rows first" % g)
        pitches.append(tuple(0 if r is None else r[0] for r in rows))
    scalars = (float(clip_param), float(value_loss_coef), float(entropy_coef), float(huber_delta))
    flags = (int(bool(use_huber_loss)), int(bool(use_clipped_value_loss)), int(bool(use_policy_active_masks)), int(bool(use_value_active_masks)),
             int(norms is not None))
    setup = (indices, fields, pitches, scalars, flags, None if norms is None else [tuple(n) for n in norms], bool(row_logp))
    nets = [t for g in range(G) for t in (mus[g], stds[g], values[g])]
    res = _MarlPpoLossGroup.apply(setup, *nets)
    out = res[G]
    info = {"policy_loss": out[:, 1], "value_loss": out[:, 2], "dist_entropy": out[:, 3], "ratio": out[:, 4]}
    if row_logp:
        info["row_logp"] = list(res[G + 1:])
    return res[:G], info

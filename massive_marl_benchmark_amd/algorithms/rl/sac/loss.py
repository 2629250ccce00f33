"""The critics' loss heads of the off-policy update WITH a gradient, as one call of the C ABI (`mms_q_heads_loss`, include/mms.h).

`q_heads_loss(hs, lasts, target=None, logp=None, alpha=0.0, mode="mse")` takes the last hidden activations of one or two critics
(`hs`: [M, H] each, wanting a gradient or not) and their last layers (`lasts`: nn.Linear(H, 1) each) and returns the 0-d loss

  mode "mse" (0)   sum_g mean((q_g - target)^2)                    compute_loss_q, sac.py:385-387 (one network: TD3's / DDPG's critic loss)
  mode "pi"  (1)   mean(alpha logp - min_g q_g)                    the critic half of compute_loss_pi, sac.py:396-401 (logp None: -mean(min q))

with q_g = lasts[g](hs[g]).  Forward, loss and backward are ONE streaming pass: the forward call runs the entry with scale = 1 and
keeps d loss / d (h_g, w_g, b_g); the backward multiplies them by the incoming 0-d gradient.  `needs_input_grad` decides which of
them the entry computes (frozen critics: no dw / db).  d loss / d logp = alpha / M is formed in the backward.  `target` takes no
gradient (the reference builds it under no_grad).  Once differentiable, like the actor's `_SacHead`.  It runs on "cuda" and, through
the CPU build, on "cpu".

`q_heads_loss_torch` is the same expression in torch ops; `q_heads_loss` uses it for anything the entry does not take -- dtype, H (a
multiple of 64 up to 1024), alignment, a target that wants a gradient, no library for the device -- and that choice is made before
anything is launched."""
import ctypes
import os

import torch
import torch.nn.functional as F

from .... import _lib
from ..ppo.loss import _p, _workspace

MAX_H = 1024             # include/mms.h: MMS_Q_LOSS_MAX_H
MODES = {"mse": 0, "pi": 1, 0: 0, 1: 1}


def q_heads_loss_torch(hs, lasts, target=None, logp=None, alpha=0.0, mode="mse"):
    """The two loss heads in torch ops (sac.py:370-371 + 385-387, and :396-401)."""
    mode = MODES[mode]
    qs = [F.linear(h, last.weight, last.bias).reshape(-1) for h, last in zip(hs, lasts)]
    if mode == 0:
        t = target.reshape(-1)
        loss = ((qs[0] - t) ** 2).mean()
        for q in qs[1:]:
            loss = loss + ((q - t) ** 2).mean()
        return loss
    m = qs[0] if len(qs) == 1 else torch.min(qs[0], qs[1])
    return (-m).mean() if logp is None else (alpha * logp.reshape(-1) - m).mean()


class _QHeadsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mode, alpha, target, logp, *nets):           # nets: h0, w0, b0[, h1, w1, b1]
        G = len(nets) // 3
        h, w, b = nets[0::3], nets[1::3], nets[2::3]
        M, H = h[0].shape
        dev = h[0].device
        L, idx, stream = _lib.for_device(dev)
        need = ctx.needs_input_grad
        loss = torch.empty((), device=dev)
        dh = [torch.empty(M, H, device=dev) if need[4 + 3 * g] else None for g in range(G)]
        pair = [need[5 + 3 * g] or need[6 + 3 * g] for g in range(G)]
        dw = [torch.empty(1, H, device=dev) if pair[g] else None for g in range(G)]
        db = [torch.empty(1, device=dev) if pair[g] else None for g in range(G)]
        second = lambda xs: _p(xs[1]) if G == 2 else None
        nbytes = ctypes.c_int64(-1)
        head = (idx, M, H, _p(h[0]), _p(w[0]), _p(b[0]), second(h), second(w), second(b), mode, _p(target), _p(logp), float(alpha), 1.0, _p(loss),
                None, None, _p(dh[0]), second(dh), _p(dw[0]), _p(db[0]), second(dw), second(db))
        _lib.check(L.mms_q_heads_loss(*head, None, ctypes.byref(nbytes), stream), None, "mms_q_heads_loss size query", L)
        ws = _workspace(nbytes.value, dev)
        _lib.check(L.mms_q_heads_loss(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_q_heads_loss", L)
        ctx.kept = (dh, dw, db)
        ctx.logp_grad = (float(alpha) / M, logp.shape) if (logp is not None and need[3]) else None
        ctx.G = G
        return loss

    @staticmethod
    def backward(ctx, g):
        # (see _SacHead.backward: under create_graph=True the stored gradients would come back silently constant)
        if torch.is_grad_enabled():
            raise RuntimeError("q_heads_loss: the fused loss head is once differentiable (no create_graph=True)")
        return _QHeadsLoss._backward(ctx, g)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _backward(ctx, g):
        dh, dw, db = ctx.kept
        need = ctx.needs_input_grad
        g = g.to(torch.float32)
        out = [None, None, None, None]
        if ctx.logp_grad is not None:
            out[3] = (g * ctx.logp_grad[0]).expand(ctx.logp_grad[1])
        for k in range(ctx.G):
            out.append(dh[k] * g if need[4 + 3 * k] else None)
            out.append(dw[k] * g if need[5 + 3 * k] else None)
            out.append(db[k] * g if need[6 + 3 * k] else None)
        return tuple(out)


def _takes(hs, lasts, target, logp, mode):
    """Whether the entry takes this call; nothing has been launched yet."""
    if len(hs) not in (1, 2) or len(lasts) != len(hs) or hs[0].dim() != 2:
        return False
    M, H = hs[0].shape
    dev = hs[0].device
    if dev.type not in ("cuda", "cpu") or M < 1 or M > 0x7fffffff or H % 64 or H > MAX_H:
        return False
    if not os.path.exists(_lib.LIB_CPU_PATH if dev.type == "cpu" else _lib.LIB_PATH):
        return False
    ok = lambda t: t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.data_ptr() % 16 == 0
    for h, last in zip(hs, lasts):
        if h.shape != (M, H) or not ok(h) or last.weight.shape != (1, H) or last.bias is None or not ok(last.weight) or not ok(last.bias):
            return False
    if mode == 0 and (target is None or target.requires_grad):
        return False
    return all(t is None or (t.numel() == M and ok(t)) for t in (target, logp))


def q_heads_loss(hs, lasts, target=None, logp=None, alpha=0.0, mode="mse"):
    """The 0-d loss of the module docstring; fused where the entry takes the call, q_heads_loss_torch otherwise."""
    mode = MODES[mode]
    if mode == 0 and target is None:
        raise ValueError("q_heads_loss: mode 'mse' needs a target")
    if mode == 1:
        target = None
    else:
        logp = None
    hs = [h.contiguous() for h in hs]
    if not _takes(hs, lasts, target, logp, mode):
        return q_heads_loss_torch(hs, lasts, target, logp, alpha, mode)
    nets = []
    for h, last in zip(hs, lasts):
        nets += [h, last.weight, last.bias]
    return _QHeadsLoss.apply(mode, float(alpha), None if target is None else target.detach(), logp, *nets)

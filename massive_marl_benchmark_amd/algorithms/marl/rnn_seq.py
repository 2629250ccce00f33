"""The GRU of RNNLayer's sequence branch (agents/algorithms/utils/rnn.py:30-77) for a list of networks, with the gate arithmetic and its
backward in HIP: `gru_sequence`, what the MAPPO / HAPPO trainers run with `fused_rnn_update` (trainer.py).

The reference cuts the sequence wherever some env's mask is zero (a host read of `masks` in the middle of the forward), multiplies the
state by that step's masks at the start of every piece and runs one nn.GRU call per piece.  A per-row 0 / 1 mask commutes with the
product, (m h) W^T = m (h W^T), and inside a piece every mask is 1, so multiplying at EVERY step is the same function: no cuts, no host
read, a launch sequence that does not depend on the data.  MASKS MUST BE 0 / 1 (the buffers' are): with any other value the reference
applies it at the cuts only, this at every step.

Per GRU layer, for G networks of one shape (time-major rows [T * N, .], N = h0.size(0), as RNNLayer reads them):
  forward   gi = X W_ih^T + b_ih over all T * N rows: one addmm per network (it does not depend on the state); then per step one
            library product gh_t = h_{t-1} W_hh^T per network into a saved [T, N, 3H] block and ONE mms_gru_gates_group call for all
            networks, which applies the mask and writes h_t into a saved [T + 1, N, H] block.
  backward  per step in reverse ONE mms_gru_gates_grad_group call for all networks (dgi_t, dgh_t, the direct dh, the step's [4H] bias
            sums; csrc/gru_grad_kernels.hip) and one addmm per network, dh_{t-1} = dh + dgh_t W_hh; after the loop one product each for
            dW_ih = dgi^T X, dW_hh = dgh^T h_{0..T-1} and dX = dgi W_ih over all T * N rows, and the [T, 4H] bias sums added over T.
            Layers in reverse, the upper layer's dX being the lower layer's second gradient dy.
Every matrix product is the library's; nothing here synchronises with the host.  torch "cpu" tensors go through the CPU build of the
same entries (an explicit choice of device, not a fallback).  The backward is once-differentiable.  Shapes the entries refuse (H not a
multiple of 4, H > 1024), networks of unequal shape and modules that are not a plain nn.GRU raise NotImplementedError."""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ... import _lib
from ..rl.ppo.loss import _workspace       # (the device's cached, 256-byte aligned workspace: one per process, calls run in stream order)

MAX_GROUPS = 32                             # include/mms.h: MMS_MAX_GROUPS


def check_grus(grus, who="gru_sequence"):
    """(input size, H, recurrent_N) of the networks' GRUs, or NotImplementedError for what gru_sequence does not cover"""
    grus = list(grus)
    if not grus or len(grus) > MAX_GROUPS:
        raise NotImplementedError("%s: 1..%d networks per call, got %d" % (who, MAX_GROUPS, len(grus)))
    for gru in grus:
        if not isinstance(gru, nn.GRU):
            raise NotImplementedError("%s: every network's recurrent module must be an nn.GRU, got %s" % (who, type(gru).__name__))
        if gru.bidirectional or gru.batch_first or not gru.bias or gru.dropout != 0 or getattr(gru, "proj_size", 0):
            raise NotImplementedError("%s: only the plain nn.GRU of RNNLayer (time-major, one direction, with biases, no dropout)" % who)
        if any(p.dtype != torch.float32 for p in gru.parameters()):
            raise NotImplementedError("%s: fp32 parameters only" % who)
    K, H, R = grus[0].input_size, grus[0].hidden_size, grus[0].num_layers
    if any((g.input_size, g.hidden_size, g.num_layers) != (K, H, R) for g in grus):
        raise NotImplementedError("%s: the networks of one call must have one input size, hidden size and recurrent_N" % who)
    if H % 4 != 0 or H > 1024:
        raise NotImplementedError("%s: hidden size %d is not covered (a multiple of 4 up to 1024)" % (who, H))
    return K, H, R


def _table(tensors, offset=0):
    """HOST array of device addresses, `offset` floats into each tensor"""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() + 4 * offset for t in tensors])


class _GruSeq(torch.autograd.Function):
    """args: T, N, R, then per network x [T * N, K], h0 [N, R, H], masks [T * N] and per layer w_ih, w_hh, b_ih, b_hh.
    Returns per network y [T * N, H], hxs [N, R, H]."""

    @staticmethod
    def forward(ctx, T, N, R, *args):
        per = 3 + 4 * R
        G = len(args) // per
        nets = [args[g * per:(g + 1) * per] for g in range(G)]
        dev = nets[0][0].device
        H = nets[0][1].shape[2]
        L, idx, stream = _lib.for_device(dev)
        masks = [net[2] for net in nets]
        inp = [net[0] for net in nets]
        saved, last = [], []
        for l in range(R):
            w_ih, w_hh, b_ih, b_hh = ([net[3 + 4 * l + k] for net in nets] for k in range(4))
            gi = [torch.addmm(b_ih[g], inp[g], w_ih[g].t()) for g in range(G)]                       # [T * N, 3H]
            gh = [torch.empty(T, N, 3 * H, device=dev) for _ in range(G)]
            hb = [torch.empty(T + 1, N, H, device=dev) for _ in range(G)]
            w_hh_t = [w.t() for w in w_hh]
            bh = _table(b_hh)
            for g in range(G):
                hb[g][0].copy_(nets[g][1][:, l])
            for t in range(T):
                for g in range(G):
                    torch.mm(hb[g][t], w_hh_t[g], out=gh[g][t])
                _lib.check(L.mms_gru_gates_group(idx, G, N, H, _table(gi, t * N * 3 * H), _table(gh, t * N * 3 * H), 3 * H, _table(hb, t * N * H), H,
                                                 _table(masks, t * N), 1, bh, _table(hb, (t + 1) * N * H), H, None, stream), None, "mms_gru_gates_group", L)
            saved.append((inp, gi, gh, hb))
            last.append([b[T] for b in hb])
            inp = [b[1:].reshape(T * N, H) for b in hb]
        ctx.dims = (T, N, R, G, H)
        ctx.save_for_backward(*args)
        ctx.blocks = saved
        out = []
        for g in range(G):
            out += [inp[g], torch.stack([last[l][g] for l in range(R)], 1)]
        return tuple(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        T, N, R, G, H = ctx.dims
        per = 3 + 4 * R
        nets = [ctx.saved_tensors[g * per:(g + 1) * per] for g in range(G)]
        need = ctx.needs_input_grad[3:]
        dev = nets[0][0].device
        L, idx, stream = _lib.for_device(dev)
        masks = [net[2] for net in nets]
        dense = lambda t: None if t is None else t.to(torch.float32).contiguous()                    # (a .sum() upstream delivers a stride-0 expanded tensor)
        d_y = [dense(grads[2 * g]) for g in range(G)]
        d_hx = [dense(grads[2 * g + 1]) for g in range(G)]
        out = [None] * (G * per)
        d_h0 = [torch.empty(N, R, H, device=dev) if need[g * per + 1] else None for g in range(G)]
        nbytes = ctypes.c_int64(-1)
        for l in reversed(range(R)):
            inp, gi, gh, hb = ctx.blocks[l]
            w_ih, w_hh, b_ih, b_hh = ([net[3 + 4 * l + k] for net in nets] for k in range(4))
            want = [any(need[g * per + 3 + 4 * l + k] for k in range(4)) for g in range(G)]
            dgi = [torch.empty(T, N, 3 * H, device=dev) for _ in range(G)]
            dgh = [torch.empty(T, N, 3 * H, device=dev) for _ in range(G)]
            dbias = [torch.empty(T, 4 * H, device=dev) if want[g] else None for g in range(G)]
            cur = [d_hx[g][:, l].clone() if d_hx[g] is not None else torch.zeros(N, H, device=dev) for g in range(G)]      # (a destination later)
            nxt = [torch.empty(N, H, device=dev) for _ in range(G)]
            bh = _table(b_hh)
            for g in range(G):
                if d_y[g] is None:                                                                   # (a zero block: the tables stay whole)
                    d_y[g] = torch.zeros(T * N, H, device=dev)
            for t in reversed(range(T)):
                db = (ctypes.c_void_p * G)(*[None if b is None else b.data_ptr() + 16 * H * t for b in dbias]) if any(want) else None
                head = (idx, G, N, H, _table(gi, t * N * 3 * H), _table(gh, t * N * 3 * H), 3 * H, _table(hb, t * N * H), H, _table(masks, t * N), 1, bh,
                        _table(cur), H, _table(d_y, t * N * H), H, _table(dgi, t * N * 3 * H), _table(dgh, t * N * 3 * H), 3 * H, _table(nxt), H, db)
                if nbytes.value < 0:
                    _lib.check(L.mms_gru_gates_grad_group(*head, None, ctypes.byref(nbytes), stream), None, "mms_gru_gates_grad_group size query", L)
                    ws = ctypes.c_void_p(_workspace(nbytes.value, dev))
                _lib.check(L.mms_gru_gates_grad_group(*head, ws, ctypes.byref(nbytes), stream), None, "mms_gru_gates_grad_group", L)
                for g in range(G):
                    nxt[g].addmm_(dgh[g][t], w_hh[g])                                                 # dh_{t-1} = dh + dgh_t W_hh
                cur, nxt = nxt, cur
            for g in range(G):
                base = g * per + 3 + 4 * l
                di, dg = dgi[g].view(T * N, 3 * H), dgh[g].view(T * N, 3 * H)
                if d_h0[g] is not None:
                    d_h0[g][:, l].copy_(cur[g])
                if need[base]:
                    out[base] = di.t() @ inp[g]
                if need[base + 1]:
                    out[base + 1] = dg.t() @ hb[g][:T].view(T * N, H)
                if want[g]:
                    s = dbias[g].sum(0, dtype=torch.float64).to(torch.float32)                       # [T, 4H] over T in double, the library's fixed order, rounded once
                    out[base + 2] = s[:3 * H] if need[base + 2] else None
                    out[base + 3] = torch.cat([s[:2 * H], s[3 * H:]]) if need[base + 3] else None
                d_y[g] = di @ w_ih[g] if (l > 0 or need[g * per]) else None                          # dX: the lower layer's dy
        for g in range(G):
            out[g * per] = d_y[g] if need[g * per] else None
            out[g * per + 1] = d_h0[g]
        return (None, None, None) + tuple(out)


def gru_sequence(xs, h0s, masks, grus):
    """RNNLayer.forward's sequence (or single-step: T = 1) branch up to, but not including, `self.norm`, for a list of networks in grouped
    calls.  xs[g] [T * N, K] time-major rows, h0s[g] [N, recurrent_N, H], masks [T * N, 1] (one tensor for all networks, or a list), grus[g]
    the network's nn.GRU.  Returns [(y [T * N, H], hxs [N, recurrent_N, H])] per network.  Masks must be 0 / 1 (module docstring).
    Differentiable once in xs, h0s and the GRUs' parameters; a gradient on hxs is accepted."""
    K, H, R = check_grus(grus)
    G = len(grus)
    if not (len(xs) == len(h0s) == G):
        raise ValueError("gru_sequence: one x and one h0 per GRU")
    masks = list(masks) if isinstance(masks, (list, tuple)) else [masks] * G
    N = h0s[0].shape[0]
    rows = xs[0].shape[0]
    if N < 1 or rows % N != 0 or rows == 0:
        raise ValueError("gru_sequence: the rows (%d) must be T * N with N = h0.size(0) = %d" % (rows, N))
    T = rows // N
    args = []
    for x, h0, m, gru in zip(xs, h0s, masks, grus):
        if tuple(x.shape) != (rows, K) or tuple(h0.shape) != (N, R, H) or m.numel() != rows:
            raise NotImplementedError("gru_sequence: networks of unequal shape (x [T * N, %d], h0 [N, %d, %d], masks [T * N, 1] for every one)" % (K, R, H))
        if x.device != xs[0].device or x.dtype != torch.float32 or h0.dtype != torch.float32:
            raise NotImplementedError("gru_sequence: fp32 tensors on one device")
        args += [x.contiguous(), h0.contiguous(), m.detach().to(torch.float32).reshape(rows).contiguous()]
        for l in range(R):
            args += [getattr(gru, "%s_l%d" % (name, l)) for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    out = _GruSeq.apply(T, N, R, *args)
    return [(out[2 * g], out[2 * g + 1]) for g in range(G)]

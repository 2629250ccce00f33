"""MLPBase.forward (agents/algorithms/utils/mlp.py:59-66, 31-35) for a list of networks with the element-wise part of every
`Linear + ELU + LayerNorm` block and its backward in HIP: `mlp_base`, what the MAPPO / HAPPO trainers run with `fused_block_update`
(trainer.py).

torch runs a block as addmm, elu, layer_norm and, backward, the LayerNorm backward (two kernels), elu_backward, a column sum for the
bias gradient and the two products, with three [M, H] tensors saved.  Here, per block level, for G networks of one width:
  forward   one library product z = x W^T per network (no bias), then ONE mms_elu_ln_group call for all networks: y and the rows'
            (mean, rstd).  Saved: z and stat (besides the inputs x, W, bias, gamma, which autograd holds anyway).
  backward  ONE mms_elu_ln_grad_group call for all networks that received a gradient: dz and [dbias | dgamma | dbeta] (column sums in
            double in a fixed order; csrc/elu_ln_kernels.hip), then the library's dW = dz^T x and dx = dz W per network.
`feature_norm` stays torch's (the observation widths need not be multiples of 4 and the observation needs no gradient).  Every matrix
product is the library's; nothing here synchronises with the host.  torch "cpu" tensors go through the CPU build of the same entries (an
explicit choice of device, not a fallback).  The backward is once-differentiable.  What the entries do not take raises
NotImplementedError (check_blocks).

`products="f16x2"` (opt-in; the trainers' `block_products`): the FORWARD products z = x W^T run on the two-plane fp16 layer kernel
(mms_linear_group_act_split16, out_mode 0, identity, a zero bias vector: z stays the bias-free product that the backward reads)
instead of the library, all networks of a level in one launch -- level 0 per input width, since the actor's and the critic's differ.
Per call: ONE mms_weight_planes16_group launch for every block's Linear.weight (the weights change with every update: nothing is kept
from call to call), one mms_split_planes16_group per input width for the normalised inputs, and at every level but the last
mms_elu_ln_planes16_group in mms_elu_ln_group's place, which leaves y as fp32 (the backward's library products read it) AND as the next
level's operand planes.  What is saved and the whole backward are the default route's.  It needs a hidden width and an M that are
multiples of 128 (the layer kernel's tiles); anything else raises NotImplementedError."""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ... import _lib
from ..rl.ppo.loss import _workspace       # (the device's cached, 256-byte aligned workspace: one per process, calls run in stream order)

MAX_GROUPS = 32                             # include/mms.h: MMS_MAX_GROUPS
PRODUCTS = ("library", "f16x2")
TILE = 128                                  # mms_linear_group_act_split16: M and N in multiples of 128


def _blocks(base):
    return [base.mlp.fc1] + list(base.mlp.fc2)


def check_blocks(bases, who="mlp_base", products="library"):
    """(hidden width, number of blocks, eps) of the networks' MLPBase modules, or NotImplementedError for what mlp_base does not cover
    with these forward products (ValueError for products that do not exist)"""
    if products not in PRODUCTS:
        raise ValueError("%s: products must be one of %s, got %r" % (who, PRODUCTS, products))
    bases = list(bases)
    if not bases or len(bases) > MAX_GROUPS:
        raise NotImplementedError("%s: 1..%d networks per call, got %d" % (who, MAX_GROUPS, len(bases)))
    shapes, eps = [], set()
    for base in bases:
        mlp = getattr(base, "mlp", None)
        if mlp is None or not hasattr(mlp, "fc1") or not hasattr(mlp, "fc2"):
            raise NotImplementedError("%s: every network's base must be an MLPBase (.mlp.fc1, .mlp.fc2), got %s" % (who, type(base).__name__))
        blocks = _blocks(base)
        for blk in blocks:
            if not (isinstance(blk, nn.Sequential) and len(blk) == 3 and isinstance(blk[0], nn.Linear) and isinstance(blk[1], nn.ELU) and
                    isinstance(blk[2], nn.LayerNorm)):
                raise NotImplementedError("%s: every block must be Sequential(Linear, ELU, LayerNorm)" % who)
            lin, act, ln = blk
            if lin.bias is None or act.alpha != 1.0 or not ln.elementwise_affine or ln.bias is None or tuple(ln.normalized_shape) != (lin.out_features,):
                raise NotImplementedError("%s: only Linear with bias, ELU(alpha=1) and an affine LayerNorm over the last dimension" % who)
            if any(p.dtype != torch.float32 for p in blk.parameters()):
                raise NotImplementedError("%s: fp32 parameters only" % who)
            eps.add(float(ln.eps))
        widths = {blk[0].out_features for blk in blocks}
        if len(widths) != 1 or any(blk[0].in_features != blocks[0][0].out_features for blk in blocks[1:]):
            raise NotImplementedError("%s: the blocks of a network must have one hidden width" % who)
        shapes.append((widths.pop(), len(blocks)))
    if len(eps) != 1:
        raise NotImplementedError("%s: the LayerNorms must have one eps, got %s" % (who, sorted(eps)))
    H, n = shapes[0]
    if any(s != (H, n) for s in shapes):
        raise NotImplementedError("%s: the networks of one call must have one hidden width and one number of blocks" % who)
    if H % 4 != 0 or H > 1024:
        raise NotImplementedError("%s: hidden width %d is not covered (a multiple of 4 up to 1024)" % (who, H))
    if products == "f16x2" and H % TILE != 0:
        raise NotImplementedError("%s: products=\"f16x2\" needs a hidden width that is a multiple of %d, got %d" % (who, TILE, H))
    return H, n, eps.pop()


_table = _lib.ptr_array                                        # HOST array of device addresses (None: NULL)


class _Planes:
    """What one mlp_base(products="f16x2") call carries from level to level: the H32 planes (include/mms.h) and inverse row scales of
    every block's Linear.weight, made here in one launch, the zero bias vector of the products, and `x`: per network the (planes,
    inverse row scales) of the coming level's input -- the normalised inputs first (split), then what mms_elu_ln_planes16_group left."""

    def __init__(self, bases, n, H, dev):
        self.dev, self.H, self.last = dev, H, n - 1
        self.lib, self.idx, self.stream = _lib.for_device(dev)
        lins = [_blocks(base)[l][0] for l in range(n) for base in bases]                               # level-major: [l * G + g]
        G, Ks = len(bases), [lin.in_features for lin in lins]
        sizes = [(_lib.h32_bytes(H, K) + 255) // 256 * 256 for K in Ks]
        arena = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        planes = list(arena.split(sizes))
        scale, inv = torch.empty(len(lins), H, device=dev), torch.empty(len(lins), H, device=dev)      # (rows of H floats: 16-byte aligned)
        ws = [lin.weight.detach().contiguous() for lin in lins]
        for i in range(0, len(lins), MAX_GROUPS):                                                      # (one launch up to 32 matrices)
            j = min(i + MAX_GROUPS, len(lins))
            _lib.check(self.lib.mms_weight_planes16_group(self.idx, j - i, (ctypes.c_int64 * (j - i))(*[H] * (j - i)), (ctypes.c_int32 * (j - i))(*Ks[i:j]),
                                                          _table(ws[i:j]), _table(planes[i:j]), _table(list(scale[i:j])), _table(list(inv[i:j])), None, self.stream),
                       None, "mms_weight_planes16_group", self.lib)
        self.w = [[(planes[l * G + g], inv[l * G + g]) for g in range(G)] for l in range(n)]
        self.zero = torch.zeros(H, device=dev)
        self.x, self.level = None, 0

    def _sets(self, widths):
        """positions of the networks of one input width, in order of first appearance"""
        sets = {}
        for g, K in enumerate(widths):
            sets.setdefault(K, []).append(g)
        return sets.items()

    def split(self, hs):
        """level 0's operands: one mms_split_planes16_group call per input width over the normalised inputs hs[g] [M, K_g]"""
        M = hs[0].shape[0]
        self.x = [(torch.empty(_lib.h32_bytes(M, h.shape[1]), dtype=torch.uint8, device=self.dev), torch.empty(M, device=self.dev)) for h in hs]
        for K, gs in self._sets([h.shape[1] for h in hs]):
            _lib.check(self.lib.mms_split_planes16_group(self.idx, len(gs), M, K, K, _table([hs[g] for g in gs]), _table([self.x[g][0] for g in gs]),
                                                         _table([None] * len(gs)), _table([self.x[g][1] for g in gs]), 0, 0, None, None, None, None, 0.0,
                                                         self.stream), None, "mms_split_planes16_group", self.lib)

    def products(self, M, widths):
        """z_g [M, H] fp32 = x_g W_g^T of this level from the operands' planes: one grouped launch per input width (one, behind level 0)"""
        z = [torch.empty(M, self.H, device=self.dev) for _ in widths]
        w = self.w[self.level]
        for K, gs in self._sets(widths):
            _lib.check(self.lib.mms_linear_group_act_split16(self.idx, len(gs), M, self.H, K, _table([self.x[g][0] for g in gs]), _table([w[g][0] for g in gs]),
                                                             _table([self.zero] * len(gs)), _table([z[g] for g in gs]), _table([self.x[g][1] for g in gs]),
                                                             _table([w[g][1] for g in gs]), None, 0, 0, None, None, None, None, None, None, self.stream),
                       None, "mms_linear_group_act_split16", self.lib)
        return z


class _EluLnLevel(torch.autograd.Function):
    """One block level of G networks.  args: eps, planes (None: the library's products; a _Planes: the plane kernel's, whose operands it
    holds and whose next operands this level leaves in it), then per network x [M, K_g], weight [H, K_g], bias, gamma, beta [H].
    Returns y [M, H] per network."""

    @staticmethod
    def forward(ctx, eps, planes, *args):
        G = len(args) // 5
        nets = [args[5 * g:5 * g + 5] for g in range(G)]
        dev = nets[0][0].device
        M, H = nets[0][0].shape[0], nets[0][1].shape[0]
        L, idx, stream = _lib.for_device(dev)
        y = [torch.empty(M, H, device=dev) for _ in range(G)]
        stat = [torch.empty(M, 2, device=dev) for _ in range(G)]
        if planes is None:
            z = [torch.mm(x, w.t()) for x, w, _, _, _ in nets]
        else:
            z = planes.products(M, [n[0].shape[1] for n in nets])
        head = (idx, G, M, H, eps, _table(z), H, _table([n[2] for n in nets]), _table([n[3] for n in nets]), _table([n[4] for n in nets]), _table(y), H, _table(stat))
        if planes is None or planes.level == planes.last:
            _lib.check(L.mms_elu_ln_group(*head, stream), None, "mms_elu_ln_group", L)
        else:
            planes.x = [(torch.empty(_lib.h32_bytes(M, H), dtype=torch.uint8, device=dev), torch.empty(M, device=dev)) for _ in range(G)]
            planes.level += 1
            _lib.check(L.mms_elu_ln_planes16_group(*head, _table([p for p, _ in planes.x]), _table([None] * G), _table([i for _, i in planes.x]), stream), None,
                       "mms_elu_ln_planes16_group", L)
        ctx.save_for_backward(*args, *z, *stat)
        ctx.set_materialize_grads(False)                            # (an output nobody used arrives as None in backward, not as zeros)
        return tuple(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        G = len(grads)
        saved = ctx.saved_tensors
        nets = [saved[5 * g:5 * g + 5] for g in range(G)]
        z, stat = saved[5 * G:6 * G], saved[6 * G:7 * G]
        need = ctx.needs_input_grad[2:]
        dev = nets[0][0].device
        M, H = z[0].shape
        L, idx, stream = _lib.for_device(dev)
        out = [None] * (5 * G)
        live = [g for g in range(G) if grads[g] is not None and any(need[5 * g:5 * g + 5])]      # (a network without a gradient: None everywhere)
        if not live:
            return (None, None) + tuple(out)
        dy = [grads[g].to(torch.float32).contiguous() for g in live]                               # (a .sum() upstream delivers a stride-0 expanded tensor)
        dz = [torch.empty(M, H, device=dev) for _ in live]
        dparams = [torch.empty(3 * H, device=dev) if any(need[5 * g + 2:5 * g + 5]) else None for g in live]
        head = (idx, len(live), M, H, _table([z[g] for g in live]), H, _table([nets[g][2] for g in live]), _table([nets[g][3] for g in live]),
                _table([stat[g] for g in live]), _table(dy), H, _table(dz), H, _table(dparams))
        nbytes = ctypes.c_int64(-1)
        _lib.check(L.mms_elu_ln_grad_group(*head, None, ctypes.byref(nbytes), stream), None, "mms_elu_ln_grad_group size query", L)
        ws = ctypes.c_void_p(_workspace(nbytes.value, dev))
        _lib.check(L.mms_elu_ln_grad_group(*head, ws, ctypes.byref(nbytes), stream), None, "mms_elu_ln_grad_group", L)
        for i, g in enumerate(live):
            x, w = nets[g][0], nets[g][1]
            if need[5 * g]:
                out[5 * g] = dz[i] @ w
            if need[5 * g + 1]:
                out[5 * g + 1] = dz[i].t() @ x
            for k in range(3):
                if need[5 * g + 2 + k]:
                    out[5 * g + 2 + k] = dparams[i][k * H:(k + 1) * H]
        return (None, None) + tuple(out)


def mlp_base(xs, bases, products="library"):
    """MLPBase.forward for a list of networks in grouped calls: xs[g] [M, input width of bases[g]] -> [y_g [M, H]].  Differentiable once
    in xs and the modules' parameters.  products: who multiplies in the forward (module docstring)."""
    H, n, eps = check_blocks(bases, products=products)
    xs, bases = list(xs), list(bases)
    if len(xs) != len(bases):
        raise ValueError("mlp_base: one x per base")
    M = xs[0].shape[0]
    for x, base in zip(xs, bases):
        if x.dim() != 2 or x.shape[0] != M or x.shape[1] != base.mlp.fc1[0].in_features:
            raise NotImplementedError("mlp_base: x must be [M, input width] with one M for every network")
        if x.device != xs[0].device or x.dtype != torch.float32:
            raise NotImplementedError("mlp_base: fp32 tensors on one device")
    if products == "f16x2" and M % TILE != 0:
        raise NotImplementedError("mlp_base: products=\"f16x2\" needs M in multiples of %d, got M = %d" % (TILE, M))
    hs = [base.feature_norm(x) if getattr(base, "_use_feature_normalization", hasattr(base, "feature_norm")) else x for x, base in zip(xs, bases)]
    hs = [h.contiguous() for h in hs]
    planes = None
    if products == "f16x2" and M > 0:
        planes = _Planes(bases, n, H, hs[0].device)
        planes.split([h.detach() for h in hs])
    for l in range(n):
        args = []
        for h, base in zip(hs, bases):
            lin, _, ln = _blocks(base)[l]
            args += [h, lin.weight, lin.bias, ln.weight, ln.bias]
        hs = list(_EluLnLevel.apply(eps, planes, *args))
    return hs

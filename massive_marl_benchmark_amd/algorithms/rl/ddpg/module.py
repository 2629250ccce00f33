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

`layers="f16x2"` (constructor keyword of MLPActor, MLPQFunction and MLPActorCritic; the default is "fp32", which is everything above,
launch for launch and bit for bit) moves the hidden Linear + activation pairs of those fused paths from the exact-fp32 MFMA kernel to
the two-plane fp16 kernel the PPO modules use, `mms_linear_group_act_split16` (`split16_hidden`).  What it trades, in the words of
include/mms.h: "x s = hi + lo 2^-11 with s a power of two per ROW ... the operand is kept to 2^-22 |x| (worst case; 4e-8 rms) instead
of exactly", relative to the row's bound, and the product is three f16 MFMA products with fp32 accumulation instead of fp32 ones.  The
critics' cat(obs, act) is then never written: `mms_split_planes16_cat` reads the two halves where they lie.  The weights' planes are
rebuilt from the parameters on EVERY call (two launches), so an optimizer step or a polyak update between two calls -- or between two
replays of a captured graph -- is followed with no validity rule at all.  Shapes the kernel does not take (batch or a hidden width
not a multiple of 128) run the "fp32" chain and give its bits.  The actor's Linear(H, act_dim) + tanh stays one `mms_linear2_act`
launch, the critics' Linear(H, 1) stays inside `mms_q_heads_backup`.

`fused_grad=True` (constructor keyword of MLPActor and MLPActorCritic, which hands it down; the default False is everything above, launch
for launch) gives the actor's last layer -- Linear(H, act_dim) + tanh + act_limit -- to the two entries `mms_det_heads_act` /
`mms_det_heads_grad`, on "cuda" and, through the CPU build, on "cpu":
  * where a gradient is wanted (compute_loss_pi, td3.py:383-388) the hidden layers stay in torch and the head is `_DetHead`: one
    `mms_det_heads_act` launch forward (the action, and tanh(pre) kept for the backward), one `mms_det_heads_grad` call plus the two
    library products backward.  Once differentiable: `create_graph=True` raises.
  * where none is wanted the head is one `mms_det_heads_act` launch behind the hidden-layer paths above.
  * `MLPActor.smoothed(obs, sigma, noise_clip)` is the no-gradient target action of td3.py:361-367 (ddpg.py:357-365 smooths too) with
    the noise and both clamps inside that launch; `MLPActorCritic.act(deterministic=False)` on the HIP device takes its exploration
    noise there as well (`sigma = act_noise`, no noise clip).
  * `MLPActorCritic.q_loss` / `pi_loss` are compute_loss_q / compute_loss_pi on sac.loss.q_heads_loss; `pi_loss` has the head write the
    action into the action columns of the critic's `[o | a]` input block, so no `torch.cat` runs, and the backward reads the action
    columns of that block's gradient where they lie.
A head the entries do not take (dtype, H not a multiple of 64, act_dim > 128, alignment, another device) runs the torch expression; that
is decided before anything is launched.  The noise of the fused head is this build's counter stream keyed (seed, row_offset + row, the
row's draw counter, column), not torch's generator: another stream of normals, the same distribution.  Seed, counters and row_offset are
owned as sac.module's actor owns them (`_NoiseOwner`): plain attributes, not buffers -- the state_dict keys stay the reference's -- with
the counters pinned once a graph capture has used them (`pi.reserve_counters(rows, device)` before capturing).
"""
import copy
import ctypes

import torch
import torch.nn as nn

from .... import _lib
from ....engine import current_stream_ptr

_ACT_CODES = {nn.Identity: 0, nn.ELU: 1, nn.ReLU: 2, nn.Tanh: 3}
_Q_MAX_H = 4096          # include/mms.h: MMS_Q_MAX_H


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _draw_seed():
    """A noise-stream key from torch's default generator, so that torch.manual_seed makes runs reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class _NoiseOwner:
    """What an actor with a fused sampling head keeps besides its layers: `seed`, `row_offset` (global index of row 0: data-parallel
    shards draw disjoint rows) and the per-row draw counters -- a plain device tensor, not a buffer, grown to the largest row count
    seen.  A captured graph holds only the counters' device address, so once a graph capture has used them they are pinned: a call
    that would need more rows (or another device) raises instead of moving them."""

    def _init_noise(self, seed, row_offset):
        self.seed = int(seed)
        self.row_offset = int(row_offset)
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
                raise RuntimeError("%s: %d rows on %s need new draw counters, but a graph capture holds or is recording the current "
                                   "ones (%s); call pi.reserve_counters(<largest row count>, device) before capturing"
                                   % (type(self).__name__, n, torch.device(device), "none" if c is None else "%d on %s" % (c.numel(), c.device)))
            old = None if c is None else c.to(device)
            c = torch.zeros(max(n, 0 if old is None else old.numel()), dtype=torch.int64, device=device)
            if old is not None:
                c[:old.numel()].copy_(old)
            self._counters = c
        return c

    def _draw_counters(self, n, device):
        """The counters for a call that draws, pinned if a capture is recording it."""
        c = self.counters(n, device)
        if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            self._counters_pinned = True
        return c


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


LAYERS = ("fp32", "f16x2")
_MAX_GROUPS = 32         # include/mms.h: MMS_MAX_GROUPS
_last_split16 = None     # the launch arguments of a split16_hidden call without a scratch dict: referenced until the next one




class _Split16Owner:
    """What a module with the `layers` keyword keeps: the setting and a plain dict of split16_hidden's scratch memory.  The dict is
    no parameter and no buffer (state_dict keys stay the reference's); a deepcopy (actor_critic_targ) and a pickle get an EMPTY one."""

    def _init_layers(self, layers):
        if layers not in LAYERS:
            raise ValueError("layers must be one of %s, not %r" % (LAYERS, layers))
        self.layers = layers
        self._split16_scratch = {}

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_split16_scratch" else copy.deepcopy(v, memo)
        return new

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_split16_scratch"] = {}
        return state


def split16_hidden(nets, x_or_pair, scratch=None):
    """The hidden Linear + activation pairs of one or two networks of equal shape (`nets`: nn.Sequential prefixes) on two scaled fp16
    planes per operand; the input is a 2-D fp32 tensor or an (obs, act) pair whose row-wise concatenation the networks take (never
    written).  Returns the last hidden activations [M, H] f32 per network (fresh tensors), or None -- decided before the first launch
    -- when anything does not qualify: fp32, dense 16-byte aligned parameters, ELU / ReLU / Tanh / Identity, M > 0 and every hidden
    width multiples of 128, nothing wanting a gradient.  The library is the input's device's (_lib.for_device): the CPU build runs it too.

    Every call, in order: mms_weight_planes16_group over all hidden matrices of all nets (planes, row scales, row 1-norms),
    mms_chain_refresh16 with rows = 0 (the bound chain), mms_split_planes16_cat (a pair) or mms_split_planes16_group (one split
    serves every network; it also leaves each row's hidden scales), then one mms_linear_group_act_split16 per layer for all nets,
    planes out (out_mode 1) but for the last (f32).  The weights are re-split UNCONDITIONALLY: there is no version counter, address
    tag or refresh(), so whatever rewrote the parameters since the last call (optimizer.step(), the polyak loop, .data writes) is in
    this result.  No host synchronisation: after one call that allocated the scratch the sequence is graph-capturable.
    `scratch`: the owning module's dict; it keeps device scratch memory per (device, M, layer shapes, number of nets) and, until
    the next call, the ctypes arrays and every tensor the launches read."""
    global _last_split16
    nets = [list(n) for n in nets]
    pair = isinstance(x_or_pair, (tuple, list))
    xs = list(x_or_pair) if pair else [x_or_pair]
    G = len(nets)
    if G not in (1, 2) or len(xs) != (2 if pair else 1) or any(len(m) != len(nets[0]) or len(m) % 2 or len(m) < 2 for m in nets):
        return None
    x0 = xs[0]
    for x in xs:
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or x.device != x0.device or x.shape[0] != x0.shape[0] or x.shape[1] < 1:
            return None
        if x.stride(1) != 1 or x.stride(0) < x.shape[1] or x.data_ptr() % 4:
            return None
    dev, M = x0.device, x0.shape[0]
    if dev.type not in ("cuda", "cpu") or M <= 0 or M % 128:
        return None
    nl = len(nets[0]) // 2
    if G * nl > _MAX_GROUPS:
        return None
    grad = torch.is_grad_enabled()
    if grad and any(x.requires_grad for x in xs):
        return None
    K_in = sum(x.shape[1] for x in xs)
    for m in nets:
        for i in range(nl):
            lin, fn, lin0, fn0 = m[2 * i], m[2 * i + 1], nets[0][2 * i], nets[0][2 * i + 1]
            if not isinstance(lin, nn.Linear) or lin.bias is None or type(fn) not in _ACT_CODES or type(fn) is not type(fn0):
                return None
            if isinstance(fn, nn.ELU) and fn.alpha != 1.0:
                return None
            if not isinstance(lin0, nn.Linear) or (lin.in_features, lin.out_features) != (lin0.in_features, lin0.out_features) or lin.out_features % 128:
                return None
            for t in (lin.weight, lin.bias):
                if t.dtype != torch.float32 or t.device != dev or not _kernel_layout(t) or (grad and t.requires_grad):
                    return None
            if lin.in_features != (K_in if i == 0 else m[2 * i - 2].out_features):
                return None
    acts = [_ACT_CODES[type(nets[0][2 * i + 1])] for i in range(nl)]
    lins = [[m[2 * i] for i in range(nl)] for m in nets]
    shapes = tuple((l.out_features, l.in_features) for l in lins[0])
    Lh = nl - 1                                           # layers whose output stays in planes: the bound chain's length
    L, idx, stream = _lib.for_device(dev)
    key = (str(dev), M, shapes, G)
    holder = scratch if scratch is not None else {}
    buf = holder.get(key)
    if buf is None:
        f32 = lambda *s: torch.empty(*s, device=dev)
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        buf = {"w": [[(u8(_lib.h32_bytes(N, K)), f32(N), f32(N), f32(N)) for N, K in shapes] for _ in range(G)],     # planes, scale, inv, l1
               "chain": torch.zeros(G, max(Lh, 1), 2, device=dev),
               "x": u8(_lib.h32_bytes(M, K_in)), "xs": f32(M), "xi": f32(M), "cs": f32(G, max(Lh, 1), M), "ci": f32(G, max(Lh, 1), M),
               "h": [[u8(_lib.h32_bytes(M, N)) for N, _ in shapes[:-1]] for _ in range(G)]}
        holder[key] = buf
    out = [torch.empty(M, shapes[-1][0], device=dev) for _ in range(G)]
    vp = ctypes.c_void_p
    arr = lambda ts: (vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    p = lambda t: vp(t.data_ptr())
    flat = [(lins[g][i], buf["w"][g][i]) for g in range(G) for i in range(nl)]
    ws, bs = [l.weight.detach() for l, _ in flat], [[l.bias.detach() for l in lins[g]] for g in range(G)]
    keep = [xs, ws, bs, out, buf]
    calls = [(L.mms_weight_planes16_group, (idx, len(flat), (ctypes.c_int64 * len(flat))(*[l.out_features for l, _ in flat]),
                                            (ctypes.c_int32 * len(flat))(*[l.in_features for l, _ in flat]), arr(ws), arr([b[0] for _, b in flat]),
                                            arr([b[1] for _, b in flat]), arr([b[2] for _, b in flat]), arr([b[3] for _, b in flat])), "mms_weight_planes16_group")]
    if Lh:
        ent = [(g, i) for g in range(G) for i in range(Lh)]
        calls.append((L.mms_chain_refresh16, (idx, G, Lh, arr([buf["w"][g][i][3] for g, i in ent]), arr([bs[g][i] for g, i in ent]),
                                              (ctypes.c_int32 * len(ent))(*[shapes[i][0] for _, i in ent]), p(buf["chain"]), 0.0, 0, None, None), "mms_chain_refresh16"))
    nch = G if Lh else 0
    if pair:
        calls.append((L.mms_split_planes16_cat, (idx, M, xs[0].shape[1], xs[0].stride(0), p(xs[0]), xs[1].shape[1], xs[1].stride(0), p(xs[1]), p(buf["x"]), None,
                                                 p(buf["xi"]), nch, Lh, p(buf["chain"]) if nch else None, p(buf["cs"]) if nch else None,
                                                 p(buf["ci"]) if nch else None), "mms_split_planes16_cat"))
    else:
        calls.append((L.mms_split_planes16_group, (idx, 1, M, K_in, x0.stride(0), arr([x0]), arr([buf["x"]]), arr([buf["xs"]]), arr([buf["xi"]]), nch, Lh,
                                                   arr([buf["chain"]]) if nch else None, arr([buf["cs"]]) if nch else None, arr([buf["ci"]]) if nch else None,
                                                   None, 0.0), "mms_split_planes16_group"))
    cur, cur_inv = [buf["x"]] * G, [buf["xi"]] * G
    for i, (N, K) in enumerate(shapes):
        last = i == nl - 1
        y = out if last else [buf["h"][g][i] for g in range(G)]
        ysc = None if last else [buf["cs"][g, i] for g in range(G)]
        calls.append((L.mms_linear_group_act_split16, (idx, G, M, N, K, arr(cur), arr([buf["w"][g][i][0] for g in range(G)]), arr([bs[g][i] for g in range(G)]), arr(y),
                                                       arr(cur_inv), arr([buf["w"][g][i][2] for g in range(G)]), None if last else arr(ysc), acts[i], 0 if last else 1,
                                                       None, None, None, None, None, None), "mms_linear_group_act_split16"))
        if not last:
            cur, cur_inv = y, [buf["ci"][g, i] for g in range(G)]
            keep.append((ysc, cur_inv))
    keep.append(calls)
    if scratch is not None:
        scratch["last"] = keep
    else:
        _last_split16 = keep
    for fn, args, what in calls:
        _lib.check(fn(*args, stream), None, what, L)
    return out


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
    if len(nets[0]) > 2 and all(getattr(q, "layers", "fp32") == "f16x2" for q in qs):
        # the two-plane fp16 layers on (obs, act) where they lie: no cat; None (shapes the kernel does not take): the chain below
        hs = split16_hidden([m[:-2] for m in nets], (obs.reshape(-1, obs.shape[-1]), act.reshape(-1, act.shape[-1])), getattr(qs[0], "_split16_scratch", None))
        if hs is not None:
            return hs, [m[-2] for m in nets], obs.shape[:-1]
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


def det_head_act(hidden, weight, bias, act_limit, sigma=0.0, noise_clip=-1.0, seed=0, counters=None, row_offset=0, out=None, tanh_out=None):
    """One mms_det_heads_act call on hidden [M, H] (16-byte aligned, dense): the action into `out` ([M, A] with unit column stride and
    any row pitch; allocated when None and tanh_out is None) and tanh(pre) into `tanh_out` ([M, A] dense).  Returns `out`."""
    M, H = hidden.shape
    A = weight.shape[0]
    if out is None and tanh_out is None:
        out = torch.empty(M, A, device=hidden.device)
    L, idx, stream = _lib.for_device(hidden.device)
    _lib.check(L.mms_det_heads_act(idx, M, H, A, _p(hidden), _p(weight), _p(bias), float(act_limit), float(sigma), float(noise_clip), seed, _p(counters),
                                   row_offset, _p(out), 0 if out is None else out.stride(0), _p(tanh_out), stream), None, "mms_det_heads_act", L)
    return out


class _DetHead(torch.autograd.Function):
    """The actor's head behind its hidden layers with a gradient (`fused_grad=True`): mms_det_heads_act forward with tanh(pre) kept,
    mms_det_heads_grad + two library products backward.  With `obs` [N, W] the result is the critic's input block [o | a] ([N, W + A]:
    the head writes the action columns at pitch W + A, the observation is copied in front) and the backward reads the action columns
    of the block's gradient where they lie; with obs None the result is the action [N, A]."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, act_limit, obs):
        N, A = hidden.shape[0], weight.shape[0]
        W = 0 if obs is None else obs.shape[1]
        block = torch.empty(N, W + A, device=hidden.device)
        t = torch.empty(N, A, device=hidden.device)
        if W:
            block[:, :W].copy_(obs)
        det_head_act(hidden, weight, bias, act_limit, out=block[:, W:], tanh_out=t)
        ctx.save_for_backward(hidden, weight, t)
        ctx.act_limit, ctx.W = act_limit, W
        return block

    @staticmethod
    def backward(ctx, g):
        # once_differentiable alone raises only where the incoming gradient itself requires one; under create_graph=True with a constant
        # incoming gradient it would hand back a silently constant head: refuse that as well (sac.module._SacHead)
        if torch.is_grad_enabled():
            raise RuntimeError("MLPActor(fused_grad=True): the fused head is once differentiable (no create_graph=True)")
        return _DetHead._backward(ctx, g)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _backward(ctx, g):
        from ..ppo.loss import _workspace      # (the device's cached, 256-byte aligned workspace: calls run in stream order)
        hidden, weight, t = ctx.saved_tensors
        need = ctx.needs_input_grad
        N, A = t.shape
        W, dev = ctx.W, t.device
        if g.dtype != torch.float32 or g.stride(1) != 1 or g.stride(0) < W + A:      # (a .sum() upstream delivers a stride-0 expanded tensor)
            g = g.to(torch.float32).contiguous()
        g_obs = g[:, :W] if (W and need[4]) else None
        if not any(need[:3]):
            return None, None, None, None, g_obs
        g_act = g[:, W:]
        L, idx, stream = _lib.for_device(dev)
        dy = torch.empty(N, A, device=dev)
        dbias = torch.empty(A, device=dev) if need[2] else None
        nbytes = ctypes.c_int64(-1)
        head = (idx, N, A, ctx.act_limit, _p(t), _p(g_act), g.stride(0), _p(dy), _p(dbias))
        _lib.check(L.mms_det_heads_grad(*head, None, ctypes.byref(nbytes), stream), None, "mms_det_heads_grad size query", L)
        ws = _workspace(nbytes.value, dev)
        _lib.check(L.mms_det_heads_grad(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_det_heads_grad", L)
        return dy @ weight if need[0] else None, dy.t() @ hidden if need[1] else None, dbias, None, g_obs


class MLPActor(_NoiseOwner, _Split16Owner, nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit, seed=None, row_offset=0, fused_grad=False, layers="fp32"):
        super().__init__()
        self.pi = mlp([obs_dim, *hidden_sizes, act_dim], activation, nn.Tanh)
        self.act_limit = act_limit
        self._init_layers(layers)          # "f16x2": the hidden pairs through split16_hidden (module docstring)
        self.fused_grad = bool(fused_grad)  # True: the last layer through mms_det_heads_act / mms_det_heads_grad (module docstring)
        # drawn after the layers (their initialisation is the reference's) and only where a fused head can use it: the default
        # constructor leaves torch's generator where the reference's does
        self._init_noise(_draw_seed() if (seed is None and self.fused_grad) else (seed or 0), row_offset)

    def forward(self, obs):
        if self._head_fusable(obs):
            if torch.is_grad_enabled() and (obs.requires_grad or any(p.requires_grad for p in self.parameters())):
                return self._block(obs, None)
            return self._fused_head(obs)
        return self.torch_forward(obs)

    def torch_forward(self, obs):
        """`fused_grad=False`, and every head the entries do not take: the hidden-layer paths of the module docstring, torch otherwise."""
        out = None
        if self.layers == "f16x2" and obs.is_cuda and obs.dim() == 2 and len(self.pi) > 2:
            hs = split16_hidden([list(self.pi)[:-2]], obs, self._split16_scratch)
            if hs is not None:             # Linear(H, act_dim) + tanh: act_dim is no multiple of 128, one mms_linear2_act launch
                out = fused_mlp_forward(self.pi[-2:], hs[0])
        if out is None:
            out = fused_mlp_forward(self.pi, obs)
        if out is None:
            out = self.pi(obs)
        return out if self.act_limit == 1.0 else self.act_limit * out       # x 1.0 is exact: one launch less for the ant / helicopter tasks

    def _head_fusable(self, obs):
        """`fused_grad=True` and the two entries take this actor's last layer for `obs`: Linear(H, A) with a bias + Tanh behind at least
        one hidden pair, fp32, dense, 16-byte aligned parameters on "cuda" or "cpu", H % 64 == 0, 1 <= A <= 128, a non-empty fp32
        input on the parameters' device.  Nothing has been launched when this returns."""
        if not self.fused_grad or len(self.pi) < 4 or not torch.is_tensor(obs) or obs.dtype != torch.float32 or obs.dim() < 1 or obs.numel() == 0:
            return False
        last, fn = self.pi[-2], self.pi[-1]
        if not isinstance(last, nn.Linear) or last.bias is None or type(fn) is not nn.Tanh:
            return False
        dev = last.weight.device
        H, A = last.in_features, last.out_features
        return (dev.type in ("cuda", "cpu") and obs.device == dev and H % 64 == 0 and 1 <= A <= 128 and obs.shape[-1] == self.pi[0].in_features
                and all(p.dtype == torch.float32 and p.device == dev and _kernel_layout(p) for p in (last.weight, last.bias)))

    def _hidden(self, x):
        """The last hidden activations [M, H] of x [M, W], dense and 16-byte aligned: without a gradient through the fused hidden-layer
        paths where they apply, in torch otherwise (autograd keeps them)."""
        body = self.pi[:-2]
        h = None
        if not torch.is_grad_enabled() or not (x.requires_grad or any(p.requires_grad for p in body.parameters())):
            if self.layers == "f16x2":
                hs = split16_hidden([list(body)], x, self._split16_scratch)
                h = None if hs is None else hs[0]
            if h is None:
                h = fused_mlp_forward(body, x)
        if h is None:
            h = body(x).contiguous()
        return h.clone() if h.data_ptr() % 16 else h

    def _fused_head(self, obs, sigma=0.0, noise_clip=-1.0):
        """No gradient: the hidden layers, then one mms_det_heads_act launch (sigma > 0: noise, clamps and counters inside it)."""
        with torch.no_grad():
            x = obs.reshape(-1, obs.shape[-1])
            h = self._hidden(x)
            counters = self._draw_counters(h.shape[0], h.device) if sigma > 0 else None
            a = det_head_act(h, self.pi[-2].weight.detach(), self.pi[-2].bias.detach(), self.act_limit, sigma, noise_clip, self.seed, counters, self.row_offset)
        return a.view(*obs.shape[:-1], a.shape[1])

    def _block(self, obs, cat_obs):
        """With a gradient: the hidden layers in torch, the head through _DetHead.  cat_obs None: the action in obs's leading shape;
        else the critic's input block [cat_obs | action] as [M, W + A] (MLPActorCritic.pi_loss)."""
        x = obs.reshape(-1, obs.shape[-1])
        last = self.pi[-2]
        out = _DetHead.apply(self._hidden(x), last.weight, last.bias, float(self.act_limit), cat_obs)
        return out.view(*obs.shape[:-1], out.shape[1]) if (cat_obs is None and obs.dim() != 2) else out

    def smoothed(self, obs, sigma, noise_clip, eps=None):
        """The target action of td3.py:361-367 / ddpg.py:357-365, no gradient: clamp(pi(obs) + clamp(sigma z, -noise_clip, noise_clip),
        -act_limit, act_limit).  On the fused path (`fused_grad=True`, a head the entry takes, no `eps`) the draw and both clamps sit
        inside the head launch and z is the counter stream; otherwise the reference's five statements, on `eps` (given standard
        normals: a recorded run) or torch.randn_like."""
        with torch.no_grad():
            if eps is None and sigma > 0 and noise_clip >= 0 and self._head_fusable(obs):
                return self._fused_head(obs, float(sigma), float(noise_clip))
            pi_targ = self(obs)
            epsilon = (torch.randn_like(pi_targ) if eps is None else eps) * sigma
            epsilon = torch.clamp(epsilon, -noise_clip, noise_clip)
            a2 = pi_targ + epsilon
            return torch.clamp(a2, -self.act_limit, self.act_limit)


class MLPQFunction(_Split16Owner, nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, fused_q=True, layers="fp32"):
        super().__init__()
        self.q = mlp([obs_dim + act_dim, *hidden_sizes, 1], activation)
        self.fused_q = bool(fused_q)       # False: torch always
        self._init_layers(layers)          # "f16x2": the fused paths' hidden pairs through split16_hidden on (obs, act), no cat

    def forward(self, obs, act):
        out = fused_q_forward([self], obs, act) if self.fused_q else None
        if out is not None:
            return out[0]
        return self.q(torch.cat([obs, act], dim=-1))      # [..., 1], as the reference returns it


class MLPActorCritic(nn.Module):
    def __init__(self, observation_space, action_space, act_noise, device, hidden_sizes=(256, 256), activation=nn.ReLU, layers="fp32",
                 fused_grad=False, seed=None, row_offset=0, fused_q=True):
        super().__init__()
        self.fused_q = bool(fused_q)
        self.fused_grad = bool(fused_grad)  # handed down to the actor (module docstring)
        if layers not in LAYERS:
            raise ValueError("layers must be one of %s, not %r" % (LAYERS, layers))
        self.layers = layers               # handed down to the actor and the critics ("f16x2": module docstring)
        obs_dim, act_dim = observation_space.shape[0], action_space.shape[0]
        self.act_limit = action_space.high[0]
        self.act_noise = act_noise
        self.device = device
        self.pi = MLPActor(obs_dim, act_dim, hidden_sizes, activation, self.act_limit, seed=0, row_offset=row_offset, fused_grad=self.fused_grad, layers=self.layers)
        self._build_q(obs_dim, act_dim, hidden_sizes, activation)
        if self.fused_grad:                # after every layer: initialisation identical to the reference's
            self.pi.seed = _draw_seed() if seed is None else int(seed)

    def _build_q(self, obs_dim, act_dim, hidden_sizes, activation):
        self.q = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, self.layers)

    def _critics(self):
        return [self.q]

    def q_backup(self, o2, a2, r, d, gamma, alpha=None, logp=None):
        """r + gamma * (1 - d) * (min over this network's critics of q(o2, a2) - alpha * logp), no gradient: called on the target
        copy it is ddpg.py:368-369 / td3.py:370-373 in one line (see fused_q_backup)."""
        return fused_q_backup(self._critics(), o2, a2, r, d, gamma, alpha, logp)

    def q_loss(self, o, a, backup):
        """compute_loss_q's loss for a given Bellman backup (ddpg.py:353, 372; td3.py:356-357, 376-378): sum over this network's critics
        of mean((q(o, a) - backup)^2).  The critics' hidden layers run in torch on cat(o, a) (autograd keeps them); the last layers, the
        loss and their backward are one mms_q_heads_loss call (sac.loss.q_heads_loss)."""
        from ..sac.loss import q_heads_loss
        qs = self._critics()
        x = torch.cat([o, a], dim=-1)
        x = x.reshape(-1, x.shape[-1])
        return q_heads_loss([q.q[:-2](x) for q in qs], [q.q[-2] for q in qs], target=backup, mode="mse")

    def pi_loss(self, o):
        """compute_loss_pi (ddpg.py:377-382; td3.py:383-388): -mean(q(o, pi(o))) over the FIRST critic only (`q`; TD3: `q1`).  With
        `fused_grad` the actor's head writes the action into the [o | a] block (no torch.cat); the critic's hidden layers run in torch,
        its last layer, the mean and their backward are one mms_q_heads_loss call.  A critic whose parameters do not require a gradient
        gets none computed."""
        from ..sac.loss import q_heads_loss
        q = self._critics()[0]
        if self.pi._head_fusable(o) and torch.is_grad_enabled():
            x = self.pi._block(o, o.reshape(-1, o.shape[-1]))
        else:
            x = torch.cat([o, self.pi(o)], dim=-1)
            x = x.reshape(-1, x.shape[-1])
        return q_heads_loss([q.q[:-2](x)], [q.q[-2]], mode="pi")

    def act(self, obs, deterministic=True):
        with torch.no_grad():
            if not deterministic and obs.is_cuda and self.act_noise > 0 and self.pi._head_fusable(obs):
                return self.pi._fused_head(obs, float(self.act_noise))      # mean + act_noise * N(0, 1) and the clamp inside the head launch
            a = self.pi(obs)
            if not deterministic:
                if a.is_cuda:      # mean + std * N(0, 1) in one launch, clamp in place (the collection loop is launch bound)
                    a = torch.normal(a, float(self.act_noise)).clamp_(-self.act_limit, self.act_limit)
                else:
                    a = torch.clamp(a + self.act_noise * torch.randn_like(a), -self.act_limit, self.act_limit)
        return a

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
"""
import copy
import ctypes

import torch
import torch.nn as nn

from .... import _lib
from ....engine import current_stream_ptr

_ACT_CODES = {nn.Identity: 0, nn.ELU: 1, nn.ReLU: 2, nn.Tanh: 3}
_Q_MAX_H = 4096          # include/mms.h: MMS_Q_MAX_H


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


class MLPActor(_Split16Owner, nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit, layers="fp32"):
        super().__init__()
        self.pi = mlp([obs_dim, *hidden_sizes, act_dim], activation, nn.Tanh)
        self.act_limit = act_limit
        self._init_layers(layers)          # "f16x2": the hidden pairs through split16_hidden (module docstring)

    def forward(self, obs):
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
    def __init__(self, observation_space, action_space, act_noise, device, hidden_sizes=(256, 256), activation=nn.ReLU, layers="fp32", fused_q=True):
        super().__init__()
        self.fused_q = bool(fused_q)
        if layers not in LAYERS:
            raise ValueError("layers must be one of %s, not %r" % (LAYERS, layers))
        self.layers = layers               # handed down to the actor and the critics ("f16x2": module docstring)
        obs_dim, act_dim = observation_space.shape[0], action_space.shape[0]
        self.act_limit = action_space.high[0]
        self.act_noise = act_noise
        self.device = device
        self.pi = MLPActor(obs_dim, act_dim, hidden_sizes, activation, self.act_limit, self.layers)
        self._build_q(obs_dim, act_dim, hidden_sizes, activation)

    def _build_q(self, obs_dim, act_dim, hidden_sizes, activation):
        self.q = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, self.layers)

    def _critics(self):
        return [self.q]

    def q_backup(self, o2, a2, r, d, gamma, alpha=None, logp=None):
        """r + gamma * (1 - d) * (min over this network's critics of q(o2, a2) - alpha * logp), no gradient: called on the target
        copy it is ddpg.py:368-369 / td3.py:370-373 in one line (see fused_q_backup)."""
        return fused_q_backup(self._critics(), o2, a2, r, d, gamma, alpha, logp)

    def act(self, obs, deterministic=True):
        with torch.no_grad():
            a = self.pi(obs)
            if not deterministic:
                if a.is_cuda:      # mean + std * N(0, 1) in one launch, clamp in place (the collection loop is launch bound)
                    a = torch.normal(a, float(self.act_noise)).clamp_(-self.act_limit, self.act_limit)
                else:
                    a = torch.clamp(a + self.act_noise * torch.randn_like(a), -self.act_limit, self.act_limit)
        return a

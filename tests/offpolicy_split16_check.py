"""Checks of the opt-in fp16-plane layers of the off-policy modules (`layers="f16x2"`: ddpg.module.split16_hidden in front of
mms_q_heads_backup / mms_sac_heads_act / the actor's last mms_linear2_act), shared by the CPU-build tests
(test_offpolicy_split16.py: split16_hidden and the tail entries on CPU tensors) and the GPU tests (test_offpolicy_split16_gpu.py:
the modules).

Error gate.  The yardstick is the exact-fp32 entry chain the modules run by default -- `fp32_hidden` below restates it: one
mms_linear2_act launch per hidden layer, both networks per launch, on torch.cat([obs, act], 1) -- on the same build, inputs and
parameters; both are compared with a float64 evaluation of the torch modules.  e = rms error of split16_hidden, ey = the yardstick's:
    e <= 1.25 ey          for the last hidden activations and for q (the project's factor for a kernel against its fp32 yardstick,
                          mlp_grad_check.py)
    max e <= 2 max ey     the ratio of the two maxima is noisy at these sample counts (0.92 - 1.5 on the CPU build); recorded
torch's fp32 modules on the same device are recorded beside them and not gated.  STATS holds what a session measured;
MMS_OFFPOLICY_SPLIT16_RECORD=<path> makes the tests write it there (profiles/offpolicy_split16_error.json)."""
import copy
import ctypes
import json

import torch
import torch.nn as nn

from massive_marl_benchmark_amd import _lib
from massive_marl_benchmark_amd.algorithms.rl.ddpg import module as ddpg_module
from massive_marl_benchmark_amd.algorithms.rl.ddpg.module import _ACT_CODES, _q_tail, split16_hidden

STATS = {}
M_SIZES = [128, 256]
WIDTHS = [(52, 24), (13, 3)]
HIDDEN = [(256, 256, 256), (128, 128)]
ACTS = [nn.ELU, nn.ReLU]


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def make_q(G, K0, K1, hidden, act, seed, dev, layers="f16x2"):
    """G critics (ddpg.MLPQFunction: `q` = hidden Linear + activation pairs, Linear(H, 1), Identity), torch's default initialisation."""
    torch.manual_seed(seed)
    return [ddpg_module.MLPQFunction(K0, K1, hidden, act, True, layers).to(dev) for _ in range(G)]


def prefixes(qs):
    return [q.q[:-2] for q in qs]


def lasts(qs):
    return [q.q[-2] for q in qs]


def inputs(M, K0, K1, seed, dev, obs_scale=1.0):
    """Observations N(0, 1) clamped to +-5 (times obs_scale), actions U(-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(M, K0, generator=g).clamp_(-5, 5) * obs_scale
    act = torch.rand(M, K1, generator=g) * 2 - 1
    return obs.to(dev), act.to(dev)


@torch.no_grad()
def fp32_hidden(nets, x):
    """The default path's hidden chain, restated: mms_linear2_act per Linear + activation pair, one or two networks per launch."""
    nets = [list(n) for n in nets]
    L, idx, stream = _lib.for_device(x.device)
    two = len(nets) == 2
    hs = [x.contiguous()] * len(nets)
    for i in range(0, len(nets[0]), 2):
        lins = [m[i] for m in nets]
        ys = [torch.empty(x.shape[0], lin.out_features, device=x.device) for lin in lins]
        _lib.check(L.mms_linear2_act(idx, x.shape[0], lins[0].out_features, lins[0].in_features, p(hs[0]), p(lins[0].weight), p(lins[0].bias), p(ys[0]),
                                     p(hs[1]) if two else None, p(lins[1].weight) if two else None, p(lins[1].bias) if two else None, p(ys[1]) if two else None,
                                     _ACT_CODES[type(nets[0][i + 1])], stream), None, "mms_linear2_act", L)
        hs = ys
    return hs


@torch.no_grad()
def q_of(hs, last):
    """mms_q_heads_backup's forward on hidden activations: [q_g [M]]."""
    out = [torch.empty(hs[0].shape[0], device=hs[0].device) for _ in hs]
    _q_tail(hs, last, out)
    return out


@torch.no_grad()
def f64(nets, last, x):
    """(hidden, q) per network in float64 from copies of the torch modules."""
    hs = [copy.deepcopy(n).double()(x.double()) for n in nets]
    return hs, [copy.deepcopy(l).double()(h)[:, 0] for l, h in zip(last, hs)]


def _rms(a, b):
    d = torch.cat([(x.double() - y).flatten() for x, y in zip(a, b)])
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


def error_case(dev, M, K0, K1, hidden, act, G, obs_scale=1.0, seed=0):
    """One shape: measure, print, record, gate."""
    qs = make_q(G, K0, K1, hidden, act, 17 + seed, dev)
    obs, a = inputs(M, K0, K1, 23 + seed, dev, obs_scale)
    x = torch.cat([obs, a], 1)
    nets, last = prefixes(qs), lasts(qs)
    with torch.no_grad():
        h16 = split16_hidden(nets, (obs, a))
        assert h16 is not None
        h32 = fp32_hidden(nets, x)
        ht = [n(x) for n in nets]
        q16, q32, qt = q_of(h16, last), q_of(h32, last), [l(h)[:, 0] for l, h in zip(last, ht)]
    h64, q64 = f64(nets, last, x)
    assert all(bool(torch.isfinite(t).all()) for t in (*h16, *q16))
    res = {}
    for name, got, yard, tor, truth in (("hidden", h16, h32, ht, h64), ("q", q16, q32, qt, q64)):
        (e, em), (ey, eym), (et, etm) = _rms(got, truth), _rms(yard, truth), _rms(tor, truth)
        res[name] = {"rms": e, "rms_fp32_entry": ey, "rms_torch": et, "rms_ratio": e / ey, "max_ratio": em / eym, "max": em, "max_fp32_entry": eym, "max_torch": etm}
    key = "%s_M%d_K%d+%d_H%s_%s_G%d_x%g" % (torch.device(dev).type, M, K0, K1, "x".join(map(str, hidden)), act.__name__, G, obs_scale)
    STATS[key] = res
    print(key, " ".join("%s: e / ey = %.3f (rms), %.3f (max), torch / ey = %.3f" % (k, v["rms_ratio"], v["max_ratio"], v["rms_torch"] / v["rms_fp32_entry"])
                        for k, v in res.items()))
    for k, v in res.items():
        assert v["rms"] <= 1.25 * v["rms_fp32_entry"], (key, k, v)
        assert v["max"] <= 2.0 * v["max_fp32_entry"], (key, k, v)
    return res


def write_error_record(path, what):
    if path and STATS:
        with open(path, "w") as f:
            json.dump({"what": what, "shapes": STATS}, f, indent=1, sort_keys=True)


RECORD_WHAT = ("split16_hidden (layers=\"f16x2\") against the exact-fp32 entry chain (mms_linear2_act) on the same build, inputs and parameters, both against a "
               "float64 evaluation of the torch modules (tests/offpolicy_split16_check.py::error_case): rms and max error of the last hidden activations and of "
               "q, their ratios (gates: rms <= 1.25 x, max <= 2 x), and torch's fp32 modules on the same device beside them (not gated).")


def zero_rows(dev):
    """Rows of zeros take the bias path: with one hidden layer the pre-activation of such a row is the bias exactly (zero planes, scale 1),
    so a ReLU layer returns relu(bias) bit for bit; with more layers every zero row gives the bits of a batch that is all zeros (a row's
    result depends on that row and the parameters alone)."""
    obs, a = inputs(128, 13, 3, 3, dev)
    obs[5], a[5], obs[77], a[77] = 0.0, 0.0, 0.0, 0.0
    with torch.no_grad():
        one = make_q(2, 13, 3, (128,), nn.ReLU, 5, dev)
        hs = split16_hidden(prefixes(one), (obs, a))
        for q, h in zip(one, hs):
            want = torch.relu(q.q[0].bias)
            assert torch.equal(h[5], want) and torch.equal(h[77], want)
        deep = make_q(2, 13, 3, (128, 128), nn.ELU, 6, dev)
        hs = [h.clone() for h in split16_hidden(prefixes(deep), (obs, a))]
        zs = split16_hidden(prefixes(deep), (torch.zeros_like(obs), torch.zeros_like(a)))
        for h, z in zip(hs, zs):
            assert bool(torch.isfinite(h).all()) and torch.equal(h[5], z[0]) and torch.equal(h[77], z[0]) and torch.equal(z[0], z[100])


def does_not_qualify(dev):
    """split16_hidden declines, before any launch, what the kernel does not take."""
    with torch.no_grad():
        qs = make_q(2, 13, 3, (128, 128), nn.ELU, 1, dev)
        ok = inputs(128, 13, 3, 1, dev)
        assert split16_hidden(prefixes(qs), ok) is not None
        assert split16_hidden(prefixes(qs), inputs(100, 13, 3, 1, dev)) is None                                    # M % 128
        assert split16_hidden(prefixes(make_q(1, 13, 3, (192, 128), nn.ELU, 1, dev)), ok) is None                  # a hidden width % 128
        assert split16_hidden(prefixes(qs), (ok[0].double(), ok[1].double())) is None
        assert split16_hidden(prefixes(qs), (ok[0], ok[1][:, :2])) is None                                         # widths do not add up
        assert split16_hidden([prefixes(qs)[0], prefixes(make_q(1, 13, 3, (128, 256), nn.ELU, 1, dev))[0]], ok) is None
        assert split16_hidden(prefixes(make_q(1, 13, 3, (128, 128), nn.Sigmoid, 1, dev)), ok) is None
    assert split16_hidden(prefixes(qs), ok) is None                                                               # parameters want a gradient
    for q in qs:
        q.requires_grad_(False)
    assert split16_hidden(prefixes(qs), ok) is not None


def polyak_(targ, online):
    with torch.no_grad():
        for pt, po in zip(targ.parameters(), online.parameters()):
            pt.data.mul_(0.995).add_(0.005 * po.data)


def adam_step_(module, seed):
    """One Adam step with seeded gradients on every parameter (in place, as the off-policy trainers' optimizers do)."""
    g = torch.Generator().manual_seed(seed)
    params = list(module.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)
    for q in params:
        q.grad = torch.randn(q.shape, generator=g).to(q.device)
    opt.step()
    for q in params:
        q.grad = None


def scratch_dicts(module):
    return [m._split16_scratch for m in module.modules() if hasattr(m, "_split16_scratch")]


def follows_updates(make, call):
    """make(): a freshly constructed module; call(module): a list of result tensors.  An online module and its deepcopy, called,
    updated in place (Adam / polyak), called again: every result equals, bit for bit, a fresh module's with the same state_dict."""
    def fresh_result(m):
        f = make()
        f.load_state_dict(m.state_dict())
        return call(f)

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))

    online = make()
    first = [t.clone() for t in call(online)]
    assert any(scratch_dicts(online)), "the f16x2 path did not run"
    targ = copy.deepcopy(online)
    assert scratch_dicts(targ) and not any(scratch_dicts(targ)), "a deepcopy starts with empty scratch"
    assert list(targ.state_dict().keys()) == list(online.state_dict().keys())
    t0 = [t.clone() for t in call(targ)]
    assert same(t0, first) and same(t0, fresh_result(targ))
    for step in range(2):
        adam_step_(online, 40 + step)
        assert same(call(targ), t0), "updating the original changed the copy's output"
        o1 = [t.clone() for t in call(online)]
        assert not same(o1, first)
        assert same(o1, fresh_result(online))
        polyak_(targ, online)
        t1 = [t.clone() for t in call(targ)]
        assert not same(t1, t0)
        assert same(t1, fresh_result(targ))
        t0, first = t1, o1


def sac_heads(actor, hidden, deterministic, counters):
    """mms_sac_heads_act on `hidden` with the actor's head parameters, seed and row offset: (action [N, A], logp [N])."""
    L, idx, stream = _lib.for_device(hidden.device)
    N, A = hidden.shape[0], actor.mu_layer.out_features
    act, logp = torch.empty(N, A, device=hidden.device), torch.empty(N, device=hidden.device)
    _lib.check(L.mms_sac_heads_act(idx, p(hidden), hidden.shape[1], p(actor.mu_layer.weight.detach()), p(actor.mu_layer.bias.detach()),
                                   p(actor.log_std_layer.weight.detach()), p(actor.log_std_layer.bias.detach()), float(actor.act_limit), 1e-6,
                                   int(bool(deterministic)), actor.seed, p(counters), actor.row_offset, p(act), None, p(logp), None, None, None, N, A, stream),
               None, "mms_sac_heads_act", L)
    return act, logp

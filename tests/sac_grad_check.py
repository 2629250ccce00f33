"""Checks of mms_sac_heads_grad (include/mms.h) and of the actor's `fused_grad=True` path (algorithms/rl/sac/module.py) shared by the
CPU-build tests (test_sac_grad.py) and the GPU tests (test_sac_grad_gpu.py).  A "build" below is the tuple _lib.for_device gives --
(library, device argument, stream argument) -- plus the torch device the tensors live on.

Gates.  Per element the yardstick is the header's formula in float64 evaluated from the call's own fp32 u, mu and log_std (u - mu is
then exact on both sides); torch's fp32 autograd chain is NOT the yardstick: near |tanh u| = 1 it is off by up to 20 of these gates.
The gate is the first-order propagation of dt = 8 * 2^-24, sac_check's constant for the device tanh, plus 16 ulp of each term:
with t = tanh u, s = 1 - t^2, r = 2 t s / (s + eps), r' = 2 s / (s + eps) - 4 t^2 eps / (s + eps)^2,
    gate_mu = 16 ulp (|L s g_a| + |g_l r|) + (2 |t| |L g_a| + |g_l| |r'|) dt
    gate_ls = inside (gate_mu |u - mu| + 4 ulp (|G (u - mu)| + |g_l|)),          masked elements exactly 0.
dbias is one rounding of a double sum of the call's own dy: |dbias_c - sum64| <= 2^-24 |sum| + N 2^-52 sum_i |dy_ic|.
Module level: per gradient tensor, the relative Frobenius error against float64 autograd of torch_forward(eps=z) is at most twice
that of fp32 torch_forward(eps=z) + autograd on the same inputs (both are fp32 evaluations whose head GEMMs sum in different orders:
errors of one order, not equal)."""
import copy
import ctypes
import json
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":                   # run as a script (it writes profiles/sac_head_grad_error.json): the package is one level up
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import sac_check as sc
from massive_marl_benchmark_amd import _lib, spaces
from massive_marl_benchmark_amd.algorithms.rl.sac import MLPActorCritic

ULP1 = sc.ULP1
DT = 8 * ULP1
ENTRY_SHAPES = [(200, 128, 24, 1.0, False), (100, 64, 128, 2.5, False), (37, 192, 3, 1.0, False), (64, 128, 17, 1.0, True), (1, 64, 1, 1.0, False)]
LARGE = (70001, 64, 6, 1.0, False)           # 417 tiles of 168 rows (sac_grad_lane.h): many workgroups, an odd N * A, a partial last tile
WRAP = (9601, 64, 127, 1.0, False)           # 8-row tiles, 1201 of them: more than the largest grid (1024), so the grid-stride loop
                                             # wraps; an odd A and an odd N * A, one row in the last tile
PAD = 64                                     # canary floats behind dy and dbias


def build(device):
    """(L, device argument, stream argument, torch device)"""
    return _lib.for_device(device) + (torch.device(device),)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def aligned(nbytes, dev, align=256, offset=0):
    """(keep-alive tensor, address): `nbytes` behind an address that is `offset` past a multiple of `align`"""
    buf = torch.empty(int(nbytes) + 2 * align, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + (-buf.data_ptr()) % align + offset


def ws_bytes(b, N, A):
    L, idx, stream, dev = b
    n = ctypes.c_int64(-1)
    _lib.check(L.mms_sac_heads_grad(idx, N, A, 1.0, 1e-6, None, None, None, None, None, None, None, None, ctypes.byref(n), stream), None,
               "mms_sac_heads_grad size query", L)
    return n.value


def raw_call(b, N, A, limit, eps, u, mu, ls, ga, gl, dy, dbias, ws, nbytes):
    L, idx, stream, dev = b
    n = ctypes.c_int64(nbytes)
    return L.mms_sac_heads_grad(idx, N, A, float(limit), float(eps), _p(u), _p(mu), _p(ls), _p(ga), _p(gl), _p(dy), _p(dbias),
                                None if ws is None else ctypes.c_void_p(ws), ctypes.byref(n), stream)


def grad(b, u, mu, ls, ga, gl, limit=1.0, eps=1e-6, want_bias=True):
    """One call with canaries behind both destinations; returns (dy [N,2A], dbias [2A] or None)."""
    L, idx, stream, dev = b
    N, A = u.shape
    dy = torch.full((N * 2 * A + PAD,), 7.0, device=dev)
    db = torch.full((2 * A + PAD,), 7.0, device=dev) if want_bias else None
    need = ws_bytes(b, N, A)
    keep, ws = aligned(need, dev)
    _lib.check(raw_call(b, N, A, limit, eps, u, mu, ls, ga, gl, dy, db, ws, need), None, "mms_sac_heads_grad", L)
    assert (dy[N * 2 * A:] == 7.0).all() and (db is None or (db[2 * A:] == 7.0).all()), "canary"
    return dy[:N * 2 * A].view(N, 2 * A), (None if db is None else db[:2 * A])


def f64_formula(u, mu, ls, ga, gl, limit, eps):
    """(dmu, dls, gate_mu, gate_ls, inside) in float64 from the fp32 operands; ga / gl None = 0"""
    n = lambda t: np.asarray(t.detach().cpu(), np.float64)
    u, mu, ls = n(u), n(mu), n(ls)
    ga = np.zeros_like(u) if ga is None else n(ga)
    gl = np.zeros(u.shape[0]) if gl is None else n(gl)
    gl = gl[:, None]
    t = np.tanh(u)
    s = 1.0 - t * t
    r = 2.0 * t * s / (s + eps)
    rp = 2.0 * s / (s + eps) - 4.0 * t * t * eps / (s + eps) ** 2
    G = limit * s * ga + gl * r
    inside = (ls > -20.0) & (ls < 2.0)
    d = u - mu
    dls = inside * (G * d - gl)
    gate_mu = 16 * ULP1 * (np.abs(limit * s * ga) + np.abs(gl * r)) + (2 * np.abs(t) * np.abs(limit * ga) + np.abs(gl) * np.abs(rp)) * DT
    gate_ls = inside * (gate_mu * np.abs(d) + 4 * ULP1 * (np.abs(G * d) + np.abs(gl)))
    return G, dls, gate_mu, gate_ls, inside


def check_against_formula(dy, u, mu, ls, ga, gl, limit, eps, what=""):
    """dy against the float64 formula; returns the worst error over its gate (dmu, dls)"""
    A = u.shape[1]
    G, dls, gate_mu, gate_ls, inside = f64_formula(u, mu, ls, ga, gl, limit, eps)
    got = np.asarray(dy.detach().cpu(), np.float64)
    e_mu, e_ls = np.abs(got[:, :A] - G), np.abs(got[:, A:] - dls)
    assert (got[:, A:][~inside] == 0.0).all(), what
    assert (e_mu <= gate_mu).all(), (what, "dmu", float((e_mu / np.maximum(gate_mu, 1e-300)).max()))
    assert (e_ls <= gate_ls).all(), (what, "dls", float((e_ls[inside] / np.maximum(gate_ls[inside], 1e-300)).max()))
    return float((e_mu / np.maximum(gate_mu, 1e-300)).max()), float((e_ls / np.maximum(gate_ls, 1e-300)).max())


def check_bias(dbias, dy, what=""):
    d = np.asarray(dy.detach().cpu(), np.float64)
    s, sa = d.sum(0), np.abs(d).sum(0)
    e = np.abs(np.asarray(dbias.detach().cpu(), np.float64) - s)
    assert (e <= ULP1 * np.abs(s) + d.shape[0] * 2.0 ** -52 * sa).all(), (what, float(e.max()))


_forwards = {}


def forward(b, N, H, A, limit, det):
    """A mms_sac_heads_act call of this build on sac_check.problem(scaled=True) with every slot kept, and random incoming gradients;
    computed once per (build, shape) and shared (read-only) by the tests."""
    L, idx, stream, dev = b
    key = (str(dev), N, H, A, limit, det)
    if key not in _forwards:
        h, mw, mb, lw, lb = (t.to(dev) for t in sc.problem(N, H, A, seed=N + A))
        counters = (torch.arange(N, dtype=torch.int64) % 5).to(dev)
        out = sc.run(L, idx, stream, h, mw, mb, lw, lb, act_limit=limit, deterministic=det, seed=77, counters=counters, row_offset=3)
        g = torch.Generator().manual_seed(1000 + N)
        out["ga"], out["gl"] = torch.randn(N, A, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
        _forwards[key] = out
    return _forwards[key]


def check_entry(b, N, H, A, limit, det):
    """The entry against float64 per element, and its bias sums, on one shape; returns (dy, dbias)."""
    o = forward(b, N, H, A, limit, det)
    u, mu, ls = o["u"], o["mu"], o["log_std"]
    if N >= 37:                                     # both clamp bounds and saturated tanh are part of the check
        assert (ls == -20.0).any() and (ls == 2.0).any() and (u.abs().max(-1).values >= 3).any()
        assert ((ls > -20.0) & (ls < 2.0)).any()
    if det:
        assert torch.equal(u, mu)
    dy, db = grad(b, u, mu, ls, o["ga"], o["gl"], limit)
    check_against_formula(dy, u, mu, ls, o["ga"], o["gl"], limit, 1e-6, "both")
    check_bias(db, dy)
    return dy, db


def check_structure(b):
    """Row independence, determinism, each gradient alone, the scalar path, the grid-stride wrap, N == 0."""
    L, idx, stream, dev = b
    N, H, A, limit, det = LARGE
    o = forward(b, N, H, A, limit, det)
    u, mu, ls, ga, gl = o["u"], o["mu"], o["log_std"], o["ga"], o["gl"]
    dy, db = check_entry(b, N, H, A, limit, det)
    part, _ = grad(b, u[:64].clone(), mu[:64].clone(), ls[:64].clone(), ga[:64].clone(), gl[:64].clone(), limit)
    assert torch.equal(part, dy[:64])                              # a row depends on that row and the scalars alone
    dy2, db2 = grad(b, u, mu, ls, ga, gl, limit)
    assert torch.equal(dy2, dy) and torch.equal(db2, db)           # bit-identical run to run, the sums included
    dy_nb, none = grad(b, u, mu, ls, ga, gl, limit, want_bias=False)
    assert none is None and torch.equal(dy_nb, dy)
    # each incoming gradient alone = the formula with the other at 0
    n = 5000
    for a_, l_, what in ((ga[:n].clone(), None, "grad_action only"), (None, gl[:n].clone(), "grad_logp only")):
        d, bsum = grad(b, u[:n].clone(), mu[:n].clone(), ls[:n].clone(), a_, l_, limit)
        check_against_formula(d, u[:n], mu[:n], ls[:n], a_, l_, limit, 1e-6, what)
        check_bias(bsum, d, what)
    # operands 4 bytes off a 16-byte boundary (the element-by-element path): the same bits, dbias included
    off = lambda t: torch.cat([torch.zeros(1, device=dev), t.reshape(-1)])[1:].view(t.shape)
    uo, muo, lso, gao = off(u), off(mu), off(ls), off(ga)
    assert uo.data_ptr() % 16 == 4
    dy3, db3 = grad(b, uo, muo, lso, gao, gl, limit)
    assert torch.equal(dy3, dy) and torch.equal(db3, db)
    check_entry(b, *WRAP)
    # N == 0: success, nothing written, also without pointers
    dst, dbz = torch.full((8,), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    keep, ws = aligned(256, dev)
    assert raw_call(b, 0, 4, 1.0, 1e-6, None, None, None, None, None, dst, dbz, ws, 256) == 0
    assert (dst == 7.0).all() and (dbz == 7.0).all()
    assert ws_bytes(b, 0, 4) == 0


def check_abi_errors(b):
    L, idx, stream, dev = b
    N, H, A = 300, 64, 4
    o = forward(b, N, H, A, 1.0, False)
    dy, db = torch.full((N, 2 * A), 7.0, device=dev), torch.full((2 * A,), 7.0, device=dev)
    need = ws_bytes(b, N, A)
    keep, ws = aligned(need + 256, dev)
    base = dict(N=N, A=A, u=o["u"], mu=o["mu"], ls=o["log_std"], ga=o["ga"], gl=o["gl"], dy=dy, ws=ws, nbytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return raw_call(b, a["N"], a["A"], 1.0, 1e-6, a["u"], a["mu"], a["ls"], a["ga"], a["gl"], a["dy"], db, a["ws"], a["nbytes"])

    bad = [dict(ga=None, gl=None), dict(A=0), dict(A=129), dict(N=-1), dict(u=None), dict(mu=None), dict(ls=None), dict(dy=None), dict(ws=ws + 16)]
    if need > 0:
        bad.append(dict(nbytes=need - 1))
    for kw in bad:
        assert call(**kw) != 0 and _lib.last_error(None, L), kw
        assert "mms_sac_heads_grad" in _lib.last_error(None, L), kw
        if stream is not None:
            torch.cuda.synchronize()
        assert (dy == 7.0).all() and (db == 7.0).all(), kw
    assert "aligned" in (call(ws=ws + 16), _lib.last_error(None, L))[1]
    assert "both NULL" in (call(ga=None, gl=None), _lib.last_error(None, L))[1]
    n = ctypes.c_int64(0)
    assert L.mms_sac_heads_grad(idx, N, A, 1.0, 1e-6, None, None, None, None, None, None, None, None, None, stream) != 0     # no ws_bytes
    assert L.mms_sac_heads_grad(-1 if idx >= 0 else 0, N, A, 1.0, 1e-6, None, None, None, None, None, None, None, None, ctypes.byref(n), stream) != 0
    assert call() == 0 and not (dy == 7.0).any() and not (db == 7.0).any()


# ---- the module ---------------------------------------------------------------------------------------------------------------------

def make_ac(W, A, hidden, limit=1.0, **kw):
    return MLPActorCritic(spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-limit * np.ones(A), limit * np.ones(A)),
                          hidden_sizes=hidden, **kw)


def problem_actor(dev, N=300, H=128, A=6, limit=1.0, seed=11):
    """An actor (`net` = Linear(H, H) + ELU) with sac_check.problem(scaled=False)'s head parameters, and its hidden rows as the input."""
    h, mw, mb, lw, lb = sc.problem(N, H, A, seed=seed, scaled=False)
    torch.manual_seed(seed)
    pi = make_ac(H, A, (H,), limit=limit, seed=5, fused_grad=True).pi
    with torch.no_grad():
        for p, v in ((pi.mu_layer.weight, mw), (pi.mu_layer.bias, mb), (pi.log_std_layer.weight, lw), (pi.log_std_layer.bias, lb)):
            p.copy_(v)
    return pi.to(dev), h.to(dev)


def _grads(pi, x, forward, loss_of):
    x = x.clone().requires_grad_(True)
    pi.zero_grad(set_to_none=True)
    a, logp = forward(x)
    loss_of(a, logp).backward()
    out = {"input": x.grad.clone()}
    out.update({k: p.grad.clone() for k, p in pi.named_parameters()})
    return out


def module_gradient_ratios(b, N=300, H=128, A=6):
    """{loss variant: {tensor: error of fused_grad=True over error of fp32 torch_forward(eps=z), both against float64}} -- and the
    asserts that every ratio is at most 2 and that the counters advanced by exactly one."""
    L, idx, stream, dev = b
    pi, x = problem_actor(dev, N, H, A)
    pi64 = copy.deepcopy(pi).double()
    g = torch.Generator().manual_seed(3)
    c_a, c_l = torch.randn(N, A, generator=g).to(dev), torch.randn(N, 1, generator=g).to(dev)
    losses = {"weighted sum and mean": lambda a, logp: (c_a.to(a.dtype) * a).sum() + (c_l.to(a.dtype) * logp).mean(),
              "sum and [N,1] mean": lambda a, logp: a.sum() - logp.mean()}             # (both gradients arrive stride-0 expanded)
    ratios = {}
    for name, loss_of in losses.items():
        c0 = pi.counters(N, dev).clone()
        z = sc.draws(L, idx, stream, pi.seed, c0, pi.row_offset, N, A)
        fused = _grads(pi, x, lambda t: pi(t), loss_of)
        assert torch.equal(pi._counters[:N], c0 + 1), name
        plain = _grads(pi, x, lambda t: pi.torch_forward(t, eps=z), loss_of)
        ref = _grads(pi64, x.double(), lambda t: pi64.torch_forward(t, eps=z.double()), loss_of)
        ratios[name] = {}
        for k, r in ref.items():
            err = lambda t: float((t.double() - r).norm() / r.norm())
            e_f, e_t = err(fused[k]), err(plain[k])
            ratios[name][k] = {"fused": e_f, "torch_fp32": e_t, "ratio": e_f / e_t}
            print("%-22s %-24s fused %.3e torch %.3e ratio %.3f" % (name, k, e_f, e_t, e_f / e_t))
        for k, v in ratios[name].items():
            assert v["fused"] <= 2 * v["torch_fp32"], (name, k, v)
    return ratios


def check_module_semantics(b):
    L, idx, stream, dev = b
    N, H, A = 50, 64, 5
    pi, x = problem_actor(dev, N, H, A)
    x = x.clone().requires_grad_(True)
    c0 = pi.counters(N, dev).clone()
    a, logp = pi(x)
    assert a.shape == (N, A) and logp.shape == (N, 1) and a.requires_grad and logp.requires_grad
    assert torch.equal(pi._counters[:N], c0 + 1)
    a, logp = pi(x, deterministic=True)
    assert torch.equal(pi._counters[:N], c0 + 1) and a.requires_grad        # deterministic: nothing drawn
    with torch.no_grad():
        assert (a - pi.act_limit * torch.tanh(pi.mu_layer(pi.net(x)))).abs().max() <= 2e-5
    a3, l3 = pi(x.view(5, 10, H))                                           # leading dimensions are kept
    assert a3.shape == (5, 10, A) and l3.shape == (5, 10, 1)
    # with_logprob=False: no logp, a differentiable action
    a, none = pi(x, with_logprob=False)
    assert none is None and a.requires_grad
    pi.zero_grad(set_to_none=True)
    a.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in pi.parameters()) and torch.isfinite(x.grad).all()
    # only what needs a gradient gets one
    pi.zero_grad(set_to_none=True)
    pi.mu_layer.requires_grad_(False)
    pi(x)[1].sum().backward()
    assert pi.mu_layer.weight.grad is None and pi.mu_layer.bias.grad is None and pi.log_std_layer.weight.grad is not None
    pi.mu_layer.requires_grad_(True)
    # a double backward raises
    a, logp = pi(x)
    try:
        (gx,) = torch.autograd.grad(logp.sum(), x, create_graph=True)
        gx.sum().backward()
        raised = False
    except RuntimeError:
        raised = True
    assert raised
    # state_dict keys are the reference's, deepcopy keeps the flag
    ac = make_ac(12, 4, (64, 64), fused_grad=True)
    assert list(ac.state_dict().keys()) == list(make_ac(12, 4, (64, 64)).state_dict().keys())
    assert ac.pi.fused_grad and copy.deepcopy(ac).pi.fused_grad and not make_ac(12, 4, (64, 64)).pi.fused_grad


def check_fallback(dev):
    """A head that does not qualify (H = 96) with fused_grad=True: bit for bit what fused_grad=False gives under the same torch seed."""
    outs = []
    for flag in (True, False):
        torch.manual_seed(21)
        pi = make_ac(10, 3, (64, 96), fused_grad=flag).pi.to(dev)
        x = torch.randn(40, 10).to(dev).requires_grad_(True)
        torch.manual_seed(22)
        a, logp = pi(x)
        (a.sum() + logp.mean()).backward()
        outs.append([a.detach(), logp.detach(), x.grad] + [p.grad for p in pi.parameters()])
        assert pi._counters is None                                           # the counter stream was not touched
    assert all(torch.equal(p, q) for p, q in zip(*outs))


def check_policy_loss(dev):
    """sac.py:336-348 restated: the Q parameters frozen, loss_pi.backward(), unfrozen."""
    torch.manual_seed(5)
    ac = make_ac(20, 4, (64, 64), fused_grad=True).to(dev)
    o = torch.randn(64, 20).to(dev)
    q_params = list(ac.q1.parameters()) + list(ac.q2.parameters())
    for p in q_params:
        p.requires_grad = False
    pi, logp_pi = ac.pi(o)
    q_pi = torch.min(ac.q1(o, pi), ac.q2(o, pi))
    loss_pi = (0.2 * logp_pi - q_pi).mean()
    loss_pi.backward()
    for p in q_params:
        p.requires_grad = True
    assert all(p.grad is None for p in q_params)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0 for p in ac.pi.parameters())
    assert torch.equal(ac.pi._counters[:64], torch.ones(64, dtype=torch.int64, device=ac.pi._counters.device))


if __name__ == "__main__":
    # the measured ratios of the module gate, as profiles/sac_head_grad_error.json records them
    result = {"cpu": module_gradient_ratios(build("cpu"))}
    if torch.cuda.is_available():
        result["cuda"] = module_gradient_ratios(build("cuda:0"))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "sac_head_grad_error.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")

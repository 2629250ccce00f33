"""Checks of mms_ppo_loss (include/mms.h, csrc/ppo_loss_kernels.hip, csrc/cpu/mms_cpu.cpp) through the C ABI, shared by the CPU-build
tests (test_ppo_loss.py) and the GPU tests (test_ppo_loss_gpu.py): seeded problems with the clip regimes forced, the float64 yardstick,
the call through ctypes with guarded outputs and an exactly sized workspace, the gates, the exact properties and the error paths.

The yardstick is this file's own statement of the loss (`expression`): the formulas of include/mms.h in torch ops, differentiated by
torch autograd -- in float64 it is the truth, in float32 on the same inputs it is what the torch chain of ppo.py:270-302 gives.  Its logp
and entropy are pinned to the reference by the `evaluate` outputs of tests/golden/ppo_act.npz (test_ppo_loss.py).

Gates, per output (dmu, dlog_std, dvalue and the five scalars), e = rms(out - truth), et = rms(torch fp32 - truth):
    e <= 1.25 et                         the project's factor for reduced outputs (mlp_grad_check.py gate (c))
    e <= 2 et + 1e-6 scale               instead, where et <= 2^-22 scale: torch's own error is then at rounding level (two ulps of
                                         the tensor's scale) and can be 0 by accident, above all on a scalar (q_check.py's form);
scale = the same reduction in float64 over the absolute values of its terms (for dmu and dvalue: rms of the truth).
What the second form was needed for on the MI355X (profiles/ppo_loss_error.json): never for dmu (0.53 - 1.18 et) or dvalue (1.00 et);
for the sums where torch's error happened to be smallest -- surrogate 4.5 et, kl 4.2 et, loss 3.3 et, entropy 1.9 et, dlog_std 1.28 et
at (7, 8) -- with errors of at most 1.8e-7 of the scale, three ulps, against the 1e-6 allowed.
The clip selection is discontinuous: rows whose float64 ratio lies within a relative 1e-3 of 1 +- clip are left out of the dmu
comparison, rows whose float64 |v - tv| lies within 1e-4 of clip out of the dvalue comparison, at most 2 % of the rows of a problem
together; on every other row the set of rows with a zero gradient must EQUAL the yardstick's.  dlog_std and the scalars are sums over
all rows: they are compared on problems without a row in either band (`problem` draws such rows again; clean=False keeps them)."""
import ctypes
import math

import torch

from massive_marl_benchmark_amd import _lib

GUARD = 64               # floats of NaN on each side of every output
WS_PAD = 512             # bytes of fill around the workspace slice (the slice starts at a 256-aligned address inside)
CLIP = 0.2
R_BAND, V_BAND, BAND_CAP = 1e-3, 1e-4, 0.02
FACTOR, ROUNDING, FLOOR = 1.25, 2.0 ** -22, 1e-6
SCALARS = ("loss", "surrogate", "value_loss", "entropy", "kl")
FIELDS = ("actions", "old_logp", "adv", "returns", "target_values", "old_mu", "old_sigma")
MAX_A = 128              # include/mms.h: MMS_PPO_LOSS_MAX_A
# (adv, ratio) of the forced surrogate rows, then (v - tv, ret - v) of the forced value rows
FORCED_R = ((1.0, 1.5), (1.0, 0.5), (-1.0, 1.5), (-1.0, 0.5), (0.0, 1.1), (0.7, 1.0))
FORCED_V = ((0.1, 0.4), (0.5, 1.0), (0.5, -1.0), (-0.5, 1.0), (-0.5, -1.0))


def logp64(mu, log_std, actions):
    mu, l, a = mu.double(), log_std.double(), actions.double()
    z = (a - mu) * torch.exp(-2.0 * l)
    return (-0.5 * z * z - 2.0 * l - 0.5 * math.log(2.0 * math.pi)).sum(-1)


def _draw(M, A, seed, clean):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    l = 0.2 * rn(A) - 0.3
    mu, v = rn(M, A), rn(M)
    actions = mu + torch.exp(2.0 * l) * rn(M, A)
    old_mu = mu + 0.1 * rn(M, A)
    old_sigma = l + 0.05 * rn(M, A)
    adv, tv, ret = rn(M), v + 0.3 * rn(M), v + rn(M)
    lp = logp64(mu, l, actions)
    old_logp = lp + 0.3 * rn(M).double()
    # the forced regimes over the last rows (as many as fit beside one free row): adv > 0 and adv < 0 with r above and below the clip
    # range, adv = 0, r = 1 (to the rounding of old_logp); |v - tv| below clip, and above it on each side with ret on each side of v
    nf = min(len(FORCED_R) + len(FORCED_V), M - 1)
    for k in range(nf):
        row = M - nf + k
        if k < len(FORCED_R):
            adv[row] = FORCED_R[k][0]
            old_logp[row] = lp[row] - math.log(FORCED_R[k][1])
        else:
            d, e = FORCED_V[k - len(FORCED_R)]
            tv[row], ret[row] = v[row] - d, v[row] + e
    pr = dict(M=M, A=A, mu=mu, log_std=l, value=v, actions=actions, old_logp=old_logp.float(), adv=adv, returns=ret, target_values=tv,
              old_mu=old_mu, old_sigma=old_sigma, redraws=0)
    while clean:                                                     # rows in a band draw their old_logp / tv again (never a forced row)
        in_r, in_v = bands(pr)
        if not bool((in_r | in_v).any()):
            break
        pr["redraws"] += int((in_r | in_v).sum())
        assert pr["redraws"] < 64 + M // 8, "rows keep landing in the bands"
        pr["old_logp"][in_r] = (lp[in_r] + 0.3 * rn(int(in_r.sum())).double()).float()
        tv[in_v] = v[in_v] + 0.3 * rn(int(in_v.sum()))
    return pr


def bands(pr):
    """(rows left out of the dmu comparison, rows left out of the dvalue comparison), from the float64 ratio and v - tv."""
    r = torch.exp(logp64(pr["mu"], pr["log_std"], pr["actions"]) - pr["old_logp"].double()).cpu()
    d = (pr["value"].double() - pr["target_values"].double()).abs().cpu()
    in_r = ((r / (1.0 - CLIP) - 1.0).abs() <= R_BAND) | ((r / (1.0 + CLIP) - 1.0).abs() <= R_BAND)
    in_v = (d - CLIP).abs() <= V_BAND
    return in_r, in_v


def problem(M, A, seed=0, device="cpu", clean=True):
    """A well posed problem of M rows (module docstring; ratios span about 0.35 - 2.9 and a quarter of the rows have a zero surrogate
    gradient).  clean: a row that lands in a band draws again (a 1e-3 band holds about one row in 200), so that the sums compare too;
    pr["redraws"] counts them."""
    pr = _draw(M, A, 7919 * seed + 31 * A + M, clean)
    return {k: (t.contiguous().to(device) if torch.is_tensor(t) else t) for k, t in pr.items()}


def expression(pr, dtype, clipped_value, value_coef, entropy_coef, clip=CLIP):
    """Every output by name from torch autograd of the loss in `dtype`, with the float64 scales ("scale:<name>") when dtype is float64."""
    c = lambda k: pr[k].detach().to(dtype)
    mu, l, v = (c(k).requires_grad_(True) for k in ("mu", "log_std", "value"))
    a, olp, adv, ret, tv, om, os = (c(k) for k in FIELDS)
    einv = torch.exp(-2.0 * l)
    z = (a - mu) * einv
    t_lp = -0.5 * z * z - 2.0 * l - 0.5 * math.log(2.0 * math.pi)
    logp = t_lp.sum(-1)
    t_ent = 0.5 + 0.5 * math.log(2.0 * math.pi) + 2.0 * l
    entropy = t_ent.sum()
    with torch.no_grad():
        quot = (torch.square(os.exp()) + torch.square(om - mu)) / (2.0 * torch.square(l.exp()))
        kl = torch.sum(l - os + quot - 0.5, dim=-1).mean()
    r = torch.exp(logp - olp)
    s_i = torch.max(-adv * r, -adv * torch.clamp(r, 1.0 - clip, 1.0 + clip))
    surrogate = s_i.mean()
    if clipped_value:
        vc = tv + (v - tv).clamp(-clip, clip)
        value_loss = torch.max((v - ret).pow(2), (vc - ret).pow(2)).mean()
    else:
        value_loss = (ret - v).pow(2).mean()
    loss = surrogate + value_coef * value_loss - entropy_coef * entropy
    dmu, dl, dv = torch.autograd.grad(loss, (mu, l, v))
    out = {"dmu": dmu, "dlog_std": dl, "dvalue": dv, "loss": loss.detach(), "surrogate": surrogate.detach(), "value_loss": value_loss.detach(),
           "entropy": entropy.detach(), "kl": kl}
    if dtype == torch.float64:
        with torch.no_grad():
            M = mu.shape[0]
            # the reductions once more over the absolute values of their terms
            take = (dmu != 0).any(-1)                                              # rows whose surrogate gradient passes
            gi = torch.where(take, (adv * r).abs() / M, torch.zeros_like(r))
            sc = {"dmu": dmu.pow(2).mean().sqrt(), "dvalue": dv.pow(2).mean().sqrt(),
                  "dlog_std": ((gi[:, None] * (2.0 * z * z + 2.0)).sum(0) + 2.0 * abs(entropy_coef)).pow(2).mean().sqrt(),
                  "surrogate": s_i.abs().mean(), "value_loss": value_loss.detach(), "entropy": t_ent.abs().sum(),
                  "kl": ((l - os).abs() + quot + 0.5).sum(-1).mean()}
            sc["loss"] = sc["surrogate"] + abs(value_coef) * sc["value_loss"] + abs(entropy_coef) * sc["entropy"]
            out.update({"scale:" + k: t for k, t in sc.items()})
    return out


# ---- the call ------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Guarded:
    """A float32 output of `shape` inside a larger NaN-filled buffer, GUARD floats on each side."""

    def __init__(self, shape, device):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=device)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)

    def guards_nan(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[-GUARD:]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


class Workspace:
    """A slice of exactly `need` bytes at a 256-aligned address inside a larger uint8 buffer filled with `fill`."""

    def __init__(self, need, fill, device):
        self.n = int(need)
        self.fill = fill
        self.buf = torch.full((self.n + 2 * WS_PAD,), fill, dtype=torch.uint8, device=device)
        self.off = 256 + (-self.buf.data_ptr()) % 256
        assert 256 <= self.off < WS_PAD and (self.buf.data_ptr() + self.off) % 256 == 0

    def ptr(self, shift=0):
        return ctypes.c_void_p(self.buf.data_ptr() + self.off + shift)

    def outside_untouched(self):
        return bool((self.buf[:self.off] == self.fill).all()) and bool((self.buf[self.off + self.n:] == self.fill).all())


def raw(L, device, stream, pr, out, dmu, dls, dv, ws, nbytes, clipped_value=1, value_coef=1.0, entropy_coef=0.0, clip=CLIP, indices=None, **over):
    """The raw entry; `over` replaces arguments by name (M, A, or a tensor's name -> tensor or None); returns the return code."""
    a = dict(pr, **over)
    n = nbytes if isinstance(nbytes, ctypes.c_int64) else ctypes.c_int64(nbytes)
    return L.mms_ppo_loss(device, a["M"], a["A"], _p(a["mu"]), _p(a["log_std"]), _p(a["value"]), _p(indices), _p(a["actions"]),
                          _p(a["old_logp"]), _p(a["adv"]), _p(a["returns"]), _p(a["target_values"]), _p(a["old_mu"]), _p(a["old_sigma"]), clip,
                          value_coef, entropy_coef, clipped_value, _p(out), _p(dmu), _p(dls), _p(dv), ws, ctypes.byref(n), stream)


def query(L, device, stream, M, A):
    """(return code, bytes) of the size query: every pointer NULL."""
    n = ctypes.c_int64(-1)
    rc = L.mms_ppo_loss(device, M, A, *([None] * 11), CLIP, 1.0, 0.0, 1, None, None, None, None, None, ctypes.byref(n), stream)
    return rc, int(n.value)


def run(L, device, stream, pr, clipped_value=1, value_coef=1.0, entropy_coef=0.0, indices=None, grads=True, fill=0x00, dense=None):
    """One call on guarded outputs and an exactly sized workspace slice inside a buffer of `fill` bytes.  dense: the (mu, value) of an
    indexed call (then pr is the storage).  Returns {"out": name -> tensor, "guards", "ws_outside", "bytes"}."""
    dev = pr["mu"].device
    over = {}
    if dense is not None:
        over = {"mu": dense[0], "value": dense[1], "M": dense[0].shape[0]}
    M, A = over.get("M", pr["M"]), pr["A"]
    rc, need = query(L, device, stream, M, A)
    _lib.check(rc, None, "mms_ppo_loss size query", L)
    assert need % 256 == 0 and (need > 0) == (device >= 0), need
    o = {"out": Guarded((5,), dev), "dmu": Guarded((M, A), dev), "dlog_std": Guarded((A,), dev), "dvalue": Guarded((M,), dev)}
    ws = Workspace(need, fill, dev)
    g = lambda k: o[k].t if grads else None
    _lib.check(raw(L, device, stream, pr, o["out"].t, g("dmu"), g("dlog_std"), g("dvalue"), ws.ptr(), need, clipped_value, value_coef, entropy_coef,
                   indices=indices, **over), None, "mms_ppo_loss", L)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    res = {k: o["out"].t[i] for i, k in enumerate(SCALARS)}
    if grads:
        res.update({k: o[k].t for k in ("dmu", "dlog_std", "dvalue")})
    return {"out": res, "guards": all(x.guards_nan() for x in o.values()),
            "untouched": grads or all(o[k].all_nan() for k in ("dmu", "dlog_std", "dvalue")), "ws_outside": ws.outside_untouched(), "bytes": need}


# ---- the gates -----------------------------------------------------------------------------------------------------------------------
def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def gates(pr, got, clipped_value, value_coef, entropy_coef, stats=None, sums=True):
    """The failures of the gates of the module docstring; stats (a dict) receives, per output, e / et, e / scale and which gate applied.
    sums: compare dlog_std and the scalars too (the problem has no row in a band)."""
    t64 = {k: t.cpu() for k, t in expression(pr, torch.float64, clipped_value, value_coef, entropy_coef).items()}
    t32 = {k: t.cpu() for k, t in expression(pr, torch.float32, clipped_value, value_coef, entropy_coef).items()}
    got = {k: t.detach().cpu() for k, t in got.items()}
    in_r, in_v = bands(pr)
    fails = []
    M = pr["M"]
    if int(in_r.sum()) + int(in_v.sum()) > BAND_CAP * M:
        fails.append(("bands", "more than 2 %% of the rows left out", int(in_r.sum()), int(in_v.sum())))
    if sums and bool((in_r | in_v).any()):
        fails.append(("bands", "a sum is compared on a problem with rows in a band"))
    # selection: the rows with a zero gradient are the yardstick's, outside the bands
    for name, z_got, z_ref, keep in (("dmu", (got["dmu"] == 0).all(-1), (t64["dmu"] == 0).all(-1), ~in_r),
                                     ("dvalue", got["dvalue"] == 0, t64["dvalue"] == 0, ~in_v)):
        flips = int((z_got != z_ref)[keep].sum())
        if flips:
            fails.append((name, "selection flips", flips))
    rows = {"dmu": ~in_r, "dvalue": ~in_v}
    for name in ("dmu", "dvalue") + ((("dlog_std",) + SCALARS) if sums else ()):
        o, t, y = got[name].double(), t64[name], t32[name].double()
        if not bool(torch.isfinite(o).all()):
            fails.append((name, "not finite"))
            continue
        if name in rows:
            o, t, y = o[rows[name]], t[rows[name]], y[rows[name]]
        if t.numel() == 0:
            continue
        e, et, sc = _rms(o - t), _rms(y - t), float(t64["scale:" + name])
        rounding = et <= ROUNDING * sc
        allowed = 2.0 * et + FLOOR * sc if rounding else FACTOR * et
        print("  %-10s e %.3e  et %.3e  e/et %.3g  e/scale %.3g  %s" % (name, e, et, e / et if et else float("inf") if e else 0.0, e / sc if sc else 0.0,
                                                                        "floor" if rounding else "1.25"))
        if stats is not None:
            stats[name] = {"e_over_et": (e / et) if et else None, "e_over_scale": (e / sc) if sc else None, "gate": "floor" if rounding else "factor",
                           "floor_needed": bool(e > FACTOR * et)}
        if e > allowed:
            fails.append((name, "rms error", e, "torch fp32", et, "allowed", allowed))
    return fails


def check(L, device, stream, pr, clipped_value=1, value_coef=0.7, entropy_coef=0.01, stats=None):
    """One guarded call against the yardstick; returns its result."""
    res = run(L, device, stream, pr, clipped_value, value_coef, entropy_coef)
    assert res["guards"] and res["ws_outside"], "a write outside an output or outside the workspace slice"
    fails = gates(pr, res["out"], clipped_value, value_coef, entropy_coef, stats=stats)
    assert not fails, fails
    return res


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


# ---- exact properties ----------------------------------------------------------------------------------------------------------------
def exact_properties(L, device, stream, M=1000, A=80, seed=3):
    """The exact properties of the entry (module docstring of test_ppo_loss.py lists them)."""
    dev = "cpu" if device < 0 else "cuda:%d" % device
    pr = problem(M, A, seed, dev)
    kw = dict(clipped_value=1, value_coef=0.7, entropy_coef=0.01)
    first = run(L, device, stream, pr, fill=0x00, **kw)
    # run to run, and whatever the workspace held
    again = run(L, device, stream, pr, fill=0xFF, **kw)
    assert same(first["out"], again["out"]), "results depend on the run or on the workspace's content"
    assert first["guards"] and again["guards"] and first["ws_outside"] and again["ws_outside"]
    # indices = arange(M) over the same fields
    ar = torch.arange(M, dtype=torch.int64, device=dev)
    assert same(first["out"], run(L, device, stream, pr, indices=ar, **kw)["out"]), "indices = arange(M) differs from indices = NULL"
    # a permuted, repeating index vector over a larger storage against the dense call on the gathered copies
    g = torch.Generator().manual_seed(seed)
    m2 = M // 2 + 3
    idx = torch.randint(0, M, (m2,), generator=g).to(dev)
    idx[1] = idx[0]
    mu, v = pr["mu"][idx].contiguous(), pr["value"][idx].contiguous()
    gathered = dict(pr, M=m2, mu=mu, value=v, **{k: pr[k][idx].contiguous() for k in FIELDS})
    a = run(L, device, stream, pr, indices=idx, dense=(mu, v), **kw)
    b = run(L, device, stream, gathered, **kw)
    assert a["guards"] and b["guards"] and same(a["out"], b["out"]), "an indexed call differs from the dense call on the gathered rows"
    # rows with g_i = 0 have dmu rows of exact zeros (a quarter of the rows: the yardstick's set, checked by the gates)
    t64 = expression(pr, torch.float64, 1, 0.7, 0.01)
    zero = (t64["dmu"] == 0).all(-1)
    in_r, _ = bands(pr)
    assert int(zero.sum()) > M // 8 and bool((first["out"]["dmu"][zero.to(dev) & ~in_r.to(dev)] == 0).all())
    # the entropy is the closed form whatever M is
    ent = float((0.5 + 0.5 * math.log(2.0 * math.pi) + 2.0 * pr["log_std"].double()).sum())
    for rows in (1, 7, M):
        sub = dict(pr, M=rows, **{k: pr[k][:rows].contiguous() for k in ("mu", "value") + FIELDS})
        got = run(L, device, stream, sub, **kw)["out"]["entropy"]
        assert abs(float(got) - ent) <= 2.0 ** -23 * abs(ent) and torch.equal(got, first["out"]["entropy"]), (rows, float(got), ent)
    # the gradient pointers NULL: the same five scalars, nothing else written
    terms = run(L, device, stream, pr, grads=False, **kw)
    assert terms["untouched"] and terms["guards"] and all(torch.equal(terms["out"][k], first["out"][k]) for k in SCALARS)
    return first


# ---- error paths ---------------------------------------------------------------------------------------------------------------------
def check_error_paths(L, device, stream, other_device, messages=None):
    """Every refused call returns non-zero with a message and writes nothing (outputs stay NaN).  device: the library's own device
    argument; other_device: one it must refuse.  messages: receives (label, message), the same on both builds but for the wrong device
    and the byte counts."""
    dev = "cpu" if device < 0 else "cuda:%d" % device
    M, A = 40, 8
    pr = problem(M, A, 5, dev)
    rc, need = query(L, device, stream, M, A)
    assert rc == 0
    o = {"out": Guarded((5,), dev), "dmu": Guarded((M, A), dev), "dlog_std": Guarded((A,), dev), "dvalue": Guarded((M,), dev)}
    ws = Workspace(need, 0x5A, dev)

    def go(nbytes=need, shift=0, out="out", dmu="dmu", dls="dlog_std", dv="dvalue", **over):
        t = lambda k: None if k is None else o[k].t
        return raw(L, over.pop("device", device), stream, pr, t(out), t(dmu), t(dls), t(dv), ws.ptr(shift), nbytes, **over)

    bad = [("M = 0", dict(M=0), "M must be in"), ("M above 2^31 - 1", dict(M=2 ** 31), "M must be in"), ("A = 0", dict(A=0), "A must be in 1..%d" % MAX_A),
           ("A above the limit", dict(A=MAX_A + 1), "A must be in 1..%d" % MAX_A)]
    bad += [("NULL " + k, {k: None}, "null pointer") for k in ("mu", "log_std", "value") + FIELDS]
    bad += [("NULL out", dict(out=None), "null pointer"), ("dmu and dvalue without dlog_std", dict(dls=None), "go together"),
            ("dlog_std alone", dict(dmu=None, dv=None), "go together"), ("a short workspace", dict(nbytes=need - 1), "workspace too small"),
            ("a misaligned workspace", dict(shift=64), "256-byte aligned"), ("the wrong device", dict(device=other_device), None)]
    for label, kw, contains in bad:
        rc = go(**kw)
        msg = _lib.last_error(None, L)
        assert rc != 0 and msg, (label, rc, msg)
        assert contains is None or contains in msg, (label, msg)
        if messages is not None:
            messages.append((label, msg))
        if dev != "cpu":
            torch.cuda.synchronize()
        assert all(x.all_nan() for x in o.values()) and ws.outside_untouched() and bool((ws.buf == 0x5A).all()), label
    n = ctypes.c_int64(-1)                                           # the size query reads nothing else, and needs ws_bytes
    assert L.mms_ppo_loss(device, M, A, *([None] * 11), CLIP, 1.0, 0.0, 1, None, None, None, None, None, None, stream) != 0
    assert "ws_bytes" in _lib.last_error(None, L)
    assert go() == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert not any(bool(torch.isnan(x.t).any()) for x in o.values()) and all(x.guards_nan() for x in o.values()) and ws.outside_untouched()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
def tensor_gate(name, got, yard, truth):
    """The same gate for a tensor that autograd carried further (a parameter's gradient, a loss): e <= 1.25 et, or 2 et + 1e-6 rms(truth)
    where et is at rounding level.  Returns the failure or None."""
    e, et, sc = _rms(got.detach().cpu().double() - truth.cpu()), _rms(yard.detach().cpu().double() - truth.cpu()), _rms(truth.cpu())
    rounding = et <= ROUNDING * sc
    allowed = 2.0 * et + FLOOR * sc if rounding else FACTOR * et
    print("  %-24s e %.3e  et %.3e  scale %.3e  %s" % (name, e, et, sc, "floor" if rounding else "1.25"))
    return (name, "rms error", e, "torch fp32", et, "allowed", allowed) if e > allowed else None


def storage_problem(T, N, obs_dim, A, seed, device="cpu"):
    """An ActorCritic with small ELU networks and a RolloutStorage filled by a well posed problem (T x N rows in storage order):
    the module's own mu and value at the stored observations stand in for the problem's."""
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
    torch.manual_seed(seed)
    ac = ActorCritic((obs_dim,), (0,), (A,), 0.8, {"pi_hid_sizes": [32, 16], "vf_hid_sizes": [32, 16], "activation": "elu"}, seed=seed).to(device)
    st = RolloutStorage(N, T, (obs_dim,), (0,), (A,), device=device)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(device)
    st.observations.copy_(rn(T, N, obs_dim))
    with torch.no_grad():
        mu, v = ac.actor(st.observations.view(-1, obs_dim)), ac.critic(st.observations.view(-1, obs_dim)).view(-1)
        l = ac.log_std.detach()
        act = mu + torch.exp(2.0 * l) * rn(T * N, A)
        st.actions.copy_(act.view(T, N, A))
        st.mu.copy_((mu + 0.1 * rn(T * N, A)).view(T, N, A))
        st.sigma.copy_((l + 0.05 * rn(T * N, A)).view(T, N, A))
        st.actions_log_prob.copy_((logp64(mu, l, act) + 0.3 * rn(T * N).double()).float().view(T, N, 1))
        st.advantages.copy_(rn(T, N, 1))
        st.values.copy_((v + 0.3 * rn(T * N)).view(T, N, 1))
        st.returns.copy_((v + rn(T * N)).view(T, N, 1))
    return ac, st


def unfused_loss(ac, st, indices, clip, value_coef, entropy_coef, clipped_value, dtype=torch.float32):
    """PPO.update's chain (ppo.py:253-302) on minibatch `indices` through ActorCritic.evaluate, in `dtype` (float64: on a double copy of
    the module, whose parameters receive the gradients).  Returns (loss, kl, module)."""
    import copy
    m = ac if dtype == torch.float32 else copy.deepcopy(ac).double()
    flat = lambda t: t.view(-1, *t.shape[2:]).to(dtype)[indices]
    logp, entropy, value, mu, sigma = m.evaluate(flat(st.observations), None, flat(st.actions))
    old_mu, old_sigma = flat(st.mu), flat(st.sigma)
    with torch.no_grad():
        kl = torch.sum(sigma - old_sigma + (torch.square(old_sigma.exp()) + torch.square(old_mu - mu)) / (2.0 * torch.square(sigma.exp())) - 0.5, axis=-1).mean()
    ratio = torch.exp(logp - torch.squeeze(flat(st.actions_log_prob)))
    adv = torch.squeeze(flat(st.advantages))
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    tv, ret = flat(st.values), flat(st.returns)
    if clipped_value:
        vc = tv + (value - tv).clamp(-clip, clip)
        value_loss = torch.max((value - ret).pow(2), (vc - ret).pow(2)).mean()
    else:
        value_loss = (ret - value).pow(2).mean()
    return surrogate + value_coef * value_loss - entropy_coef * entropy.mean(), kl, m


def module_check(ac, st, indices, clipped_value=True, value_coef=0.7, entropy_coef=0.01):
    """ActorCritic.ppo_loss on minibatch `indices` against the unfused chain: loss, kl and every parameter's gradient inside the gate
    (float64 module as truth, the fp32 torch chain as yardstick).  Returns (loss, info, gradients)."""
    def grads(m, loss):
        for p in m.parameters():
            p.grad = None
        loss.backward()
        return [p.grad.clone() for p in m.parameters()]

    idx_t = torch.as_tensor(indices, dtype=torch.int64, device=ac.log_std.device)
    l64, kl64, m64 = unfused_loss(ac, st, idx_t, CLIP, value_coef, entropy_coef, clipped_value, torch.float64)
    g64 = grads(m64, l64)
    lt, klt, _ = unfused_loss(ac, st, idx_t, CLIP, value_coef, entropy_coef, clipped_value)
    gt = grads(ac, lt)
    obs = st.observations.view(-1, st.observations.shape[-1])[idx_t]
    lf, info = ac.ppo_loss(obs, None, st, indices, CLIP, value_coef, entropy_coef, clipped_value)
    assert lf.requires_grad and not any(t.requires_grad for t in info.values()) and sorted(info) == ["entropy", "kl", "surrogate", "value_loss"]
    gf = grads(ac, lf)
    names = ["loss", "kl"] + [n for n, _ in ac.named_parameters()]
    fails = [tensor_gate(n, f, t, x) for n, f, t, x in zip(names, [lf, info["kl"]] + gf, [lt, klt] + gt, [l64.detach(), kl64] + g64)]
    assert not any(fails), [f for f in fails if f]
    return lf.detach(), info, gf

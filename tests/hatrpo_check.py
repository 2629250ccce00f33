"""Test infrastructure for the HATRPO trainer and the two LayerNorm-MLP entries (mms_ln_mlp_grad, mms_ln_mlp_jvp): actors with
randomised parameters, the float64 autograd statements they are compared with -- J^T g and J v per tensor, the reference's
Fisher-vector product (hatrpo_trainer.py:170-179: the KL between the actor and itself, gradient with create_graph, gradient of its dot
product with p) and the actor half of one trpo_update (:228-319) in any dtype -- and the error bound.  Not a product path.

Error bound: the yardstick is float64 autograd of the reference's expression.  A fused quantity's rms error may be at most
FACTOR x the rms error of the same expression under torch fp32 autograd on the same inputs, with a floor of 2^-24 of the quantity's
rms (`within`)."""
import copy
import ctypes
import json
import math
import os
import types

import numpy as np
import torch

import marl_modules as mm

FACTOR = 2.0
FLOOR = 2.0 ** -24


def make_actor(obs_dim, act_dim, hidden, layer_N, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    actor = mm.Actor(obs_dim, act_dim, hidden=hidden, layer_N=layer_N)
    mm.randomize(actor, g, scale)
    return actor


def make_critic(share_dim, hidden, layer_N, seed):
    g = torch.Generator().manual_seed(seed + 1)
    torch.manual_seed(seed + 1)
    critic = mm.Critic(share_dim, hidden=hidden, layer_N=layer_N)
    mm.randomize(critic, g)
    return critic


def mean_of(actor, x):
    hd = actor.act.action_out
    return torch.nn.functional.linear(mm.base_forward(actor.base, x), hd.fc_mean.weight, hd.fc_mean.bias)


def std_of(actor):
    hd = actor.act.action_out
    return torch.sigmoid(hd.log_std / hd.std_x_coef) * hd.std_y_coef


def names_of(actor):
    return [n for n, _ in actor.named_parameters()]


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def rms_err(a, ref):
    return rms(a.double().cpu() - ref.double().cpu())


def within(fused, fp32, ref, factor=FACTOR):
    """(ok, ratio, bound): the fused quantity's rms error against float64 within factor x torch fp32 autograd's own, floor 2^-24 of the scale."""
    e_fused, e_fp32 = rms_err(fused, ref), rms_err(fp32, ref)
    bound = max(factor * e_fp32, FLOOR * rms(ref))
    return e_fused <= bound, e_fused / max(e_fp32, 1e-300), bound


def jt_g(actor, x, g):
    """J^T g per parameter (zeros for log_std), by autograd in the actor's dtype."""
    params = list(actor.parameters())
    grads = torch.autograd.grad((mean_of(actor, x) * g).sum(), params, allow_unused=True)
    return [torch.zeros_like(q) if d is None else d for q, d in zip(params, grads)]


def j_v(actor, x, direction):
    """J v [M, A] for a direction with one tensor per parameter, by forward-over-reverse autograd (the double-backward trick)."""
    params = list(actor.parameters())
    mu = mean_of(actor, x)
    w = torch.zeros_like(mu, requires_grad=True)
    grads = torch.autograd.grad(mu, params, w, create_graph=True, allow_unused=True)
    dot = sum((d * v).sum() for d, v in zip(grads, direction) if d is not None)
    return torch.autograd.grad(dot, w)[0]


def gaussian_kl(mu_old, std_old, mu, std):
    kl = torch.log(std) - torch.log(std_old) + (std_old.pow(2) + (mu_old - mu).pow(2)) / (2.0 * std.pow(2)) - 0.5
    return kl.sum(1, keepdim=True)


def flat(ts):
    return torch.cat([t.contiguous().view(-1) for t in ts if t is not None])


def fvp_autograd(actor, x, p, damping=0.1):
    """The reference's fisher_vector_product in the actor's dtype."""
    params = list(actor.parameters())
    mu, std = mean_of(actor, x), std_of(actor)
    kl = gaussian_kl(mu.detach(), std.detach(), mu, std).mean()
    kl_grad = flat(torch.autograd.grad(kl, params, create_graph=True, allow_unused=True))
    return flat(torch.autograd.grad((kl_grad * p).sum(), params, allow_unused=True)).detach() + damping * p


def to_dtype(module, dtype):
    return copy.deepcopy(module).to(dtype)


def make_sample(actor, critic, M, obs_dim, share_dim, seed, adv_scale=1.0, noise=0.3):
    """A minibatch in the generators' tuple layout, drawn around the actor's own policy."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    obs, share = rn(M, obs_dim) * 2.0, rn(M, share_dim) * 2.0
    with torch.no_grad():
        mu, std = mean_of(actor, obs), std_of(actor)
        v = torch.nn.functional.linear(mm.base_forward(critic.base, share), critic.v_out.weight, critic.v_out.bias)
    A = mu.shape[1]
    actions = mu + std * rn(M, A)
    old_logp = mm.log_prob(mu, std, actions) + noise / A ** 0.5 * rn(M, A)
    adv = adv_scale * rn(M, 1)
    vp, ret = v + 0.3 * rn(M, 1), v + rn(M, 1)
    masks = (torch.rand(M, 1, generator=g) > 0.2).float()
    factor = torch.exp(0.3 * rn(M, 1))
    return (share, obs, None, None, actions, vp, ret, None, masks, old_logp, adv, None, factor)


def actor_update(actor, sample, cfg, fvp=None):
    """The actor half of hatrpo_trainer.py's trpo_update (:228-319) in the actor's dtype, on a COPY of the actor: the surrogate's
    gradient, conjugate gradient over `fvp` (default: the reference's double backward), the step and the line search.  Returns a dict:
    loss_grad, step_dir, full_step, tries, accepted, params (flat, afterwards) and per try kl, loss_improve, expected_improve."""
    actor = copy.deepcopy(actor)
    dt = next(actor.parameters()).dtype
    c = lambda t: t.to(dt)
    obs, actions, masks, old_logp, adv, factor = c(sample[1]), c(sample[4]), c(sample[8]), c(sample[9]), c(sample[10]), c(sample[12])
    params_list = list(actor.parameters())

    def surrogate():
        mu, std = mean_of(actor, obs), std_of(actor)
        ratio = torch.exp((mm.log_prob(mu, std, actions) - old_logp).sum(-1, keepdim=True))
        s = torch.sum(ratio * factor * adv, dim=-1, keepdim=True)
        return ((s * masks).sum() / masks.sum() if cfg["use_policy_active_masks"] else s.mean()), mu, std

    loss, mu_old, std_old = surrogate()
    mu_old, std_old = mu_old.detach(), std_old.detach()
    loss_grad = flat(torch.autograd.grad(loss, params_list, allow_unused=True)).detach()
    fvp = fvp or (lambda p: fvp_autograd(actor, obs, p))
    x, r, p = torch.zeros_like(loss_grad), loss_grad.clone(), loss_grad.clone()
    rdotr = torch.dot(r, r)
    for _ in range(10):
        avp = fvp(p)
        alpha = rdotr / torch.dot(p, avp)
        x += alpha * p
        r -= alpha * avp
        new = torch.dot(r, r)
        p = r + new / rdotr * p
        rdotr = new
        if rdotr < 1e-10:
            break
    step_dir = x
    shs = 0.5 * (step_dir * fvp(step_dir)).sum()
    full_step = step_dir / torch.sqrt(shs / cfg["kl_threshold"])
    expected = float((loss_grad * full_step).sum())
    params = flat([q.data for q in params_list]).clone()

    def write(vec):
        i = 0
        for q in params_list:
            q.data.copy_(vec[i:i + q.numel()].view(q.shape))
            i += q.numel()

    out = {"loss_grad": loss_grad, "step_dir": step_dir, "full_step": full_step, "kl": [], "loss_improve": [], "expected_improve": [], "accepted": False}
    fraction = 1.0
    for t in range(cfg["ls_step"]):
        write(params + fraction * full_step)
        with torch.no_grad():
            new_loss, mu, std = surrogate()
            kl = float(gaussian_kl(mu_old, std_old, mu, std).mean())
        improve = float(new_loss) - float(loss.detach())
        out["kl"].append(kl)
        out["loss_improve"].append(improve)
        out["expected_improve"].append(expected)
        if kl < cfg["kl_threshold"] and improve / expected > cfg["accept_ratio"] and improve > 0:
            out["accepted"] = True
            break
        expected *= 0.5
        fraction *= 0.5
    out["tries"] = t + 1
    if not out["accepted"]:
        write(params)
    out["params"] = flat([q.data for q in params_list]).clone()
    return out


def margins(run, cfg):
    """The smallest distance of a deciding quantity from its threshold over the tries of `run`, each relative to the threshold's own
    scale: kl against kl_threshold, loss_improve / expected_improve against accept_ratio, loss_improve against 0 (over |expected|)."""
    m = math.inf
    for kl, li, ei in zip(run["kl"], run["loss_improve"], run["expected_improve"]):
        m = min(m, abs(kl - cfg["kl_threshold"]) / cfg["kl_threshold"], abs(li / ei - cfg["accept_ratio"]), abs(li) / abs(ei))
    return m


def deviation(run_a, run_b, cfg):
    """The largest difference of the same deciding quantities between two runs over their common tries, in margins()' units."""
    d = 0.0
    for ka, la, ea, kb, lb, eb in zip(run_a["kl"], run_a["loss_improve"], run_a["expected_improve"], run_b["kl"], run_b["loss_improve"],
                                      run_b["expected_improve"]):
        d = max(d, abs(ka - kb) / cfg["kl_threshold"], abs(la / ea - lb / eb), abs(la / abs(ea) - lb / abs(eb)))
    return d


def config(**over):
    cfg = {"kl_threshold": 0.016, "ls_step": 10, "accept_ratio": 0.5, "clip_param": 0.2, "num_mini_batch": 1, "data_chunk_length": 1,
           "value_loss_coef": 1.0, "entropy_coef": 0.0, "max_grad_norm": 10.0, "huber_delta": 10.0, "use_recurrent_policy": False,
           "use_naive_recurrent_policy": False, "use_max_grad_norm": True, "use_clipped_value_loss": True, "use_huber_loss": True,
           "use_popart": True, "use_value_active_masks": False, "use_policy_active_masks": False}
    cfg.update(over)
    return cfg


def make_policy(actor, critic, lr=5e-4, eps=1e-5):
    return types.SimpleNamespace(actor=actor, critic=critic,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=lr, eps=eps),
                                 critic_optimizer=torch.optim.Adam(critic.parameters(), lr=lr, eps=eps))


# ---- the two entries through ctypes, as a C caller sees them -----------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ptrs(ts):
    return None if ts is None else (ctypes.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


def entry_problem(actor, x, seed=0):
    """Everything one call of each entry reads and writes, on x's device: saved state, parameters, g, a direction, and outputs."""
    from massive_marl_benchmark_amd.algorithms.marl.hatrpo import _ActorMap
    amap = _ActorMap(actor)
    mu, hs = amap.forward(x)
    gen = torch.Generator().manual_seed(seed)
    M, A = mu.shape
    dev = x.device
    like = lambda ts: [torch.randn(t.shape, generator=gen).to(dev) for t in ts]
    pr = {"amap": amap, "M": M, "dims": list(amap.dims), "blocks": amap.blocks, "eps": amap.eps, "x": x.contiguous(), "h": [h.contiguous() for h in hs],
          "ln_g": [ln.weight.data for ln in amap.lns], "ln_t": [ln.bias.data for ln in amap.lns], "w": [lin.weight.data for lin in amap.lins],
          "g": torch.randn(M, A, generator=gen).to(dev), "col_scale": (torch.rand(A, generator=gen) + 0.5).to(dev)}
    pr["vg"], pr["vt"], pr["vw"] = like(pr["ln_g"]), like(pr["ln_t"]), like(pr["w"])
    pr["vc"] = like([lin.bias.data for lin in amap.lins])
    return pr


SENTINEL = 12345.0


def fresh_outputs(pr):
    f = lambda ts: [torch.full_like(t, SENTINEL) for t in ts]
    return {"dln_g": f(pr["ln_g"]), "dln_t": f(pr["ln_t"]), "dw": f(pr["w"]), "db": f(pr["vc"]),
            "rmu": torch.full((pr["M"], pr["dims"][-1]), SENTINEL, device=pr["x"].device)}


def untouched(out):
    return all(bool((t == SENTINEL).all()) for v in out.values() for t in (v if isinstance(v, list) else [v]))


def call(L, idx, stream, which, pr, out, ws, nbytes, **over):
    """rc of mms_ln_mlp_grad / mms_ln_mlp_jvp; `over` replaces arguments by name (M, dims, blocks, eps, or a pointer argument -> None)."""
    a = dict(pr, **out)
    a.update(over)
    dims = (ctypes.c_int32 * len(a["dims"]))(*a["dims"])
    head = (idx, a["blocks"], a["M"], dims, a["eps"], _p(a["x"]), _ptrs(a["h"]), _ptrs(a["ln_g"]), _ptrs(a["ln_t"]), _ptrs(a["w"]))
    nb = None if nbytes is None else ctypes.byref(nbytes)
    if which == "grad":
        return L.mms_ln_mlp_grad(*head, _p(a["g"]), _ptrs(a["dln_g"]), _ptrs(a["dln_t"]), _ptrs(a["dw"]), _ptrs(a["db"]), ws, nb, stream)
    return L.mms_ln_mlp_jvp(*head, _ptrs(a["vg"]), _ptrs(a["vt"]), _ptrs(a["vw"]), _ptrs(a["vc"]), _p(a["col_scale"]), _p(a["rmu"]), ws, nb, stream)


def workspace(L, idx, stream, which, pr, device):
    """(aligned pointer, c_int64 size, the tensor that owns it) from the size query."""
    nbytes = ctypes.c_int64(-1)
    assert call(L, idx, stream, which, pr, fresh_outputs(pr), None, nbytes) == 0
    assert nbytes.value >= 0
    buf = torch.zeros(nbytes.value + 512, dtype=torch.uint8, device=device)
    at = buf.data_ptr() + (-buf.data_ptr()) % 256
    return at, nbytes, buf


def run_entries(L, idx, stream, pr, device):
    """Both entries once: {"dln_g": [...], "dln_t": [...], "dw": [...], "db": [...], "rmu": tensor}."""
    out = fresh_outputs(pr)
    for which in ("grad", "jvp"):
        at, nbytes, buf = workspace(L, idx, stream, which, pr, device)
        rc = call(L, idx, stream, which, pr, out, ctypes.c_void_p(at), nbytes)
        assert rc == 0, L.mms_last_error(None)
        if device != "cpu" and str(device) != "cpu":
            torch.cuda.synchronize()
    return out


def reference_outputs(actor, pr, dtype):
    """The same outputs by autograd in `dtype` (on the CPU)."""
    a = to_dtype(actor, dtype).cpu()
    amap = pr["amap"]
    x, g = pr["x"].cpu().to(dtype), pr["g"].cpu().to(dtype)
    by_param = dict(zip([id(q) for q in amap.params], jt_g(a, x, g)))
    out = {"dln_g": [by_param[id(ln.weight)] for ln in amap.lns], "dln_t": [by_param[id(ln.bias)] for ln in amap.lns],
           "dw": [by_param[id(lin.weight)] for lin in amap.lins], "db": [by_param[id(lin.bias)] for lin in amap.lins]}
    direction = []
    for kind, l in amap.order:
        direction.append({"g": pr["vg"], "t": pr["vt"], "w": pr["vw"], "c": pr["vc"]}[kind][l].cpu().to(dtype) if kind != "s"
                         else torch.zeros(pr["dims"][-1], dtype=dtype))
    out["rmu"] = j_v(a, x, direction) * pr["col_scale"].cpu().to(dtype)
    return out


def compare_outputs(got, fp32, ref, record=None, label=""):
    """Every output against float64 within the bound; returns the worst ratio to torch fp32 autograd's own error."""
    worst = 0.0
    for key in ("dln_g", "dln_t", "dw", "db", "rmu"):
        for i, (a, b, c) in enumerate(zip(*[(v[key] if isinstance(v[key], list) else [v[key]]) for v in (got, fp32, ref)])):
            ok, ratio, bound = within(a, b, c)
            print("%s %s[%d]: rms error %.3g, torch fp32 %.3g, ratio %.3g, scale %.3g" % (label, key, i, rms_err(a, c), rms_err(b, c), ratio, rms(c)))
            assert ok, (label, key, i, rms_err(a, c), bound)
            if rms_err(b, c) > 0:
                worst = max(worst, ratio)
            if record is not None:
                record["%s %s[%d]" % (label, key, i)] = {"rms_error": rms_err(a, c), "torch_fp32_rms_error": rms_err(b, c), "scale": rms(c)}
    return worst


def write_error_record(path, what, entries):
    """Merge `entries` under key `what` into the JSON record at `path` (profiles/hatrpo_error.json); only where MMS_HATRPO_RECORD names
    the file."""
    if not path:
        return
    try:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[what] = entries
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass

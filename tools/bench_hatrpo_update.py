#!/usr/bin/env python3
"""HATRPO's update of one agent (agents/algorithms/marl/hatrpo_trainer.py:181-319) at the shipped widths: obs 46 -> 512 x 3 -> 8 actions,
share_obs 388, cfg/hatrpo/config.yaml (kl_threshold 0.016, ls_step 10, accept_ratio 0.5, PopArt, Huber, clipped value loss), actor and
critic of tests/marl_modules.py with perturbed parameters, a minibatch drawn around the actor's own policy (tests/hatrpo_check.py).
Row counts: 32768 (8 steps x 4096 envs, num_mini_batch 1) and 640 (the reference's 80 rollout threads).

Three series, in one process on one card, alternating within every repeat:
  autograd      fvp="autograd": the reference's Fisher-vector product (the KL between the actor and itself, autograd.grad with
                create_graph, autograd.grad of its dot product with p) -- the baseline;
  fisher-torch  the same Fisher algebra as fvp="fisher" in plain torch ops, written here: one saved forward, J p by a forward-mode pass over
                its activations, J^T g by autograd.grad over its retained graph -- what the algebra alone saves;
  fisher        fvp="fisher": mms_ln_mlp_jvp + mms_ln_mlp_grad -- what the kernels add.
Measured: (a) one Fisher-vector product from standing state, (b) one whole trpo_update (critic step, actor gradient, 10 CG steps, the
shs product, the line search).  Each: warm-up, then --repeats timings between HIP events; the line reports the median and the spread
(min, max).  (b) restores both networks, the critic's optimizer and the normaliser before every call, outside the timed window, and
records the line search's tries.  One JSON line per series and row count, then one line with the ratios.

    python tools/bench_hatrpo_update.py [--rows 32768 640] [--repeats 7] [--warmup 2] [--out profiles/hatrpo_update_bench.jsonl]
"""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SERIES = ("autograd", "fisher-torch", "fisher")


class TorchFisherState:
    """LnMlpState's interface (grad, jvp) in torch ops over one saved forward."""

    def __init__(self, amap, x, hs):
        import torch
        import torch.nn.functional as F
        self.amap = amap
        self.M = x.shape[0]
        self.params = amap.params
        # the saved forward, with its graph (J^T g is a backward over it) and the pieces the forward-mode pass reads
        self.xhat, self.rstd, self.u, self.fp = [], [], [], []
        v = x
        for l, ln in enumerate(amap.lns):
            mean = v.mean(-1, keepdim=True)
            rstd = torch.rsqrt(v.var(-1, unbiased=False, keepdim=True) + amap.eps)
            xhat = (v - mean) * rstd
            u = xhat * ln.weight + ln.bias
            self.xhat.append(xhat.detach())
            self.rstd.append(rstd.detach())
            self.u.append(u.detach())
            a = F.linear(u, amap.lins[l].weight, amap.lins[l].bias)
            if l == len(amap.lns) - 1:
                self.mu = a
                break
            v = F.elu(a)
            self.fp.append(torch.where(v.detach() > 0, torch.ones_like(v), v.detach() + 1.0))

    def grad(self, g):
        import torch
        grads = torch.autograd.grad(self.mu, self.params, g, retain_graph=True, allow_unused=True)
        return torch.cat([torch.zeros_like(q).view(-1) if d is None else d.contiguous().view(-1) for q, d in zip(self.params, grads)])

    def jvp(self, p, col_scale=None):
        import torch.nn.functional as F
        v = self.amap.split(p)
        ru = v["g"][0] * self.xhat[0] + v["t"][0]
        for l, lin in enumerate(self.amap.lins):
            ra = F.linear(ru, lin.weight.data) + F.linear(self.u[l], v["w"][l], v["c"][l])
            if l == len(self.amap.lins) - 1:
                return ra if col_scale is None else ra * col_scale
            rh = self.fp[l] * ra
            xh = self.xhat[l + 1]
            ln = self.amap.lns[l + 1]
            ru = ln.weight.data * self.rstd[l + 1] * (rh - rh.mean(-1, keepdim=True) - xh * (rh * xh).mean(-1, keepdim=True)) + v["g"][l + 1] * xh + v["t"][l + 1]


def timed(fn, reset, warmup, repeats, orders):
    """Per series name: the timings (ms) of fn[name], the series alternating within every repeat."""
    import torch
    out = {k: [] for k in fn}
    for rep in range(warmup + repeats):
        for name in orders[rep % len(orders)]:
            if reset:
                reset(name)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn[name]()
            b.record()
            b.synchronize()
            if rep >= warmup:
                out[name].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32768, 640])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_hatrpo_update: no GPU (timings on a CPU say nothing; nothing falls back)")
    import hatrpo_check as hc
    from massive_marl_benchmark_amd.algorithms.marl import hatrpo
    dev = torch.device("cuda:0")
    lines = []
    orders = [SERIES, SERIES[::-1], (SERIES[1], SERIES[2], SERIES[0])]
    for M in args.rows:
        cfg = hc.config()
        actor0, critic0 = hc.make_actor(46, 8, args.hidden, 2, 31), hc.make_critic(388, args.hidden, 2, 31)
        sample = tuple(None if t is None else t.to(dev) for t in hc.make_sample(actor0, critic0, M, 46, 388, 32))
        trainers, states0 = {}, {}
        for name in SERIES:
            policy = hc.make_policy(copy.deepcopy(actor0).to(dev), copy.deepcopy(critic0).to(dev))
            t = hatrpo.HATRPO(cfg, policy, dev, fvp="autograd" if name == "autograd" else "fisher")
            trainers[name] = t
            states0[name] = (copy.deepcopy(policy.actor.state_dict()), copy.deepcopy(policy.critic.state_dict()),
                             copy.deepcopy(policy.critic_optimizer.state_dict()))
        obs = sample[1].contiguous()
        p = torch.randn(sum(q.numel() for q in actor0.parameters()), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

        # (a) one Fisher-vector product from standing state
        fvps = {}
        for name in SERIES:
            t = trainers[name]
            if name == "autograd":
                fvps[name] = lambda t=t: t._fvp_autograd(obs, p)
                continue
            mu, hs = t._map.forward(obs)
            state = (hatrpo.LnMlpState if name == "fisher" else TorchFisherState)(t._map, obs, hs)
            std = t._std().detach()
            head = t.policy.actor.act.action_out
            curv = 2.0 * ((1.0 - torch.sigmoid(head.log_std.detach() / head.std_x_coef)) / head.std_x_coef) ** 2
            scale = (1.0 / (M * std ** 2)).contiguous()
            fvps[name] = lambda t=t, state=state, scale=scale, curv=curv: t._fvp_fisher(state, scale, curv, p)
        ref = fvps["autograd"]()
        agree = {name: float((fvps[name]() - ref).norm() / ref.norm()) for name in SERIES}
        fvp_ms = timed(fvps, None, args.warmup, args.repeats * 3, orders)
        del fvps, state

        # (b) one whole trpo_update
        tries = {k: [] for k in SERIES}

        def reset(name):
            t = trainers[name]
            a, c, o = states0[name]
            t.policy.actor.load_state_dict(a)
            t.policy.critic.load_state_dict(c)
            t.policy.critic_optimizer.load_state_dict(copy.deepcopy(o))
            if t.value_normalizer is not None:
                t.value_normalizer.reset_parameters()

        def update(name):
            t = trainers[name]
            with contextlib.redirect_stdout(io.StringIO()):
                if name == "fisher-torch":
                    keep = hatrpo.LnMlpState
                    hatrpo.LnMlpState = TorchFisherState
                    try:
                        t.trpo_update(sample)
                    finally:
                        hatrpo.LnMlpState = keep
                else:
                    t.trpo_update(sample)
            tries[name].append(t.last["tries"])
        upd_ms = timed({k: (lambda k=k: update(k)) for k in SERIES}, reset, args.warmup, args.repeats, orders)
        for name in SERIES:
            f, u = fvp_ms[name], upd_ms[name]
            lines.append({"bench": "hatrpo_update", "series": name, "rows": M, "widths": [46, args.hidden, args.hidden, args.hidden, 8],
                          "device": torch.cuda.get_device_name(0), "fvp_ms_median": statistics.median(f), "fvp_ms_min": min(f), "fvp_ms_max": max(f),
                          "fvp_timings": len(f), "fvp_rel_diff_to_autograd": agree[name], "update_ms_median": statistics.median(u),
                          "update_ms_min": min(u), "update_ms_max": max(u), "update_timings": len(u), "line_search_tries": tries[name][-len(u):]})
        med = lambda name, k: statistics.median((fvp_ms if k == "fvp" else upd_ms)[name])
        lines.append({"bench": "hatrpo_update", "rows": M, "ratios": {
            "fvp autograd / fisher": med("autograd", "fvp") / med("fisher", "fvp"), "fvp autograd / fisher-torch": med("autograd", "fvp") / med("fisher-torch", "fvp"),
            "update autograd / fisher": med("autograd", "upd") / med("fisher", "upd"),
            "update autograd / fisher-torch": med("autograd", "upd") / med("fisher-torch", "upd")}})
        del trainers
        torch.cuda.empty_cache()
    for line in lines:
        print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

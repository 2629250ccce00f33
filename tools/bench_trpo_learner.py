#!/usr/bin/env python3
"""The TRPO and PPO learners (algorithms/rl/trpo/trpo.py, ppo/ppo.py) on their opt-in routes, in one process on the HIP device, at the
shipped shape: 8192 envs x 8 steps (65536 stored rows, 4 minibatches of 16384), 388 observations, 80 actions, [1024, 1024, 512] ELU
networks, cfg/trpo/config.yaml's and cfg/ppo/config.yaml's update (5 epochs; cg_nsteps 3, max_num_backtrack 10, step_fraction 0.1).
The rollout is seeded data collected by a behaviour policy a small step away from the start, so mu != old_mu everywhere.

  heads     mms_trpo_heads alone at [16384, 80] per output subset the learner asks for, through the minibatch's index vector: the time
            per call and GB/s over the bytes the subset needs
  product   one curvature product (H + damping I) v of a prepared minibatch: the reference's expression over torch autograd on the
            plain module ("autograd"), the same expression over the module's kernels (fused_grad=True: "autograd_kernels"), and
            fvp="direct" (mms_mlp_grad_rop, mms_trpo_heads, mms_mlp_grad)
  trpo      one `TRPO.update()`: the default route (what the reference's trpo.py obtains from the modules), `fused_update`, and
            `fused_update` + fvp="direct"
  ppo       one `PPO.update()`: the default route against `fused_update`

After warm-up, `--rounds` rounds alternating the sides; `heads` and `product` between two device events, the updates on the host clock
around a call that ends in a device synchronise (an update reads the device from the host many times).  Every update starts from the
same parameters and optimizer state (restored before each call, outside the window).  Per side the median with min and max; where two
sides' ranges overlap the line says "no result".  One JSON line per series on stdout, appended to --out.

    python tools/bench_trpo_learner.py [--series heads,product,trpo,ppo] [--envs 8192] [--rounds 5] [--out profiles/trpo_learner_bench.jsonl]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, A, T = 388, 80, 8
TRPO_LEARN = dict(optim_stepsize=1e-3, cliprange=0.2, nsteps=T, noptepochs=5, nminibatches=4, max_grad_norm=10, schedule="adaptive", gamma=0.99, lam=0.95,
                  init_noise_std=0.8, damping=0.1, cg_nsteps=3, max_kl=0.1, max_num_backtrack=10, accept_ratio=0.01, step_fraction=0.1)
PPO_LEARN = dict(optim_stepsize=3e-4, cliprange=0.2, ent_coef=0, nsteps=T, noptepochs=5, nminibatches=4, max_grad_norm=1, schedule="adaptive",
                 desired_kl=0.016, gamma=0.96, lam=0.95, init_noise_std=0.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", default="heads,product,trpo,ppo")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--hidden", type=int, nargs="+", default=[1024, 1024, 512])
    ap.add_argument("--reps", type=int, default=20, help="calls per window of `heads`; `product` takes a quarter of it, the updates one")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="\"cpu\": a rehearsal on the CPU build (wall-clock windows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trpo_learner_bench.jsonl"))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("bench_trpo_learner.py: at least 5 rounds")
    import numpy as np
    import torch
    from massive_marl_benchmark_amd.algorithms.rl.ppo import PPO
    from massive_marl_benchmark_amd.algorithms.rl.trpo import TRPO
    from massive_marl_benchmark_amd.algorithms.rl.trpo.heads import StoredRows, trpo_heads
    from massive_marl_benchmark_amd.spaces import Box
    dev = torch.device(args.device)
    gpu = dev.type == "cuda"
    if gpu and not torch.cuda.is_available():
        sys.exit("bench_trpo_learner.py needs a HIP device (or --device cpu for a rehearsal)")
    sync = torch.cuda.synchronize if gpu else (lambda: None)
    summary = lambda ts: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    series = args.series.split(",")
    envs, rows = args.envs, args.envs * T // 4

    def emit(res):
        res.update(device=torch.cuda.get_device_name(0) if gpu else "cpu", envs=envs, rounds=args.rounds, hidden=args.hidden, minibatch_rows=rows)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def verdict(res, a, b):
        """`b` against `a`: the ratio of the medians where the two ranges do not overlap, "no result" where they do."""
        if res[a]["min"] <= res[b]["max"] and res[b]["min"] <= res[a]["max"]:
            return "%s against %s: no result (the ranges overlap)" % (b, a)
        return "%s / %s = %.3f" % (b, a, res[b]["median"] / res[a]["median"])

    def alternate(paths, reps, warm=2, events=True, before=None):
        for k, f in paths.items():
            for _ in range(warm):
                if before:
                    before(k)
                f()
        sync()
        if gpu:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        res = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, f in paths.items():
                if before:
                    before(k)
                    sync()
                t0 = time.perf_counter()
                if gpu and events:
                    e0.record()
                for _ in range(reps):
                    f()
                if gpu and events:
                    e1.record()
                    e1.synchronize()
                sync()
                res[k].append((e0.elapsed_time(e1) if gpu and events else 1e3 * (time.perf_counter() - t0)) / reps)
        return {k: summary(v) for k, v in res.items()}

    env = types.SimpleNamespace(observation_space=Box(-np.inf, np.inf, (W,)), state_space=Box(-np.inf, np.inf, (0,)), action_space=Box(-1.0, 1.0, (A,)),
                                num_envs=envs)
    policy = {"pi_hid_sizes": list(args.hidden), "vf_hid_sizes": list(args.hidden), "activation": "elu"}

    def make(cls, learn, **keys):
        torch.manual_seed(0)
        return cls(env, {"policy": policy, "learn": dict(learn, **keys)}, device=str(dev), log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)

    # one behaviour policy, one rollout, one start for every learner
    base = make(TRPO, TRPO_LEARN)
    ac, g = base.actor_critic, torch.Generator().manual_seed(1)
    with torch.no_grad():
        for t in range(T):
            obs = torch.randn(envs, W, generator=g).to(dev)
            act = ac.actor(obs) + (2 * ac.log_std).exp() * torch.randn(envs, A, generator=g).to(dev)
            logp, _, value, mu, sigma = ac.evaluate(obs, None, act)
            rew, done = torch.randn(envs, 1, generator=g).to(dev), (torch.rand(envs, 1, generator=g) < 0.05).to(torch.uint8).to(dev)
            base.storage.add_transitions(obs, torch.zeros(envs, 0, device=dev), act, rew, done, value, logp.view(-1, 1), mu, sigma)
        base.storage.compute_returns(torch.zeros(envs, 1, device=dev), 0.99, 0.95)
        start = {k: v + 0.002 * torch.randn(v.shape, generator=g).to(dev) for k, v in ac.state_dict().items()}
    fields = ("observations", "states", "rewards", "actions", "dones", "actions_log_prob", "values", "returns", "advantages", "mu", "sigma")

    def learner(cls, learn, **keys):
        agent = make(cls, learn, **keys)
        agent.actor_critic.load_state_dict(start)
        for k in fields:
            setattr(agent.storage, k, getattr(base.storage, k))
        agent.storage.step = T
        return agent

    def restorer(agents):
        """Every timed update starts where the first one did: the parameters and the optimizer's state, restored outside the window."""
        opt0 = {k: copy.deepcopy(a.optimizer.state_dict()) for k, a in agents.items()}

        def before(k):
            agents[k].actor_critic.load_state_dict(start)
            agents[k].optimizer.load_state_dict(copy.deepcopy(opt0[k]))
            agents[k].step_size = agents[k].learning_rate
        return before

    indices = torch.arange(rows, dtype=torch.int64, device=dev)

    if "heads" in series:
        stored = StoredRows(base.storage, indices)
        log_std = ac.log_std.detach()
        with torch.no_grad():
            mu = ac.actor(base.storage.observations.view(-1, W)[indices]).contiguous()
        rmu, olp = torch.randn(rows, A, generator=g).to(dev), stored.old_logp[indices].contiguous()
        subsets = {"loss (out, logp; dense old_logp)": (dict(mu=mu, stored=stored, old_logp=olp, want=("out", "logp")), 4 * rows * (2 * A + 3) + 8 * rows),
                   "first call (out, logp, gsur, gkl)": (dict(mu=mu, stored=stored, want=("out", "logp", "gsur", "gkl")), 4 * rows * (6 * A + 3) + 8 * rows),
                   "gn": (dict(rmu=rmu, want=("gn",)), 4 * rows * 2 * A)}
        res = alternate({k: (lambda kw=kw: trpo_heads(log_std, **kw)) for k, (kw, _) in subsets.items()}, args.reps)
        for k, (_, nbytes) in subsets.items():
            res[k]["bytes_needed"] = nbytes
            res[k]["achieved_GB_per_s"] = round(nbytes / (res[k]["median"] * 1e-3) / 1e9, 1)
        emit({"series": "heads", "rows": rows, "A": A, "unit": "ms per call (every launch of the entry and the output allocations of the Python call): "
              "median (min - max) over the rounds", **res})

    if "product" in series:
        sides = {"autograd": learner(TRPO, TRPO_LEARN), "autograd_kernels": learner(TRPO, TRPO_LEARN), "direct": learner(TRPO, TRPO_LEARN, fvp="direct")}
        sides["autograd_kernels"].actor_critic.fused_grad = True
        n = sum(p.numel() for p in ac.actor.parameters())
        v = torch.randn(n, generator=g).to(dev)
        calls = {}
        for k, agent in sides.items():
            b = agent._gather(indices)
            if k == "direct":
                agent._prepare_direct(b['obs'], indices)
                calls[k] = lambda agent=agent: agent.kl_hessian_times_vector(v, None)
            else:
                _, _, _, mu_b, sigma_b = agent.actor_critic.evaluate(b['obs'], None, b['actions'])
                kl = torch.mean(agent._kl(sigma_b, mu_b, b))
                calls[k] = lambda agent=agent, kl=kl: agent.kl_hessian_times_vector(v, kl)
        hv = {k: f() for k, f in calls.items()}
        rel = {k: float((hv[k] - hv["autograd"]).norm() / hv["autograd"].norm()) for k in hv}
        res = alternate(calls, max(1, args.reps // 4))
        emit({"series": "product", "parameters": n, "unit": "ms per product: median (min - max) over the rounds", "difference_from_autograd_rel_norm": rel,
              "verdict": [verdict(res, "autograd", "direct"), verdict(res, "autograd_kernels", "direct")], **res})
        del sides, calls, hv

    for name, cls, learn, routes in (("trpo", TRPO, TRPO_LEARN, {"default": {}, "fused_update": dict(fused_update=True),
                                                                  "fused_update+direct": dict(fused_update=True, fvp="direct")}),
                                     ("ppo", PPO, PPO_LEARN, {"default": {}, "fused_update": dict(fused_update=True)})):
        if name not in series:
            continue
        agents = {k: learner(cls, learn, **keys) for k, keys in routes.items()}
        means = {}

        def call(k):
            means[k] = agents[k].update()
            sync()
        first = {}
        for k in agents:
            call(k)
            first[k] = means[k]
        # (the restore state is taken AFTER one update, so that the optimizer's state exists; the parameters go back to the start)
        res = alternate({k: (lambda k=k: call(k)) for k in agents}, 1, warm=1, events=False, before=restorer(agents))
        assert all(np.isfinite(x) for m in means.values() for x in m), means
        extra = {}
        if name == "trpo":
            for k, a in agents.items():
                a.trace = []
                restorer({k: a})(k)
            extra["line_search (success, trials) of the first minibatches"] = {}
            for k, a in agents.items():
                a.update()
                extra["line_search (success, trials) of the first minibatches"][k] = [(bool(r["success"]), int(r["trials"])) for r in a.trace[:4]]
                a.trace = None
        others = [k for k in routes if k != "default"]
        emit({"series": name, "steps": "5 epochs x 4 minibatches", "unit": "ms per update(), host clock to a device synchronise: median (min - max) over "
              "the rounds", "means (value loss, surrogate loss) of the last timed update": {k: [round(x, 6) for x in m] for k, m in means.items()},
              "verdict": [verdict(res, "default", k) for k in others] + ([verdict(res, others[0], others[1])] if len(others) > 1 else []), **extra, **res})
        del agents
        if gpu:
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

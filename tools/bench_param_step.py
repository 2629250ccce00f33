#!/usr/bin/env python3
"""The parameter step -- gradient-norm clip + Adam + polyak -- as FusedAdam.clip_and_step (mms_param_step: two launches) against what
the learners run without it, on the HIP device.  Three sides everywhere:

  fused        optim.FusedAdam.clip_and_step (with the targets where there are any)
  torch        nn.utils.clip_grad_norm_ + torch.optim.Adam(defaults).step() + the per-parameter polyak loop: the parent path
  torch_fused  the same with torch.optim.Adam(fused=True): what the library can already do

  (a) ppo_call      the call alone on PPO's ActorCritic parameters (cfg/ppo/config.yaml: actor and critic [1024, 1024, 512] on TenAnt's
                    388 observations and 80 actions), max_grad_norm 1
  (b) maddpg_call   the call alone on one MADDPG agent's critic and its target at TenAnt's shapes (388 + 80 inputs, [1024, 1024, 512])
                    and at the 64-wide test networks, max_grad_norm 1, polyak 0.995
  (c) ddpg_update   one MADDPG.ddpg_update at TenAnt's shapes (tools/bench_maddpg_update.py's problem) per number of envs, config
                    "fused_step" on and off, and off with fused=True Adams
  (d) ppo_step      one PPO minibatch step as tools/bench_ppo_loss.py's `step` (8192 rows: gather, both networks, the fused loss head,
                    zero_grad, backward, then the parameter step) with the three parameter steps

(a), (b), (d): after warm-up, `--rounds` rounds alternating the sides, each `--reps` calls between two device events; (c): host-clock
windows that end in a device synchronise, the sides alternating.  Per side the median with min and max.  One JSON line per section on
stdout, appended to --out.

    python tools/bench_param_step.py [--sections a,b,c,d] [--envs 80,4096] [--reps 200] [--rounds 5] [--out profiles/param_step_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="a,b,c,d")
    ap.add_argument("--envs", default="80,4096")
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window of (a), (b), (d)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="\"cpu\": a rehearsal on the CPU build (wall-clock windows, no fused=True Adam)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_step_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn as nn
    from massive_marl_benchmark_amd.optim import FusedAdam
    dev = torch.device(args.device)
    gpu = dev.type == "cuda"
    if gpu and not torch.cuda.is_available():
        sys.exit("bench_param_step.py needs a HIP device (or --device cpu for a rehearsal)")
    sides = ("fused", "torch", "torch_fused") if gpu else ("fused", "torch")
    summary = lambda ts: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    def emit(res):
        res["device"] = torch.cuda.get_device_name(0) if gpu else "cpu"
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def sync():
        if gpu:
            torch.cuda.synchronize()

    def alternate(paths, reps, warm=8):
        """ms per call and side: args.rounds rounds alternating the sides, `reps` calls between two device events each."""
        for f in paths.values():
            for _ in range(warm):
                f()
        sync()
        res = {k: [] for k in paths}
        if gpu:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for k, f in paths.items():
                t0 = time.perf_counter()
                if gpu:
                    e0.record()
                for _ in range(reps):
                    f()
                if gpu:
                    e1.record()
                    e1.synchronize()
                res[k].append((e0.elapsed_time(e1) if gpu else 1e3 * (time.perf_counter() - t0)) / reps)
        return {k: summary(v) for k, v in res.items()}

    def make_adam(side, params, lr):
        if side == "fused":
            return FusedAdam(params, lr=lr)
        return torch.optim.Adam(params, lr=lr, fused=True) if side == "torch_fused" else torch.optim.Adam(params, lr=lr)

    def polyak_loop(params, targets, polyak):
        with torch.no_grad():
            for p, p_targ in zip(params, targets):
                p_targ.data.mul_(polyak)
                p_targ.data.add_((1 - polyak) * p.data)

    def call_alone(tensors, with_targets, max_norm=1.0, polyak=0.995, lr=3e-4):
        """The three sides on copies of `tensors` with fixed random gradients."""
        g = torch.Generator().manual_seed(0)
        paths = {}
        for side in sides:
            params = [nn.Parameter(t.detach().clone()) for t in tensors]
            for p in params:
                p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
            targets = [t.detach().clone() for t in tensors] if with_targets else None
            opt = make_adam(side, params, lr)
            if side == "fused":
                paths[side] = (lambda opt=opt, targets=targets: opt.clip_and_step(max_norm, targets=targets, polyak=polyak if targets else None))
            else:
                def plain(opt=opt, params=params, targets=targets):
                    nn.utils.clip_grad_norm_(params, max_norm)
                    opt.step()
                    if targets:
                        polyak_loop(params, targets, polyak)
                paths[side] = plain
        return alternate(paths, args.reps)

    sections = args.sections.split(",")
    if "a" in sections:
        from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
        from massive_marl_benchmark_amd.utils.config import default_train_cfg
        cfg = default_train_cfg("ppo")
        ac = ActorCritic((388,), (0,), (80,), cfg["learn"]["init_noise_std"], cfg["policy"], seed=0).to(dev)
        tensors = list(ac.parameters())
        numel = sum(t.numel() for t in tensors)
        res = {"bench": "param_step", "section": "ppo_call", "tensors": len(tensors), "elements": numel, "calls_per_round": args.reps, "rounds": args.rounds,
               # p, g, m, v read and p, m, v written (4 bytes each), g read once more for the norm
               "bytes_moved": 32 * numel, "ms": call_alone(tensors, False)}
        emit(res)
        del ac
    if "b" in sections:
        from massive_marl_benchmark_amd.algorithms.marl.maddpg.module import Critic
        for hidden in ([1024, 1024, 512], [64, 64]):
            so = types.SimpleNamespace(shape=(388,))
            sa = [types.SimpleNamespace(shape=(8,))] * 10
            critic = Critic(so, sa, hidden, nn.ELU(), dev)
            tensors = list(critic.q.parameters())
            numel = sum(t.numel() for t in tensors)
            emit({"bench": "param_step", "section": "maddpg_call", "hidden": hidden, "tensors": len(tensors), "elements": numel, "calls_per_round": args.reps,
                  "rounds": args.rounds, "bytes_moved": 44 * numel, "ms": call_alone(tensors, True)})
    if "c" in sections:
        from massive_marl_benchmark_amd.algorithms.marl.maddpg import MADDPG, MADDPG_policy
        N, OBS, SOBS, ACT, HIDDEN, ROWS = 10, 46, 388, 8, [1024, 1024, 512], 16
        o, s = types.SimpleNamespace(shape=(OBS,)), types.SimpleNamespace(shape=(SOBS,))
        a = types.SimpleNamespace(shape=(ACT,), high=np.ones(ACT, np.float32))

        def trainer(side):
            config = {"learning_rate": 5e-4, "hidden_size": HIDDEN, "activation": "elu", "act_noise": 0.1, "num_learning_epochs": 2, "num_mini_batch": 1,
                      "gamma": 0.96, "polyak": 0.995, "max_grad_norm": 1.0, "fused_step": side == "fused"}
            torch.manual_seed(1)
            policies = [MADDPG_policy(config, o, s, a, [a] * N, device=dev) for _ in range(N)]
            if side == "torch_fused":
                for po in policies:
                    po.actor_optimizer = torch.optim.Adam(po.actor.pi.parameters(), lr=po.lr, fused=True)
                    po.critic_optimizer = torch.optim.Adam(po.critic.q.parameters(), lr=po.lr, fused=True)
            return MADDPG(config, policies, N, device=dev)

        for envs in [int(v) for v in args.envs.split(",")]:
            g = torch.Generator().manual_seed(envs)
            rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)

            def padded(*lead):
                base = torch.zeros(*lead, 48, device=dev)
                base[..., :OBS] = rnd(*lead, OBS)
                return base[..., :OBS]
            samples = [{"obs": padded(ROWS, envs), "sobs": rnd(ROWS, envs, SOBS), "jact": torch.tanh(rnd(ROWS, envs, N * ACT)), "r": rnd(ROWS, envs, 1),
                        "obs2": padded(ROWS, envs), "sobs2": rnd(ROWS, envs, SOBS), "done": (torch.rand(ROWS, envs, 1, generator=g) < 0.05).to(torch.uint8).to(dev)}
                       for _ in range(N)]
            trainers = {side: trainer(side) for side in sides}
            first, times = {}, {side: [] for side in sides}
            for rnd_i in range(2 + args.rounds):                      # two warm-up rounds
                for side, t in trainers.items():
                    sync()
                    t0 = time.perf_counter()
                    v, _ = t.ddpg_update(samples)
                    sync()
                    if rnd_i >= 2:
                        times[side].append((time.perf_counter() - t0) * 1e3)
                    first.setdefault(side, float(v[0].detach()))
            emit({"bench": "param_step", "section": "ddpg_update", "agents": N, "hidden": HIDDEN, "ring_rows": ROWS, "envs": envs, "M": ROWS * envs,
                  "rounds": args.rounds, "ms": {k: summary(v) for k, v in times.items()}, "first_value_loss": first})
            del trainers, samples
            if gpu:
                torch.cuda.empty_cache()
    if "d" in sections:
        from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
        from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
        from massive_marl_benchmark_amd.utils.config import default_train_cfg
        cfg = default_train_cfg("ppo")
        learn = cfg["learn"]
        Nenv, T, W, A = 4096, learn["nsteps"], 388, 80
        M = Nenv * T // learn["nminibatches"]
        clip, ent_coef, value_coef = learn["cliprange"], learn["ent_coef"], 2.0
        torch.manual_seed(0)
        st = RolloutStorage(Nenv, T, (W,), (0,), (A,), device=str(dev), sampler="random")
        acs = {side: ActorCritic((W,), (0,), (A,), learn["init_noise_std"], cfg["policy"], seed=0).to(dev) for side in sides}
        ac = acs["fused"]
        with torch.no_grad():                                         # tools/bench_ppo_loss.py's synthetic rollout
            st.observations.normal_()
            obs = st.observations.view(-1, W)
            mu0 = torch.cat([ac.actor(x) for x in obs.split(8192)])
            v0 = torch.cat([ac.critic(x) for x in obs.split(8192)])
            l = ac.log_std.detach()
            act = mu0 + torch.exp(2.0 * l) * torch.randn_like(mu0)
            z = (act - mu0) * torch.exp(-2.0 * l)
            st.actions.copy_(act.view(T, Nenv, A))
            st.mu.copy_((mu0 + 0.02 * torch.randn_like(mu0)).view(T, Nenv, A))
            st.sigma.copy_(l.repeat(T * Nenv, 1).view(T, Nenv, A))
            st.actions_log_prob.copy_(((-0.5 * z * z - 2.0 * l - 0.5 * np.log(2 * np.pi)).sum(-1) + 0.1 * torch.randn(T * Nenv, device=dev)).view(T, Nenv, 1))
            st.values.copy_((v0 + 0.3 * torch.randn_like(v0)).view(T, Nenv, 1))
            st.returns.copy_((v0 + torch.randn_like(v0)).view(T, Nenv, 1))
            st.advantages.normal_()
        indices = torch.randperm(Nenv * T, device=dev)[:M]
        flat = lambda t: t.view(-1, *t.shape[2:])
        paths = {}
        for side in sides:
            net = acs[side]
            opt = make_adam(side, list(net.parameters()), 0.0)        # lr 0: the step's cost without moving the networks under the timing

            def step(net=net, opt=opt, side=side):
                loss, info = net.ppo_loss(flat(st.observations)[indices], None, st, indices, clip, value_coef, ent_coef, False)
                opt.zero_grad()
                loss.backward()
                if side == "fused":
                    opt.clip_and_step(learn["max_grad_norm"])
                else:
                    nn.utils.clip_grad_norm_(net.parameters(), learn["max_grad_norm"])
                    opt.step()
            paths[side] = step
        step_reps = max(20, args.reps // 4) if gpu else 1
        emit({"bench": "param_step", "section": "ppo_step", "num_envs": Nenv, "rows": M, "hidden": cfg["policy"]["pi_hid_sizes"], "calls_per_round": step_reps,
              "rounds": args.rounds, "ms": alternate(paths, step_reps, warm=4 if gpu else 1)})


if __name__ == "__main__":
    main()

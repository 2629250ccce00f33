#!/usr/bin/env python3
"""One `Runner.train()` of the on-policy MARL drop-in (algorithms/marl/runner.py) at TenAnt's shapes (10 agents, obs 46, share_obs 388,
8 actions, hidden 512, layer_N 2, episode_length 8, ppo_epoch 5, one minibatch) on the HIP device, and its factor passes alone, with
`fused_factor` on (GroupedPolicyInference.evaluate_actions: the grouped layers + mms_marl_heads_eval, 1 + num_agents calls) and off (the
modules' `actor.evaluate_actions` twice per agent and the product in torch, as the reference's Runner does), both in this process.

Per algorithm (mappo, happo) and env count (default 4096 and 80: 32768 and 640 stored rows per agent) two Runners over one TenAnt env
hold the same rollout (one is collected, the other's buffers and parameters are copies); then, in alternating rounds (modules, fused,
modules, ...), each round `--calls` passes between two host-clock reads that end in a device synchronise, after warm-up passes:

  train_*_ms    one whole train(): the permutation, per agent update_factor, trainer.train, the two log-probability passes, the product
  factor_*_ms   the same loop WITHOUT trainer.train: what the two passes per agent and the product cost by themselves

reported as the median round with (min - max), in ms per pass.  `verdict` compares the two windows: "faster" / "slower" when they do
not overlap, else "no result at that size".  `max_rel_diff_factor` is the largest relative difference of the two routes' factors after
the factor-only loop on identical parameters (a check that they compute the same thing).

The kernel alone: mms_marl_heads_eval on 10 networks x `--kernel-rows` rows (default 32768) of width 512, 8 actions, with and without the
factor, timed the same way (us per launch, and the GB/s of the [rows, 512] fp32 activations it reads).

`--series grouped`: instead of the above, MAPPO's `Runner.train()` with `grouped_update` off (the agent loop) and on (MAPPO.train_group: the
agents in lockstep, one mms_marl_ppo_loss_group call per step) at the same shapes, both with fused_block_update, FusedAdam optimizers
and fused_factor, from the same rollout, alternating in this process: `train_sequential_ms`, `train_grouped_ms`, the same windows and
verdict rule (profiles/marl_grouped_update_bench.jsonl), and a third route in the same rounds: `grouped_update` with `fused_head_update`
(heads.update_heads: the 2 x agents output heads of a step in one mms_marl_heads_fwd_group call, their backward in one
mms_marl_heads_grad_group call), `train_grouped_heads_ms`, with its windows against the agent loop's and against the grouped route's
(profiles/marl_head_update_bench.jsonl).  `--trace ROUTE --trains N` (with `--series grouped`): only that route (sequential, grouped,
grouped_heads) at the first size of --envs, the rollout and N `train()` calls and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats`; launches per `train()` are the difference between a run with N = 2 and one with N = 1.

One JSON line per measurement on stdout, appended to --out when given.

    python tools/bench_marl_runner.py [--envs 4096,80] [--algos mappo,happo] [--rounds 5] [--calls 2] [--out profiles/marl_runner_bench.jsonl]
    python tools/bench_marl_runner.py --series grouped [--envs 80,4096] [--out profiles/marl_grouped_update_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,80")
    ap.add_argument("--algos", default="mappo,happo")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-rows", type=int, default=32768)
    ap.add_argument("--out", default="")
    ap.add_argument("--series", default="factor", choices=("factor", "grouped"))
    ap.add_argument("--trace", default="", choices=("", "sequential", "grouped", "grouped_heads"), help="--series grouped: only this route, --trains train() calls")
    ap.add_argument("--trains", type=int, default=1)
    args = ap.parse_args()
    import torch
    import marl_runner_check as rc
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.algorithms.marl.runner import Runner, _rows
    if not torch.cuda.is_available():
        sys.exit("bench_marl_runner.py needs a HIP device")
    dev = "cuda:0"

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fns, calls, warmup):
        """fns: {name: callable}; alternating rounds; {name: (median, min, max)} in ms per pass"""
        for fn in fns.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

    def verdict(base_w, new_w):
        if new_w[2] < base_w[1]:
            return "faster"
        if new_w[1] > base_w[2]:
            return "slower"
        return "no result at that size"

    win = lambda w: {"median": round(w[0], 3), "min": round(w[1], 3), "max": round(w[2], 3)}

    def factor_only(r):
        """Runner.train's loop without trainer.train (runner.py: train)"""
        order = torch.randperm(r.num_agents)
        T, N = r.episode_length, r.n_rollout_threads
        factor = torch.ones(T, N, 1, device=r.device)
        if r.fused_factor:
            obs, acts = [_rows(b.obs[:-1]) for b in r.buffer], [_rows(b.actions) for b in r.buffer]
            old = [t.clone() for t in r.grouped.evaluate_actions(obs, acts)]
        for agent_id in order:
            a = int(agent_id)
            r.buffer[a].update_factor(factor)
            if r.fused_factor:
                r.grouped.evaluate_actions([obs[a]], [acts[a]], agents=[a], old_logp=[old[a]], factor=factor.view(-1, 1))
            else:
                old_logp = r._module_logp(a)
                new_logp = r._module_logp(a)
                factor = factor * torch.exp((new_logp - old_logp).reshape(T, N, -1).sum(dim=-1, keepdim=True))
        return factor

    def rollout_into(first, others):
        """one rollout on `first`, so that the buffers hold what a run leaves in them; the others receive copies of it and of the parameters"""
        first.warmup()
        for step in range(first.episode_length):
            values, actions, logp, rs, rsc = first.collect(step)
            obs, share_obs, rewards, dones, infos, _ = first.envs.step(actions)
            first.insert((obs, share_obs, rewards, dones, infos, values, actions, logp, rs, rsc))
        first.compute()
        for r in others:
            for a in range(first.num_agents):
                r.policy[a].actor.load_state_dict(first.policy[a].actor.state_dict())
                r.policy[a].critic.load_state_dict(first.policy[a].critic.state_dict())
                if r.trainer[a].value_normalizer is not None:
                    r.trainer[a].value_normalizer.load_state_dict(first.trainer[a].value_normalizer.state_dict())
                for k, v in vars(first.buffer[a]).items():
                    if torch.is_tensor(v):
                        getattr(r.buffer[a], k).copy_(v)

    if args.series == "grouped":
        from massive_marl_benchmark_amd.optim import FusedAdam
        for n in [int(v) for v in args.envs.split(",") if v]:
            env = rc.make_env("cuda", n)
            torch.manual_seed(1)
            over = dict(run_dir=tempfile.mkdtemp(), n_rollout_threads=n, hidden_size=512, ppo_epoch=5, num_env_steps=8 * n, fused_block_update=True)
            routes = {"sequential": dict(grouped_update=False), "grouped": dict(grouped_update=True), "grouped_heads": dict(grouped_update=True, fused_head_update=True)}
            if args.trace:
                r = Runner(env, rc.config("mappo", **routes[args.trace], **over))
                for pol in r.policy:
                    pol.actor_optimizer, pol.critic_optimizer = FusedAdam.from_torch(pol.actor_optimizer), FusedAdam.from_torch(pol.critic_optimizer)
                rollout_into(r, [])
                for _ in range(args.trains):
                    r.train()
                torch.cuda.synchronize()
                return
            pair = {k: Runner(env, rc.config("mappo", **kw, **over)) for k, kw in routes.items()}
            for r in pair.values():
                for pol in r.policy:
                    pol.actor_optimizer, pol.critic_optimizer = FusedAdam.from_torch(pol.actor_optimizer), FusedAdam.from_torch(pol.critic_optimizer)
            rollout_into(pair["sequential"], [pair["grouped"], pair["grouped_heads"]])
            trn = timed({k: r.train for k, r in pair.items()}, args.calls, args.warmup)
            emit({"bench": "marl_grouped_update", "algo": "mappo", "envs": n, "rows": 8 * n, "agents": pair["grouped"].num_agents, "hidden": 512, "ppo_epoch": 5,
                  "num_mini_batch": 1, "fused_block_update": True, "optimizer": "FusedAdam", "rounds": args.rounds, "calls": args.calls,
                  "train_sequential_ms": win(trn["sequential"]), "train_grouped_ms": win(trn["grouped"]),
                  "train_speedup_median": round(trn["sequential"][0] / trn["grouped"][0], 3), "train_verdict": verdict(trn["sequential"], trn["grouped"]),
                  "train_grouped_heads_ms": win(trn["grouped_heads"]), "heads_speedup_median_over_sequential": round(trn["sequential"][0] / trn["grouped_heads"][0], 3),
                  "heads_verdict_over_sequential": verdict(trn["sequential"], trn["grouped_heads"]),
                  "heads_speedup_median_over_grouped": round(trn["grouped"][0] / trn["grouped_heads"][0], 3),
                  "heads_verdict_over_grouped": verdict(trn["grouped"], trn["grouped_heads"])})
            del pair, env
            torch.cuda.empty_cache()
        return

    for n in [int(v) for v in args.envs.split(",") if v]:
        env = rc.make_env("cuda", n)
        for algo in args.algos.split(","):
            torch.manual_seed(1)
            over = dict(run_dir=tempfile.mkdtemp(), n_rollout_threads=n, hidden_size=512, ppo_epoch=5, num_env_steps=8 * n)
            fused = Runner(env, rc.config(algo, fused_factor=True, **over))
            plain = Runner(env, rc.config(algo, fused_factor=False, **over))
            fused.warmup()
            for step in range(fused.episode_length):                 # one rollout, so that the buffers hold what a run leaves in them
                values, actions, logp, rs, rsc = fused.collect(step)
                obs, share_obs, rewards, dones, infos, _ = env.step(actions)
                fused.insert((obs, share_obs, rewards, dones, infos, values, actions, logp, rs, rsc))
            fused.compute()
            for a in range(fused.num_agents):
                plain.policy[a].actor.load_state_dict(fused.policy[a].actor.state_dict())
                plain.policy[a].critic.load_state_dict(fused.policy[a].critic.state_dict())
                for k, v in vars(fused.buffer[a]).items():
                    if torch.is_tensor(v):
                        getattr(plain.buffer[a], k).copy_(v)
            fa, fb = factor_only(fused), factor_only(plain)          # identical parameters: old == new, both factors are 1 up to rounding
            with torch.no_grad():                                    # ... so compare them after ONE agent's parameters moved in both
                for r in (fused, plain):
                    for q in r.policy[0].actor.act.action_out.fc_mean.parameters():
                        q.add_(1e-3)
            new_f = fused.grouped.evaluate_actions([_rows(fused.buffer[0].obs[:-1])], [_rows(fused.buffer[0].actions)], agents=[0])[0]
            new_p = plain._module_logp(0)
            rel = float((new_f - new_p).abs().max() / new_p.abs().max())
            fac = timed({"modules": lambda: factor_only(plain), "fused": lambda: factor_only(fused)}, max(args.calls, 2), args.warmup)
            trn = timed({"modules": plain.train, "fused": fused.train}, args.calls, args.warmup)
            emit({"bench": "marl_runner", "algo": algo, "envs": n, "rows": 8 * n, "agents": fused.num_agents, "hidden": 512, "rounds": args.rounds,
                  "calls": args.calls, "eval_route": fused.grouped.eval_route, "train_modules_ms": win(trn["modules"]), "train_fused_ms": win(trn["fused"]),
                  "train_speedup_median": round(trn["modules"][0] / trn["fused"][0], 3), "train_verdict": verdict(trn["modules"], trn["fused"]),
                  "factor_modules_ms": win(fac["modules"]), "factor_fused_ms": win(fac["fused"]),
                  "factor_speedup_median": round(fac["modules"][0] / fac["fused"][0], 3), "factor_verdict": verdict(fac["modules"], fac["fused"]),
                  "factor_share_of_train_modules": round(fac["modules"][0] / trn["modules"][0], 4), "max_rel_diff_logp_routes": rel,
                  "factor_noop_max_dev_fused": float((fa - 1).abs().max()), "factor_noop_max_dev_modules": float((fb - 1).abs().max())})
            del fused, plain
        del env
        torch.cuda.empty_cache()

    # the kernel alone
    M, G, H, A = args.kernel_rows, 10, 512, 8
    L, idx, stream = _lib.for_device(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    i32 = lambda v: (ctypes.c_int32 * G)(*([v] * G))
    h, gam, bet = [rnd(M, H) for _ in range(G)], [1 + 0.1 * rnd(H) for _ in range(G)], [0.1 * rnd(H) for _ in range(G)]
    w, b, sd = [rnd(A, H) / H ** 0.5 for _ in range(G)], [0.1 * rnd(A) for _ in range(G)], [0.3 + 0.1 * torch.rand(A, device=dev) for _ in range(G)]
    act, old, lp, fac = [0.5 * rnd(M, A) for _ in range(G)], [rnd(M, A) - 1 for _ in range(G)], [rnd(M, A) for _ in range(G)], [torch.ones(M, device=dev) for _ in range(G)]

    fin = [0.5 + torch.rand(M, device=dev, generator=g) for _ in range(G)]

    def kernel(with_factor):
        _lib.check(L.mms_marl_heads_eval(idx, G, M, H, tab(h), tab(gam), tab(bet), tab(w), tab(b), i32(A), tab(sd), tab(act), None, tab(lp), None,
                                         tab(old) if with_factor else None, None, tab(fin) if with_factor else None, tab(fac) if with_factor else None, 1e-5,
                                         stream), None, "mms_marl_heads_eval", L)
    k = timed({"logp": lambda: kernel(False), "logp_factor": lambda: kernel(True)}, 20, 3)
    emit({"bench": "marl_heads_eval_kernel", "rows": M, "networks": G, "hidden": H, "actions": A, "rounds": args.rounds, "calls": 20,
          "logp_us": win(tuple(1e3 * v for v in k["logp"])),
          "logp_factor_us": win(tuple(1e3 * v for v in k["logp_factor"])),
          "h_read_GBps_logp_factor_median": round(G * M * H * 4 / (k["logp_factor"][0] * 1e-3) / 1e9, 1)})


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The MAPPO / HAPPO update at the workload's shapes: one agent's rollout of episode_length 8 in an agent view of SharedRolloutBuffers
(TenAnt: 4096 envs x 10 agents, obs 46 / share_obs 388 / 8 actions, 32768 rows per minibatch; `--shape swarm`: 2048 envs x 100 agents,
share_obs 3808, 16384 rows), actor and critic of hidden 512, layer_N 2 (tests/marl_modules.py), the shipped flags (PopArt, Huber with
delta 10, clipped value loss, masks off; ppo_epoch 5, num_mini_batch 1), a synthetic rollout.

  (a) `head`: the loss head alone, forward and backward, on the same mu / std / value: `fused` = marl_ppo_loss with the minibatch's
      index vector over the buffer's own strided tensors (mms_marl_ppo_loss: two launches) + autograd.grad; `torch` = the gathers of
      feed_forward_generator, marl_ppo_loss_torch on the gathered rows + autograd.grad.  Host time per call around a synchronise.
  (b) `train`: a whole train(buffer) of one agent (5 updates: gathers, both networks forward and backward, the loss, two clips, two
      Adam steps, the normaliser): the trainer as it is against the same trainer with loss_fn = marl_ppo_loss_torch.
  (c) the kernel times come from a run of their own: `rocprofv3 --kernel-trace --stats -- python tools/bench_marl_update.py
      --kernels-only` (a few fused head calls and nothing else).

Warm-up of every path, then five rounds alternating the paths; per path the median, every round and max - min (the run-to-run spread
the comparison is read against).  One JSON line per shape, appended to profiles/marl_loss_bench.jsonl.

    python tools/bench_marl_update.py [--shape tenant|swarm] [--algo mappo|happo] [--reps 100]
"""
import argparse
import copy
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"tenant": dict(num_envs=4096, agents=10, share_obs=388), "swarm": dict(num_envs=2048, agents=100, share_obs=3808)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="tenant")
    ap.add_argument("--algo", choices=("mappo", "happo"), default="mappo")
    ap.add_argument("--num-envs", type=int, default=None, help="override the shape's env count (a rehearsal)")
    ap.add_argument("--reps", type=int, default=100, help="head calls per timed window")
    ap.add_argument("--train-reps", type=int, default=4, help="train() calls per timed window")
    ap.add_argument("--kernels-only", action="store_true", help="a few fused head calls and nothing else: the run to put under rocprofv3")
    ap.add_argument("--device", default="cuda:0", help="\"cpu\": a rehearsal on the CPU build (wall-clock windows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marl_loss_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import marl_modules as mm
    from massive_marl_benchmark_amd.algorithms.marl.loss import marl_ppo_loss, marl_ppo_loss_torch
    from massive_marl_benchmark_amd.algorithms.marl.trainer import HAPPO, MAPPO
    from massive_marl_benchmark_amd.algorithms.marl.utils.shared_buffer import SharedRolloutBuffers

    shape = SHAPES[args.shape]
    dev = torch.device(args.device)
    gpu = dev.type == "cuda"
    N, G, SD = args.num_envs or shape["num_envs"], shape["agents"], shape["share_obs"]
    T, OD, A, H, k = 8, 46, 8, 512, 3
    M = T * N
    config = {"clip_param": 0.2, "ppo_epoch": 5, "num_mini_batch": 1, "data_chunk_length": 10, "value_loss_coef": 1.0, "entropy_coef": 0.01,
              "max_grad_norm": 10.0, "huber_delta": 10.0, "use_valuenorm": False, "use_popart": True, "use_recurrent_policy": False,
              "use_naive_recurrent_policy": False, "use_max_grad_norm": True, "use_clipped_value_loss": True, "use_huber_loss": True,
              "use_value_active_masks": False, "use_policy_active_masks": False, "episode_length": T, "n_rollout_threads": N, "hidden_size": H,
              "recurrent_N": 1, "gamma": 0.99, "gae_lambda": 0.95, "use_gae": True, "use_proper_time_limits": False}
    torch.manual_seed(0)
    env = types.SimpleNamespace(num_agents=G, num_observations=OD, nums_share_observations=SD, action_space=[types.SimpleNamespace(shape=(A,))] * G)
    config_small_rnn = dict(config, hidden_size=1)                    # the rnn state tensors are not part of this path: keep them small
    buf = SharedRolloutBuffers(config_small_rnn, env, dev).agents[k]

    def policy():
        torch.manual_seed(1)
        p = types.SimpleNamespace(actor=mm.Actor(OD, A, hidden=H, layer_N=2).to(dev), critic=mm.Critic(SD, hidden=H, layer_N=2).to(dev))
        p.actor_optimizer = torch.optim.Adam(p.actor.parameters(), lr=5e-4, eps=1e-5)
        p.critic_optimizer = torch.optim.Adam(p.critic.parameters(), lr=5e-4, eps=1e-5)
        return p

    pol = policy()
    with torch.no_grad():                                             # a rollout as the collect loop leaves it, then a few steps' worth of drift
        buf.share_obs.normal_()
        buf.obs.copy_(torch.randn(T + 1, N, OD, device=dev))
        rows = lambda x: x.reshape(-1, *x.shape[2:])
        mu0, std0, v0 = mm.torch_forward(pol.actor, pol.critic, rows(buf.obs[:-1]), rows(buf.share_obs[:-1]))
        act = mu0 + std0 * torch.randn_like(mu0)
        buf.actions.copy_(act.view(T, N, A))
        buf.action_log_probs.copy_((mm.log_prob(mu0, std0, act) + 0.1 / A ** 0.5 * torch.randn_like(mu0)).view(T, N, A))
        buf.value_preds[:-1].copy_((v0 + 0.3 * torch.randn_like(v0)).view(T, N, 1))
        buf.returns[:-1].copy_((v0 + torch.randn_like(v0)).view(T, N, 1))
        buf.factor.copy_(torch.exp(0.1 * torch.randn(T, N, 1, device=dev)))
    adv = torch.randn(T, N, 1, device=dev)
    indices = torch.randperm(M, device=dev)
    mu = mu0.clone().requires_grad_(True)
    std = std0.clone().requires_grad_(True)
    value = v0.clone().requires_grad_(True)
    nm, nv = torch.tensor([0.1], device=dev), torch.tensor([1.3], device=dev)
    happo = args.algo == "happo"
    kw = dict(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, huber_delta=10.0, use_huber_loss=True, use_clipped_value_loss=True, norm_mean=nm, norm_var=nv)

    def head_fused():
        obj, info = marl_ppo_loss(mu, std, value, buf.actions, buf.action_log_probs, adv, buf.value_preds, buf.returns, None,
                                  buf.factor if happo else None, indices=indices, **kw)
        return (obj, info["ratio"]) + torch.autograd.grad(obj, (mu, std, value))

    def head_torch():                                                 # feed_forward_generator's gathers, then the expression
        pick = lambda x, drop_last: rows(x[:-1] if drop_last else x)[indices]
        fields = (pick(buf.actions, False), pick(buf.action_log_probs, False), adv.reshape(-1, 1)[indices], pick(buf.value_preds, True),
                  pick(buf.returns, True), pick(buf.active_masks, True), pick(buf.factor, False) if happo else None)
        obj, info = marl_ppo_loss_torch(mu, std, value, *fields, **kw)
        return (obj, info["ratio"]) + torch.autograd.grad(obj, (mu, std, value))

    def clock():
        if gpu:
            torch.cuda.synchronize()
        return time.perf_counter()

    if args.kernels_only:
        for _ in range(20):
            head_fused()
        clock()
        print("kernels-only: 20 fused head calls at %d x %d" % (M, A))
        return

    trainers = {}
    for name in ("fused", "torch"):
        t = (HAPPO if happo else MAPPO)(config, policy(), dev)
        if name == "torch":
            t.loss_fn = marl_ppo_loss_torch
        t.prep_training()
        trainers[name] = t

    out = {"bench": "marl_update", "device": torch.cuda.get_device_name(0) if gpu else "cpu", "shape": args.shape, "algo": args.algo, "num_envs": N, "agents": G,
           "episode_length": T, "rows": M, "actions": A, "hidden": H, "layer_N": 2, "share_obs": SD, "ppo_epoch": config["ppo_epoch"],
           "num_mini_batch": config["num_mini_batch"], "head_calls_per_round": args.reps, "train_calls_per_round": args.train_reps,
           # what mms_marl_ppo_loss must move per row: mu, actions, old_logp in and dmu out (4 A each); the index (8), value, adv, value_preds, returns in, dvalue out
           "kernel_bytes": M * (16 * A + 8 + 20 + (4 if happo else 0))}
    groups = (("head", {"fused": head_fused, "torch": head_torch}, args.reps),
              ("train", {n: (lambda t=t: tuple(torch.as_tensor(float(v)) for v in t.train(buf).values())) for n, t in trainers.items()}, args.train_reps))
    for group, paths, reps in groups:
        res, last = {n: [] for n in paths}, {}
        for f in paths.values():
            for _ in range(3):
                f()
        for _ in range(5):
            for n, f in paths.items():
                t0 = clock()
                for _ in range(reps):
                    last[n] = f()
                res[n].append(1e3 * (clock() - t0) / reps)
        for n, v in res.items():
            out["%s_%s_ms_per_call" % (group, n)] = float(np.median(v))
            out["%s_%s_ms_rounds" % (group, n)] = v
            out["%s_%s_ms_spread" % (group, n)] = float(max(v) - min(v))
        out[group + "_speedup_fused"] = out[group + "_torch_ms_per_call"] / out[group + "_fused_ms_per_call"]
        out[group + "_finite"] = bool(all(torch.isfinite(t).all() for v in last.values() for t in v))
        if group == "head":
            out["head_max_diff_vs_torch"] = [float((a.detach().double() - b.detach().double()).abs().max() / (1e-30 + b.detach().double().abs().max()))
                                             for a, b in zip(last["fused"], last["torch"])]
    out["train_ms_per_update_fused"] = out["train_fused_ms_per_call"] / (config["ppo_epoch"] * config["num_mini_batch"])
    out["train_ms_per_update_torch"] = out["train_torch_ms_per_call"] / (config["ppo_epoch"] * config["num_mini_batch"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

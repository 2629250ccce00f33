#!/usr/bin/env python3
"""SAC's policy loss with the actor's head differentiated by this build (`fused_grad=True`: mms_sac_heads_act forward,
mms_sac_heads_grad + three library products backward) against the same modules with `fused_grad=False` (torch_forward + autograd: the
parent path), in one process on the HIP device.  cfg/sac/config.yaml's shapes: W = 52 observations, A = 24 actions, hidden 3 x 1024
ELU, a minibatch of 8 ring rows x 8192 envs = 65536 rows.

  head      the head forward + backward from a given `hidden` [65536, 1024] that requires a gradient: a, logp = head(hidden);
            (alpha logp - a.sum(-1, keepdim)).mean().backward() -- grad_hidden, both weight and both bias gradients
  loss_pi   compute_loss_pi forward + backward (sac.py:392-403 restated): the actor, two frozen critics, the min and the mean
  update    one whole minibatch update (sac.py:325-359 restated): the Q loss and step, the frozen-critic policy loss and step, both
            gradient clips, the polyak loop

After warm-up, `--rounds` rounds alternating the two sides, each `--reps` calls between two device events; per side the median with
min and max.  The two sides hold equal parameters at the start and draw different noise (the counter stream against torch.randn), so
`update` times two trajectories of the same cost, not the same numbers.  One JSON line per series on stdout, appended to --out.

    python tools/bench_sac_update.py [--series head,loss_pi,update] [--envs 8192] [--reps 20] [--rounds 5] [--out profiles/sac_pi_loss_bench.jsonl]
"""
import argparse
import copy
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", default="head,loss_pi,update")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--ring-rows", type=int, default=8)
    ap.add_argument("--hidden", default="1024,1024,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="\"cpu\": a rehearsal on the CPU build (wall-clock windows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_pi_loss_bench.jsonl"))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("bench_sac_update.py: at least 5 rounds")
    import numpy as np
    import torch
    import torch.nn as nn
    from massive_marl_benchmark_amd import spaces
    from massive_marl_benchmark_amd.algorithms.rl.sac import MLPActorCritic
    dev = torch.device(args.device)
    gpu = dev.type == "cuda"
    if gpu and not torch.cuda.is_available():
        sys.exit("bench_sac_update.py needs a HIP device (or --device cpu for a rehearsal)")
    W, A, hidden = 52, 24, [int(h) for h in args.hidden.split(",")]
    rows, envs = args.ring_rows, args.envs
    alpha, gamma, polyak, max_grad_norm, lr = 0.2, 0.99, 0.995, 1.0, 3e-4
    summary = lambda ts: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    def emit(res):
        res.update(device=torch.cuda.get_device_name(0) if gpu else "cpu", shape=[rows, envs, W], actions=A, hidden=hidden, reps=args.reps,
                   rounds=args.rounds, unit="ms per call: median (min - max) over the rounds")
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def alternate(paths, reps, warm=3):
        for f in paths.values():
            for _ in range(warm):
                f()
        if gpu:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        res = {k: [] for k in paths}
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

    def make(flag):
        torch.manual_seed(0)
        ac = MLPActorCritic(spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-np.ones(A), np.ones(A)), hidden_sizes=hidden,
                            activation=nn.ELU, seed=1, fused_grad=flag).to(dev)
        ac.pi.reserve_counters(rows * envs, dev)
        return ac

    g = torch.Generator().manual_seed(1)
    data = {"obs": torch.randn(rows, envs, W, generator=g).to(dev), "act": (torch.rand(rows, envs, A, generator=g) * 2 - 1).to(dev),
            "r": torch.randn(rows, envs, 1, generator=g).to(dev), "obs2": torch.randn(rows, envs, W, generator=g).to(dev),
            "done": (torch.rand(rows, envs, 1, generator=g) < 0.01).float().to(dev)}
    sides = {"fused_grad": make(True), "torch": make(False)}

    def compute_loss_pi(ac, data):                               # sac.py:392-403
        o = data["obs"]
        pi, logp_pi = ac.pi(o)
        q_pi = torch.min(ac.q1(o, pi), ac.q2(o, pi))
        return (alpha * logp_pi - q_pi).mean()

    def compute_loss_q(ac, targ, data):                          # sac.py:367-389
        o, a, r, o2, d = data["obs"], data["act"], data["r"], data["obs2"], data["done"]
        q1, q2 = ac.q1(o, a), ac.q2(o, a)
        with torch.no_grad():
            a2, logp_a2 = ac.pi(o2)
            q_pi_targ = torch.min(targ.q1(o2, a2), targ.q2(o2, a2))
            backup = r + gamma * (1 - d) * (q_pi_targ - alpha * logp_a2)
        return ((q1 - backup) ** 2).mean() + ((q2 - backup) ** 2).mean()

    series = args.series.split(",")
    if "head" in series:
        paths = {}
        for name, ac in sides.items():
            pi = ac.pi
            with torch.no_grad():
                hid = pi.net(data["obs"].reshape(-1, W))
            hid.requires_grad_(True)
            # the head alone: `net` replaced by the identity, so hidden is the module's input
            head = copy.copy(pi)
            head._modules = dict(pi._modules, net=nn.Identity())

            def run(head=head, hid=hid, pi=pi):
                hid.grad = None
                pi.zero_grad(set_to_none=True)
                a, logp = head(hid)
                (alpha * logp - a.sum(-1, keepdim=True)).mean().backward()
            paths[name] = run
        emit({"series": "head", **alternate(paths, args.reps)})
    if "loss_pi" in series:
        paths = {}
        for name, ac in sides.items():
            def run(ac=ac):
                q_params = list(itertools.chain(ac.q1.parameters(), ac.q2.parameters()))
                for p in q_params:
                    p.requires_grad = False
                ac.pi.zero_grad(set_to_none=True)
                compute_loss_pi(ac, data).backward()
                for p in q_params:
                    p.requires_grad = True
            paths[name] = run
        emit({"series": "loss_pi", **alternate(paths, args.reps)})
    if "update" in series:
        paths = {}
        for name, ac in sides.items():
            targ = copy.deepcopy(ac)
            for p in targ.parameters():
                p.requires_grad = False
            q_params = list(itertools.chain(ac.q1.parameters(), ac.q2.parameters()))
            pi_opt, q_opt = torch.optim.Adam(ac.pi.parameters(), lr=lr), torch.optim.Adam(q_params, lr=lr)

            def run(ac=ac, targ=targ, q_params=q_params, pi_opt=pi_opt, q_opt=q_opt):     # sac.py:325-359
                q_opt.zero_grad()
                compute_loss_q(ac, targ, data).backward()
                nn.utils.clip_grad_norm_(ac.parameters(), max_grad_norm)
                q_opt.step()
                for p in q_params:
                    p.requires_grad = False
                pi_opt.zero_grad()
                compute_loss_pi(ac, data).backward()
                nn.utils.clip_grad_norm_(ac.parameters(), max_grad_norm)
                pi_opt.step()
                for p in q_params:
                    p.requires_grad = True
                with torch.no_grad():
                    for p, p_targ in zip(ac.parameters(), targ.parameters()):
                        p_targ.data.mul_(polyak)
                        p_targ.data.add_((1 - polyak) * p.data)
            paths[name] = run
        emit({"series": "update", **alternate(paths, max(1, args.reps // 4))})


if __name__ == "__main__":
    main()

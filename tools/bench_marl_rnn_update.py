#!/usr/bin/env python3
"""The recurrent MAPPO update at TenAnt's shapes (obs 46, share_obs 388, 8 actions, hidden 512, layer_N 2, recurrent_N 1,
data_chunk_length 10; modules of tests/marl_rnn_modules.py) on the HIP device: the trainers' opt-in `fused_rnn_update` route
(algorithms/marl/rnn_seq.py: mms_gru_gates_group forward, mms_gru_gates_grad_group backward, every product on the library) against the
default torch route (RNNLayer's sequence branch: a host read of the masks, one nn.GRU call per piece, torch's backward through time),
both measured in this process.  Per number of sequences N in a minibatch (T * N rows; default 80 -- the configs' rollout threads -- and
4096) and per mask pattern (`none`: no resets, one piece; `resets`: each mask zero with probability 0.05, so nearly every step starts a
piece), in alternating rounds (torch, fused, torch, ...), each round `--calls` passes between two host-clock reads that end in a device
synchronise, after warm-up passes of the same shape; reported as the median round with (min - max), in ms per pass:

  rnn_*_ms      actor.rnn and critic.rnn (RNNLayer: GRU + LayerNorm) forward on [T * N, 512] features + backward of a weighted sum of
                their outputs: `torch` the modules' own forward one after the other, `fused` gru_sequence for both in grouped calls + norm
  update_*_ms   one whole MAPPO.ppo_update (bases, RNN, heads, mms_marl_ppo_loss, backward, clip, Adam step) on a gathered sample, with
                the config key off and on

`verdict` compares the two windows: "faster" / "slower" when they do not overlap, else "no result at that size".  The worst
difference of the two routes' outputs is printed as a check that they compute the same thing.  One JSON line per (N, masks) on stdout
(and appended to --out when given).

    python tools/bench_marl_rnn_update.py [--seqs 80,4096] [--rounds 5] [--calls 10] [--out profiles/marl_rnn_update_bench.jsonl]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OBS, SOBS, ACT, H, LAYER_N, R, T = 46, 388, 8, 512, 2, 1, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="80,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import marl_loss_check as mlc
    import marl_modules as mm
    import marl_rnn_modules as rm
    from massive_marl_benchmark_amd.algorithms.marl import trainer as tr
    from massive_marl_benchmark_amd.algorithms.marl.rnn_seq import gru_sequence
    if not torch.cuda.is_available():
        sys.exit("bench_marl_rnn_update.py needs a HIP device")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(1)
    torch.manual_seed(1)
    actor, critic = rm.Actor(OBS, ACT, H, LAYER_N, R), rm.Critic(SOBS, H, LAYER_N, R)
    for m in (actor, critic):
        mm.randomize(m, gen)
        m.to(dev).train()

    class Policy:
        def __init__(self):
            self.actor, self.critic = copy.deepcopy(actor), copy.deepcopy(critic)
            self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=5e-4, eps=1e-5)
            self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=5e-4, eps=1e-5)

    def timed(fns):
        """fns: {name: callable}; alternating rounds; {name: (median, min, max)} in ms per pass"""
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

    def verdict(torch_w, fused_w):
        if fused_w[2] < torch_w[1]:
            return "faster"
        if fused_w[1] > torch_w[2]:
            return "slower"
        return "no result at that size"

    for N in [int(v) for v in args.seqs.split(",")]:
        for pattern in ("none", "resets"):
            g = torch.Generator(device=dev).manual_seed(N)
            rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
            rows = T * N
            masks = torch.ones(rows, 1, device=dev) if pattern == "none" else (torch.rand(rows, 1, device=dev, generator=g) > 0.05).float()
            pieces = 1 + int((masks.view(T, N)[1:] == 0).any(1).sum())
            fa, fc = rnd(rows, H), rnd(rows, H)
            ha, hc = torch.tanh(rnd(N, R, H)), torch.tanh(rnd(N, R, H))
            wa, wc = rnd(rows, H), rnd(rows, H)
            seen = {}

            def rnn_torch():
                xa, xc = fa.clone().requires_grad_(), fc.clone().requires_grad_()
                ya, yc = actor.rnn(xa, ha, masks)[0], critic.rnn(xc, hc, masks)[0]
                ((ya * wa).sum() + (yc * wc).sum()).backward()
                seen["torch"] = (ya.detach(), xa.grad)

            def rnn_fused():
                xa, xc = fa.clone().requires_grad_(), fc.clone().requires_grad_()
                (ya, _), (yc, _) = gru_sequence([xa, xc], [ha, hc], masks, [actor.rnn.rnn, critic.rnn.rnn])
                ya, yc = actor.rnn.norm(ya), critic.rnn.norm(yc)
                ((ya * wa).sum() + (yc * wc).sum()).backward()
                seen["fused"] = (ya.detach(), xa.grad)

            config = mlc.trainer_config(use_recurrent_policy=True, data_chunk_length=T, hidden_size=H, recurrent_N=R)
            trainers = {"torch": tr.MAPPO(config, Policy(), dev), "fused": tr.MAPPO(dict(config, fused_rnn_update=True), Policy(), dev)}
            with torch.no_grad():
                mu, std, v, _, _ = rm.torch_forward(actor, critic, rnd(rows, OBS), rnd(rows, SOBS), ha, hc, masks)
            obs, sobs = rnd(rows, OBS), rnd(rows, SOBS)
            act = mu + std * rnd(rows, ACT)
            sample = (sobs, obs, ha, hc, act, v + 0.3 * rnd(rows, 1), v + rnd(rows, 1), masks, torch.ones(rows, 1, device=dev),
                      mm.log_prob(mu, std, act) + 0.1 * rnd(rows, ACT), rnd(rows, 1), None, None)
            rnn = timed({"torch": rnn_torch, "fused": rnn_fused})
            diff = [float((a - b).abs().max()) for a, b in zip(seen["torch"], seen["fused"])]
            upd = timed({k: (lambda t=t: t.ppo_update(sample)) for k, t in trainers.items()})
            win = lambda w: {"median": round(w[0], 3), "min": round(w[1], 3), "max": round(w[2], 3)}
            res = {"bench": "marl_rnn_update", "seqs": N, "T": T, "rows": rows, "hidden": H, "recurrent_N": R, "masks": pattern, "pieces": pieces,
                   "rounds": args.rounds, "calls": args.calls,
                   "rnn_torch_ms": win(rnn["torch"]), "rnn_fused_ms": win(rnn["fused"]), "rnn_speedup_median": round(rnn["torch"][0] / rnn["fused"][0], 3),
                   "rnn_verdict": verdict(rnn["torch"], rnn["fused"]),
                   "update_torch_ms": win(upd["torch"]), "update_fused_ms": win(upd["fused"]), "update_speedup_median": round(upd["torch"][0] / upd["fused"][0], 3),
                   "update_verdict": verdict(upd["torch"], upd["fused"]), "max_abs_diff_y": diff[0], "max_abs_diff_dx": diff[1]}
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The recurrent MAPPO collect pass at TenAnt's shapes (10 agents, obs 46, share_obs 388, 8 actions, hidden 512, layer_N 2,
recurrent_N 1; modules of tests/marl_rnn_modules.py) on the HIP device, per number of envs (default 4096, and the configs' 80 rollout
threads).  Timed in alternating rounds (grouped, per-agent, grouped, ...), each round `--calls` passes between two host-clock reads that
end in a device synchronise, after warm-up passes of the same shape; reported as the median round with (min - max), in ms per pass:

  grouped_ms     GroupedPolicyInference.get_actions: every stage once for all 20 networks, the GRU step as one mms_gru_group launch,
                 the new states written into the next slot of an [T + 1, N, agents, recurrent_N, H] rollout tensor in place
  per_agent_ms   the reference's way and the baseline (runner.py:205-217): agent by agent Actor.forward (base, RNNLayer, DiagGaussian
                 sample and log-probability) and Critic.forward of the same modules in torch, states copied into the slot
  gru_us         mms_gru_group alone (20 groups, K = H = 512, masks on, both destinations): `--calls` back-to-back launches between two
                 device events, with the TFLOP/s on 12 M H^2 flop per network

Both paths start from the same states; the worst difference of their values is printed as a check that they compute the same thing.
One JSON line per envs value on stdout (and appended to --out when given).

    python tools/bench_marl_rnn.py [--envs 4096,80] [--rounds 5] [--calls 20] [--out profiles/marl_rnn_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, OBS, SOBS, ACT, H, LAYER_N, R = 10, 46, 388, 8, 512, 2, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,80")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import marl_modules as mm
    import marl_rnn_modules as rm
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.algorithms.marl.policy_inference import GroupedPolicyInference
    if not torch.cuda.is_available():
        sys.exit("bench_marl_rnn.py needs a HIP device")
    dev = "cuda:0"
    L, idx, stream = _lib.for_device(dev)
    gen = torch.Generator().manual_seed(1)
    torch.manual_seed(1)
    actors = [rm.Actor(OBS, ACT, H, LAYER_N, R) for _ in range(N)]
    critics = [rm.Critic(SOBS, H, LAYER_N, R) for _ in range(N)]
    for m in actors + critics:
        mm.randomize(m, gen)
        m.to(dev).eval()
    grouped = GroupedPolicyInference(actors, critics, seed=3)

    for envs in [int(v) for v in args.envs.split(",")]:
        g = torch.Generator(device=dev).manual_seed(envs)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
        obs, sobs = rnd(envs, N, OBS), rnd(envs, SOBS)
        states = torch.tanh(rnd(2, envs, N, R, H))                        # slot 0: in, slot 1: out (actor)
        states_c = torch.tanh(rnd(2, envs, N, R, H))
        masks = (torch.rand(envs, 1, device=dev, generator=g) > 0.05).float()
        values, actions, logp = torch.empty(envs, N), torch.empty(envs, N, ACT), torch.empty(envs, N, ACT)
        values, actions, logp = values.to(dev), actions.to(dev), logp.to(dev)
        kw = dict(rnn_states=[states[0][:, k] for k in range(N)], rnn_states_critic=[states_c[0][:, k] for k in range(N)], masks=[masks] * N,
                  rnn_out=([states[1][:, k] for k in range(N)], [states_c[1][:, k] for k in range(N)]),
                  out=([values[:, k:k + 1] for k in range(N)], [actions[:, k] for k in range(N)], [logp[:, k] for k in range(N)]))
        sobs_l, obs_l = [sobs] * N, [obs[:, k] for k in range(N)]

        def run_grouped():
            grouped.get_actions(sobs_l, obs_l, **kw)

        @torch.no_grad()
        def run_per_agent():
            for k in range(N):
                a, c = actors[k], critics[k]
                fa, new_a = a.rnn(mm.base_forward(a.base, obs[:, k]), states[0][:, k], masks)
                fc, new_c = c.rnn(mm.base_forward(c.base, sobs), states_c[0][:, k], masks)
                hd = a.act.action_out
                dist = torch.distributions.Normal(hd.fc_mean(fa), torch.sigmoid(hd.log_std / hd.std_x_coef) * hd.std_y_coef)
                act = dist.sample()
                actions[:, k].copy_(act)
                logp[:, k].copy_(dist.log_prob(act))
                values[:, k:k + 1].copy_(c.v_out(fc))
                states[1][:, k].copy_(new_a)
                states_c[1][:, k].copy_(new_c)

        def a_round(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.calls

        for fn in (run_grouped, run_per_agent):
            for _ in range(3):
                fn()
        run_grouped()
        torch.cuda.synchronize()
        v_grouped, s_grouped = values.clone(), states[1].clone()
        run_per_agent()
        torch.cuda.synchronize()
        agree = {"values_max_diff": float((values - v_grouped).abs().max()), "states_max_diff": float((states[1] - s_grouped).abs().max())}
        ts = {"grouped_ms": [], "per_agent_ms": []}
        for _ in range(args.rounds):
            ts["grouped_ms"].append(a_round(run_grouped))
            ts["per_agent_ms"].append(a_round(run_per_agent))
        stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res = {"bench": "marl_rnn", "agents": N, "obs": OBS, "share_obs": SOBS, "act": ACT, "hidden": H, "layer_N": LAYER_N, "recurrent_N": R, "envs": envs,
               "rounds": args.rounds, "calls": args.calls, "device": torch.cuda.get_device_name(0), "agree": agree}
        res.update({k: stat(v) for k, v in ts.items()})
        res["speedup_median"] = round(res["per_agent_ms"]["median"] / res["grouped_ms"]["median"], 3)

        # the kernel alone
        G, M = 2 * N, envs
        tab = lambda ts_: (ctypes.c_void_p * len(ts_))(*[t.data_ptr() for t in ts_])
        x = [rnd(M, H) for _ in range(G)]
        h_in, h_out, y = torch.tanh(rnd(G, M, R, H)), torch.empty(G, M, R, H, device=dev), torch.empty(G, M, H, device=dev)
        wi, wh = [rnd(3 * H, H) * H ** -0.5 for _ in range(G)], [rnd(3 * H, H) * H ** -0.5 for _ in range(G)]
        bi, bh = [rnd(3 * H) * 0.1 for _ in range(G)], [rnd(3 * H) * 0.1 for _ in range(G)]
        args_ = (idx, G, M, H, H, tab(x), H, tab(list(h_in.unbind(0))), R * H, tab([masks] * G), 1, tab(wi), tab(wh), tab(bi), tab(bh),
                 tab(list(h_out.unbind(0))), R * H, tab(list(y.unbind(0))), stream)
        us = []
        for _ in range(args.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                _lib.check(L.mms_gru_group(*args_), None, "mms_gru_group", L)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000 / args.calls)
        us = us[1:]                                                          # (the first round is the warm-up)
        med = statistics.median(us)
        res["gru_us"] = {"median": round(med, 2), "min": round(min(us), 2), "max": round(max(us), 2), "TFLOPs": round(12.0 * G * M * H * H / med / 1e6, 2)}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del x, h_in, h_out, y, wi, wh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

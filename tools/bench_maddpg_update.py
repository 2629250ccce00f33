#!/usr/bin/env python3
"""MADDPG at TenAnt's shapes (10 agents, obs 46, share_obs 388, act 8, hidden [1024, 1024, 512], a minibatch of 16 ring rows) on the
HIP device, per number of envs (default 4096, and the config's 80 rollout threads).  Timed, each after warm-up calls of the same
shape, as the median of `--repeats` host-clock windows that end in a device synchronise (min and max alongside):

  collect_ms        one collection step: MADDPG.act_all with exploration noise into ring rows (M = envs)
  update_fused_ms   one ddpg_update, fused=True (M = 16 * envs)
  update_torch_ms   the same modules with fused=False, which is the reference's evaluation: per-agent loops, N^2 target forwards,
                    N (N - 1) discarded actor backward passes, plain torch -- the yardstick; it runs none of this project's kernels
  head_us / qtail_us   mms_det_heads_act_group (10 groups, H = 512, A = 8, noise on, act and joint destinations) and
                    mms_q_heads_backup_group (10 groups, H = 512) alone at M = 16 * envs: 100 back-to-back calls between two device
                    events after 10 warm-up calls, with the TB/s on the bytes each must move (4 G M H in)

Both updates start from the same parameters and samples; their first value losses are printed as a check that they compute the same
thing.  One JSON line per envs value on stdout (and appended to --out when given).

    python tools/bench_maddpg_update.py [--envs 4096,80] [--repeats 5] [--out profiles/maddpg_update_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, OBS, SOBS, ACT, HIDDEN, ROWS = 10, 46, 388, 8, [1024, 1024, 512], 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,80")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.algorithms.marl.maddpg import MADDPG, MADDPG_policy
    if not torch.cuda.is_available():
        sys.exit("bench_maddpg_update.py needs a HIP device")
    dev = "cuda:0"
    L, idx, stream = _lib.for_device(dev)
    config = {"learning_rate": 5e-4, "hidden_size": HIDDEN, "activation": "elu", "act_noise": 0.1, "num_learning_epochs": 2, "num_mini_batch": 1,
              "gamma": 0.96, "polyak": 0.995, "max_grad_norm": 1.0}
    o, s = types.SimpleNamespace(shape=(OBS,)), types.SimpleNamespace(shape=(SOBS,))
    a = types.SimpleNamespace(shape=(ACT,), high=np.ones(ACT, np.float32))

    def trainer(fused):
        torch.manual_seed(1)
        policies = [MADDPG_policy(config, o, s, a, [a] * N, device=dev) for _ in range(N)]
        return MADDPG(config, policies, N, device=dev, fused=fused)

    def timed(fn, repeats, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    for envs in [int(v) for v in args.envs.split(",")]:
        M = ROWS * envs
        g = torch.Generator(device=dev).manual_seed(envs)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)

        def padded(*lead):
            base = torch.zeros(*lead, 48, device=dev)
            base[..., :OBS] = rnd(*lead, OBS)
            return base[..., :OBS]
        samples = [{"obs": padded(ROWS, envs), "sobs": rnd(ROWS, envs, SOBS), "jact": torch.tanh(rnd(ROWS, envs, N * ACT)), "r": rnd(ROWS, envs, 1),
                    "obs2": padded(ROWS, envs), "sobs2": rnd(ROWS, envs, SOBS), "done": (torch.rand(ROWS, envs, 1, device=dev, generator=g) < 0.05).to(torch.uint8)}
                   for _ in range(N)]
        dense = [{k: v.contiguous() for k, v in d.items()} for d in samples]          # the yardstick's inputs: dense rows, as the reference gathers them
        res = {"bench": "maddpg_update", "agents": N, "obs": OBS, "share_obs": SOBS, "act": ACT, "hidden": HIDDEN, "ring_rows": ROWS, "envs": envs, "M": M,
               "repeats": args.repeats}
        fused, plain = trainer(True), trainer(False)
        obs_rows = [padded(envs) for _ in range(N)]
        act_slots, joint_slot = [torch.zeros(envs, ACT, device=dev) for _ in range(N)], torch.zeros(envs, N * ACT, device=dev)
        res["collect_ms"] = timed(lambda: fused.act_all(obs_rows, False, act_slots, joint_slot), max(args.repeats, 20), warm=5)
        res["collect_torch_ms"] = timed(lambda: plain.act_all(obs_rows, False, act_slots, joint_slot), max(args.repeats, 20), warm=5)
        first = {}

        def update(t, key):
            v, _ = t.ddpg_update(samples if t.fused else dense)
            first.setdefault(key, v[0].item())
        res["update_fused_ms"] = timed(lambda: update(fused, "fused"), args.repeats)
        res["update_torch_ms"] = timed(lambda: update(plain, "torch"), args.repeats)
        res["first_value_loss"] = first
        del fused, plain

        # the two kernels alone
        H, G = HIDDEN[-1], N
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        hs = [torch.nn.functional.elu(rnd(M, H)) for _ in range(G)]
        ws, bs = [rnd(ACT, H) * H ** -0.5 for _ in range(G)], [rnd(ACT) * 0.1 for _ in range(G)]
        acts, joint = [torch.empty(M, ACT, device=dev) for _ in range(G)], torch.empty(M, G * ACT, device=dev)
        counters = torch.zeros(M, dtype=torch.int64, device=dev)
        lim = (ctypes.c_float * G)(*[1.0] * G)
        qw, qb = [rnd(1, H) * H ** -0.5 for _ in range(G)], [rnd(1) for _ in range(G)]
        r, d, bk = [rnd(M) for _ in range(G)], [torch.zeros(M, dtype=torch.uint8, device=dev) for _ in range(G)], [torch.empty(M, device=dev) for _ in range(G)]

        def head():
            _lib.check(L.mms_det_heads_act_group(idx, G, M, H, ACT, 0, tab(hs), tab(ws), tab(bs), lim, 0.1, 7, p(counters), 0, tab(acts), ACT, p(joint), G * ACT,
                                                 stream), None, "mms_det_heads_act_group", L)

        def qtail():
            _lib.check(L.mms_q_heads_backup_group(idx, G, M, H, tab(hs), tab(qw), tab(qb), None, tab(r), tab(d), 0.96, tab(bk), stream), None,
                       "mms_q_heads_backup_group", L)
        for name, call in (("head_us", head), ("qtail_us", qtail)):
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                call()
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1000 / 100
            res[name] = {"us": round(us, 2), "TBps_in": round(4.0 * G * M * H / us / 1e6, 3)}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del hs, samples, dense
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The TD3 and DDPG learners (algorithms/rl/td3/td3.py, ddpg/ddpg.py) with `fused_update` on and off, in one process on the HIP device,
on MultiIngenuity at 8192 envs with cfg/td3/config.yaml's and cfg/ddpg/config.yaml's update (nsteps 8, noptepochs 5, nminibatches 4,
batch_size 64, policy_delay 2: one Q step and one policy step per epoch on a minibatch of 16 ring rows x 8192 envs = 131072 rows;
replay_size 100 for both -- the ring's length changes no shape that is timed): TD3 at SAC's width, hidden 3 x 1024, and DDPG at the
config's own 3 x 256.

  entries   mms_det_heads_act (smoothing noise and both clamps on, act_out at a W + A pitch and tanh_out) and mms_det_heads_grad (g at a
            W + A pitch, dbias wanted) alone at [131072, H] -> 24 actions, for both widths: the time per call
  update    one `update()` of a learner past its warm-up: the default route (the reference's statements on this package's modules)
            against `fused_update=True`
  run       one `run` iteration (8 env steps, each followed by an `update()`) of the same two learners; writing the checkpoint is
            left out (`save` replaced by a no-op), the log is off

After warm-up, `--rounds` rounds alternating the two sides; `entries` and `update` between two device events, `run` on the host clock
around a call that ends in a device synchronise.  Per side the median with min and max; where the two sides' ranges overlap the line
says "no result".  The two sides start from equal parameters and draw different noise, so `update` and `run` time two trajectories of
the same cost, not the same numbers.  One JSON line per series on stdout, appended to --out.

    python tools/bench_td3_learner.py [--series entries,update,run] [--algos td3,ddpg] [--envs 8192] [--rounds 5] [--out profiles/td3_learner_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = {"td3": 1024, "ddpg": 256}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", default="entries,update,run")
    ap.add_argument("--algos", default="td3,ddpg")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--hidden-layer", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="calls per window of `entries`; `update` takes a tenth of it, `run` one")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="\"cpu\": a rehearsal on the CPU build (wall-clock windows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td3_learner_bench.jsonl"))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("bench_td3_learner.py: at least 5 rounds")
    import torch
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.algorithms.rl.ddpg import DDPG
    from massive_marl_benchmark_amd.algorithms.rl.td3 import TD3
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.vec_task import VecTaskPython
    from massive_marl_benchmark_amd.tasks.multi_ingenuity import MultiIngenuity
    dev = torch.device(args.device)
    gpu = dev.type == "cuda"
    if gpu and not torch.cuda.is_available():
        sys.exit("bench_td3_learner.py needs a HIP device (or --device cpu for a rehearsal)")
    sync = torch.cuda.synchronize if gpu else (lambda: None)
    summary = lambda ts: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    def emit(res):
        res.update(device=torch.cuda.get_device_name(0) if gpu else "cpu", envs=args.envs, rounds=args.rounds)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def verdict(res, a="default", b="fused_update"):
        """`b` against `a`: the ratio of the medians where the two ranges do not overlap, "no result" where they do."""
        if res[a]["min"] <= res[b]["max"] and res[b]["min"] <= res[a]["max"]:
            return "no result (the ranges overlap)"
        return "%s / %s = %.3f" % (b, a, res[b]["median"] / res[a]["median"])

    def alternate(paths, reps, warm=2, events=True):
        for f in paths.values():
            for _ in range(warm):
                f()
        sync()
        if gpu:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        res = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, f in paths.items():
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

    series, algos = args.series.split(","), args.algos.split(",")
    W, A = 52, 24                                   # MultiIngenuity's observation and action widths
    if "entries" in series:
        M = 16 * args.envs
        L, idx, stream = _lib.for_device(dev)
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        for H in sorted({WIDTHS[a] for a in algos}):
            g = torch.Generator().manual_seed(1)
            h = torch.relu(torch.randn(M, H, generator=g)).to(dev)
            w, b = (torch.randn(A, H, generator=g) * H ** -0.5).to(dev), torch.zeros(A, device=dev)
            block, t_out = torch.empty(M, W + A, device=dev), torch.empty(M, A, device=dev)
            counters = torch.zeros(M, dtype=torch.int64, device=dev)
            gblock, dy, dbias = torch.randn(M, W + A, generator=g).to(dev), torch.empty(M, A, device=dev), torch.empty(A, device=dev)
            n = ctypes.c_int64(-1)

            def act():
                _lib.check(L.mms_det_heads_act(idx, M, H, A, p(h), p(w), p(b), 1.0, 0.2, 0.5, 7, p(counters), 0, p(block[:, W:]), W + A, p(t_out), stream), None,
                           "mms_det_heads_act", L)

            def grad(ws):
                _lib.check(L.mms_det_heads_grad(idx, M, A, 1.0, p(t_out), p(gblock[:, W:]), W + A, p(dy), p(dbias), ws, ctypes.byref(n), stream), None,
                           "mms_det_heads_grad", L)
            grad(None)
            buf = torch.empty(n.value + 256, dtype=torch.uint8, device=dev)
            ws = ctypes.c_void_p(buf.data_ptr() + (-buf.data_ptr()) % 256)
            res = alternate({"det_heads_act": act, "det_heads_grad": lambda: grad(ws)}, args.reps)
            res["det_heads_act"]["bytes_needed"] = 4 * (M * H + A * H + A + 2 * M * A) + 16 * M
            res["det_heads_grad"]["bytes_needed"] = 4 * 3 * M * A
            for k in ("det_heads_act", "det_heads_grad"):
                res[k]["achieved_TB_per_s"] = round(res[k]["bytes_needed"] / (res[k]["median"] * 1e-3) / 1e12, 3)
            emit({"series": "entries", "rows": M, "H": H, "A": A, "unit": "ms per call (every launch of the entry): median (min - max) over the rounds", **res})

    if "update" in series or "run" in series:
        for algo in algos:
            cls, H = {"td3": TD3, "ddpg": DDPG}[algo], WIDTHS[algo]
            learn = dict(hidden_nodes=H, hidden_layer=args.hidden_layer, nsteps=8, noptepochs=5, nminibatches=4, replay_size=100, polyak=0.995,
                         learning_rate=1e-4, max_grad_norm=1, policy_delay=2, gamma=0.99, act_noise=0.1, target_noise=0.2, noise_clip=0.5, reward_scale=1,
                         batch_size=64)

            def make(fused):
                cfg = default_cfg("MultiIngenuity")
                cfg["env"]["numEnvs"] = args.envs
                cfg["seed"] = 1
                env = VecTaskPython(MultiIngenuity(cfg, None, "physx", "cuda" if gpu else "cpu", 0, True), str(dev), 5.0, 1.0)
                torch.manual_seed(0)
                random.seed(0)
                agent = cls(env, {"learn": dict(learn, fused_update=fused)}, device=str(dev), log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)
                agent.save = lambda path: None
                iterations = [0]

                def one_iteration():
                    agent.current_learning_iteration = iterations[0]
                    iterations[0] += 1
                    agent.run(iterations[0], log_interval=10 ** 9)
                    sync()
                for _ in range(10):                 # past the warm-up (more than 64 transitions) and every first launch
                    one_iteration()
                assert agent.warm_up is False
                return agent, one_iteration
            sides = {"default": make(False), "fused_update": make(True)}
            shape = [16, args.envs, W]
            common = {"algo": algo, "hidden": [H] * args.hidden_layer, "minibatch": shape}
            if "update" in series:
                res = alternate({k: s.update for k, (s, _) in sides.items()}, max(1, args.reps // 10))
                emit({"series": "update", **common, "steps": "5 epochs x (Q step + policy step)", "unit": "ms per update(): median (min - max) over the rounds",
                      "verdict": verdict(res), **res})
            if "run" in series:
                res = alternate({k: it for k, (_, it) in sides.items()}, 1, warm=1, events=False)
                emit({"series": "run", **common, "env_steps": 8, "updates": 8, "unit": "ms per run iteration, host clock to a device synchronise, checkpoint "
                      "writing left out: median (min - max) over the rounds", "verdict": verdict(res), **res})
            del sides
            if gpu:
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

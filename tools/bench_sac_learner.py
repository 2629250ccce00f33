#!/usr/bin/env python3
"""The SAC learner (algorithms/rl/sac/sac.py) with `fused_update` on and off, in one process on the HIP device, at cfg/sac/config.yaml's
shapes on MultiIngenuity: 8192 envs, hidden 3 x 1024 ELU, nsteps 8, noptepochs 1, nminibatches 4, batch_size 32 -- a minibatch of 8 ring
rows x 8192 envs = 65536 rows.  (replay_size is 64 instead of 5000: the ring's length changes no shape that is timed.)

  head      mms_q_heads_loss alone at [65536, 1024], G = 2, every output wanted, mode 0 and mode 1: per call the time and the achieved
            bytes/s over the bytes the algorithm needs (4 G M H read, 4 G M H written for dh, plus the [M] vectors) -- both launches
  update    one `update()` (4 minibatches) of a learner past its warm-up: the default route (what the reference's sac.py obtains
            from this package's modules) against `fused_update=True`
  run       one `run` iteration (8 env steps, each followed by an `update()`) of the same two learners; writing the checkpoint is
            left out (`save` replaced by a no-op), the log is off

After warm-up, `--rounds` rounds alternating the two sides; `head` and `update` between two device events, `run` on the host clock
around a call that ends in a device synchronise.  Per side the median with min and max.  The two sides start from equal parameters
and draw different noise, so `update` and `run` time two trajectories of the same cost, not the same numbers.  One JSON line per
series on stdout, appended to --out.

    python tools/bench_sac_learner.py [--series head,update,run] [--envs 8192] [--rounds 5] [--out profiles/sac_learner_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", default="head,update,run")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--hidden-nodes", type=int, default=1024)
    ap.add_argument("--hidden-layer", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="calls per window of `head`; `update` takes a tenth of it, `run` one")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0", help="\"cpu\": a rehearsal on the CPU build (wall-clock windows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_learner_bench.jsonl"))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("bench_sac_learner.py: at least 5 rounds")
    import torch
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.algorithms.rl.sac import SAC
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.vec_task import VecTaskPython
    from massive_marl_benchmark_amd.tasks.multi_ingenuity import MultiIngenuity
    dev = torch.device(args.device)
    gpu = dev.type == "cuda"
    if gpu and not torch.cuda.is_available():
        sys.exit("bench_sac_learner.py needs a HIP device (or --device cpu for a rehearsal)")
    sync = torch.cuda.synchronize if gpu else (lambda: None)
    summary = lambda ts: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    def emit(res):
        res.update(device=torch.cuda.get_device_name(0) if gpu else "cpu", envs=args.envs, hidden=[args.hidden_nodes] * args.hidden_layer, rounds=args.rounds)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

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

    series = args.series.split(",")
    if "head" in series:
        M, H, G = 8 * args.envs, args.hidden_nodes, 2
        L, idx, stream = _lib.for_device(dev)
        g = torch.Generator().manual_seed(1)
        h = [torch.nn.functional.elu(torch.randn(M, H, generator=g)).to(dev) for _ in range(G)]
        w = [(torch.randn(1, H, generator=g) * H ** -0.5).to(dev) for _ in range(G)]
        b = [torch.zeros(1, device=dev) for _ in range(G)]
        target, logp = torch.randn(M, generator=g).to(dev), torch.randn(M, generator=g).to(dev)
        loss, q = torch.empty((), device=dev), [torch.empty(M, device=dev) for _ in range(G)]
        dh, dw, db = [torch.empty(M, H, device=dev) for _ in range(G)], [torch.empty(H, device=dev) for _ in range(G)], [torch.empty(1, device=dev) for _ in range(G)]
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        n = ctypes.c_int64(-1)

        def call(mode, ws):
            _lib.check(L.mms_q_heads_loss(idx, M, H, p(h[0]), p(w[0]), p(b[0]), p(h[1]), p(w[1]), p(b[1]), mode, p(target if mode == 0 else None),
                                          p(logp if mode == 1 else None), 0.2, 1.0, p(loss), p(q[0]), p(q[1]), p(dh[0]), p(dh[1]), p(dw[0]), p(db[0]), p(dw[1]),
                                          p(db[1]), ws, ctypes.byref(n), stream), None, "mms_q_heads_loss", L)
        call(0, None)
        buf = torch.empty(n.value + 256, dtype=torch.uint8, device=dev)
        ws = ctypes.c_void_p(buf.data_ptr() + (-buf.data_ptr()) % 256)
        res = alternate({"mode0_mse": lambda: call(0, ws), "mode1_policy": lambda: call(1, ws)}, args.reps)
        nbytes = 4 * G * M * H * 2 + 4 * M * (1 + G) + 4 * G * (2 * H + 2)
        for k in res:
            res[k]["achieved_TB_per_s"] = round(nbytes / (res[k]["median"] * 1e-3) / 1e12, 3)
        emit({"series": "head", "rows": M, "H": H, "G": G, "bytes_needed": nbytes, "unit": "ms per call (both launches): median (min - max) over the rounds", **res})

    if "update" in series or "run" in series:
        learn = dict(hidden_nodes=args.hidden_nodes, hidden_layer=args.hidden_layer, nsteps=8, noptepochs=1, nminibatches=4, replay_size=64, polyak=0.99,
                     learning_rate=3e-4, max_grad_norm=1, ent_coef=0.2, reward_scale=1, batch_size=32, gamma=0.99)

        def make(fused):
            cfg = default_cfg("MultiIngenuity")
            cfg["env"]["numEnvs"] = args.envs
            cfg["seed"] = 1
            env = VecTaskPython(MultiIngenuity(cfg, None, "physx", "cuda" if gpu else "cpu", 0, True), str(dev), 5.0, 1.0)
            torch.manual_seed(0)
            random.seed(0)
            sac = SAC(env, {"learn": dict(learn, fused_update=fused)}, device=str(dev), log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)
            sac.save = lambda path: None
            sac.actor_critic.pi.reserve_counters(8 * args.envs, dev)
            iterations = [0]

            def one_iteration():
                sac.current_learning_iteration = iterations[0]
                iterations[0] += 1
                sac.run(iterations[0], log_interval=10 ** 9)
                sync()
            for _ in range(5):                  # past the warm-up (32 transitions) and every first launch
                one_iteration()
            assert sac.warm_up is False
            return sac, one_iteration
        sides = {"default": make(False), "fused_update": make(True)}
        shape = [8, args.envs, int(sides["default"][0].observation_space.shape[0])]
        if "update" in series:
            res = alternate({k: s.update for k, (s, _) in sides.items()}, max(1, args.reps // 10))
            emit({"series": "update", "minibatch": shape, "minibatches": 4, "unit": "ms per update(): median (min - max) over the rounds", **res})
        if "run" in series:
            res = alternate({k: it for k, (_, it) in sides.items()}, 1, warm=1, events=False)
            emit({"series": "run", "minibatch": shape, "env_steps": 8, "updates": 8, "unit": "ms per run iteration, host clock to a device synchronise, "
                  "checkpoint writing left out: median (min - max) over the rounds", **res})


if __name__ == "__main__":
    main()

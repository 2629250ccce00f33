#!/usr/bin/env python3
"""Time per `env.step` through the two drop-in wrappers, eager, TenAnt at 4096 envs: VecTaskPython (one 388-wide agent, 80 actions)
and MultiVecTaskPython (ten agents; the learners' list of ten [N, 8] action tensors).  What it is for: the wrappers return tensors
of their own (tests/test_dropin_contract.py), and this is what that costs -- run it from two trees to compare two versions of the
wrappers (profiles/wrapper_fresh_obs.json: three alternating pairs, one process each).

20 warm-up calls, then `--blocks` blocks of 200 timed calls, each block between two device synchronisations (host clock), so a
block's figure contains the launches' host cost and the device work, whichever is longer.  One JSON line.

    python tools/bench_wrapper_step.py [--num-envs 4096] [--warmup 20] [--steps 200] [--blocks 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.multi_vec_task import MultiVecTaskPython
    from massive_marl_benchmark_amd.tasks.agent_base.vec_task import VecTaskPython
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    if not torch.cuda.is_available():
        sys.exit("needs a HIP device: a CPU timing says nothing about the MI355X")
    n = args.num_envs
    out = {"label": args.label, "task": "TenAnt", "num_envs": n, "warmup": args.warmup, "steps": args.steps, "device": torch.cuda.get_device_name(0)}

    def timed(step):
        for _ in range(args.warmup):
            step()
        blocks = []
        for _ in range(args.blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / args.steps * 1e6)
        s = sorted(blocks)
        return {"us_per_step_blocks": [round(b, 2) for b in blocks], "us_per_step_median": round(s[len(s) // 2], 2), "us_per_step_min": round(s[0], 2)}

    g = torch.Generator(device="cuda").manual_seed(0)
    for name, multi, clip in (("vec_task", False, 5.0), ("multi_vec_task", True, 7.0)):
        cfg = default_cfg("TenAnt")
        cfg["env"]["numEnvs"] = n
        cfg["clip_observations"] = clip
        cfg["seed"] = 3
        task = TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=multi)
        if multi:
            env = MultiVecTaskPython(task, "cuda:0")
            actions = [torch.rand(n, 8, generator=g, device="cuda") * 2 - 1 for _ in range(10)]
        else:
            env = VecTaskPython(task, "cuda:0", clip, 1.0)
            actions = torch.rand(n, 80, generator=g, device="cuda") * 2 - 1
        env.reset()
        out[name] = timed(lambda: env.step(actions))
        torch.cuda.synchronize()
        task.engine.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

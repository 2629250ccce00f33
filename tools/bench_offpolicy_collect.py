#!/usr/bin/env python3
"""BASELINE configs[2]: MultiIngenuity, 8192 envs, the DDPG / TD3 collection loop (ddpg.py:151-159) --
MLPActorCritic.act (cfg/ddpg/config.yaml: 3 x 256, ReLU, tanh output; exploration noise module.py:54-61, drawn on the device) +
engine step + ReplayBuffer.add_transitions.  The learner's update is a caller and not part of the measurement.

Two variants of the same loop: `copies` (the wrapper's return values copied into the ring, as the reference does) and
`bound` (the step kernel writes next_obs / reward / done into the ring row `ReplayBuffer.slot()` names).  Each is timed
eagerly and as a replayed hipGraph of one pass over a 16-row window of the ring.

`--algo sac` runs the same loop with SAC's actor (cfg/sac/config.yaml: 3 x 1024, ELU; stochastic act, sac.py:166: the hidden layers
as mms_linear2_act launches, the squashed-Gaussian head as one mms_sac_heads_act launch) and also times the Q target's
pi(o2) under no_grad with logp on an [8, N, W] gather (sac.py:374-376: batch_size 32 / nminibatches 4 = 8 ring rows), fused
against the library path (torch's Linear / clamp / exp / randn / tanh / log chain) in the same process, and `target_q`: the three
lines behind it (sac.py:379-382: both target critics, the min, the Bellman backup) on the same gather by the same protocol, as
`library` (the torch modules), `fused_separate` (the reference's four lines over the fused MLPQFunction.forward: what an unmodified
sac.py gets) and `fused_backup` (actor_critic_targ.q_backup).  `--target-only` skips the timed collection loops (the ring is filled by
the warm-up steps alone): the run to put under a kernel trace.

`--layers f16x2` builds the modules with `layers="f16x2"` (the hidden layers of every fused path on the two-plane fp16 kernel,
ddpg.module.split16_hidden): the collection series and the `fused*` paths of target_pi / target_q then run it, and a copy of the same
modules set back to "fp32" joins the same alternating rounds as `fused_fp32` / `fused_backup_fp32` -- the A/B inside one process.

    python tools/bench_offpolicy_collect.py [--algo ddpg|sac] [--layers fp32|f16x2] [--num-envs 8192] [--steps 512] [--target-only]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("ddpg", "sac"), default="ddpg")
    ap.add_argument("--task", default="MultiIngenuity")
    ap.add_argument("--num-envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--replay-size", type=int, default=1024)
    ap.add_argument("--library-actor", action="store_true", help="A/B: the actor's layers as library GEMMs + activation passes")
    ap.add_argument("--env-spacing", type=float, default=None,
                    help="override env.envSpacing (0: every env at the origin, the helicopters fly; default: the reference's grid, where every env away "
                         "from the origin resets on every step -- positions and goals are global-frame, multi_ingenuity.py:381-453)")
    ap.add_argument("--layers", choices=("fp32", "f16x2"), default="fp32", help="the modules' `layers` keyword (hidden layers of the fused paths)")
    ap.add_argument("--target-only", action="store_true", help="--algo sac: only the target_pi / target_q series (no timed collection loop, no graph)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from massive_marl_benchmark_amd import spaces
    from massive_marl_benchmark_amd.algorithms.rl.ddpg.module import MLPActorCritic
    from massive_marl_benchmark_amd.algorithms.rl.ddpg.storage import ReplayBuffer
    from massive_marl_benchmark_amd.algorithms.rl.sac.module import MLPActorCritic as SACActorCritic
    from massive_marl_benchmark_amd.engine import Engine

    N = args.num_envs
    torch.manual_seed(0)
    out = {"task": args.task, "num_envs": N, "replay_size": args.replay_size, "actor": "library" if args.library_actor else "mms_linear2_act",
           "env_spacing": "reference default" if args.env_spacing is None else args.env_spacing}
    out["layers"] = args.layers
    if args.algo == "sac":
        out = {"algo": "sac", **out, "actor": "library" if args.library_actor else "mms_linear2_act + mms_sac_heads_act", "hidden": [1024, 1024, 1024]}
    from massive_marl_benchmark_amd.model import default_cfg
    cfg = None
    if args.env_spacing is not None:
        cfg = default_cfg(args.task)
        cfg["env"]["envSpacing"] = float(args.env_spacing)
    for variant in (("bound",) if args.target_only else ("copies", "bound")):
        eng = Engine(args.task, cfg=cfg, num_envs=N, device=0, seed=0, clip_obs=5.0)
        W, AD = eng.obs_dim, eng.num_actions
        if args.algo == "sac":
            ac = SACActorCritic(spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-np.ones(AD), np.ones(AD)),
                                hidden_sizes=[1024, 1024, 1024], layers=args.layers).cuda()                # cfg/sac/config.yaml: hidden_nodes 1024 x 3, ELU
            if args.library_actor:
                ac.pi.forward = ac.pi.torch_forward
            ac.pi.reserve_counters(8 * N, torch.device("cuda:0"))     # the graph below pins them; pi(o2) later runs on 8 N rows
        else:
            ac = MLPActorCritic(spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-np.ones(AD), np.ones(AD)), 0.1, "cuda:0",
                                hidden_sizes=[256, 256, 256], layers=args.layers).cuda()                   # cfg/ddpg/config.yaml: hidden_nodes 256 x 3
            if args.library_actor:
                ac.pi.forward = lambda obs, _pi=ac.pi: _pi.act_limit * _pi.pi(obs)
        buf = ReplayBuffer(N, args.replay_size, 64, 8, (W,), (0,), (AD,), "cuda:0")
        states = torch.zeros(N, 0, device="cuda")
        act_buf, rew, done, obs_c = eng.tensor("actions"), eng.tensor("rew"), eng.tensor("reset"), eng.tensor("obs_clipped")
        eng.reset_all()
        eng.step()
        cur = obs_c.clone()
        if variant == "bound":
            eng.set_obs_outputs(raw=False, clipped=False)

        def step():
            a = ac.act(cur, deterministic=False)                                   # act_noise 0.1, act_limit 1
            k = buf.slot()
            if variant == "bound":
                eng.bind_obs_out(buf.next_observations[k])
                eng.bind_rollout_out(buf.rewards[k].view(-1), buf.dones[k].view(-1))
                act_buf.copy_(a)
                eng.step()
                buf.add_transitions(cur, states, a, buf.rewards[k], buf.next_observations[k], buf.dones[k])
                cur.copy_(buf.next_observations[k])
            else:
                act_buf.copy_(a)
                eng.step()
                buf.add_transitions(cur, states, a, rew, obs_c, done)
                cur.copy_(obs_c)

        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for _ in range(64):
                step()
            s.synchronize()
        if args.target_only:
            torch.cuda.current_stream().wait_stream(s)
            out["target_pi"] = time_target_pi(ac, buf, args.steps)
            out["target_q"] = time_target_q(ac, buf, args.steps)
            eng.bind_obs_out(None); eng.bind_rollout_out(None, None)
            eng.close()
            break
        with torch.cuda.stream(s):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.steps):
                step()
            e1.record(s); s.synchronize()
            eager_ms = e0.elapsed_time(e1) / args.steps
            # one pass over a 16-row window as a graph (the window's addresses are baked in; a learner that wants the whole ring
            # captures replay_size / 16 such graphs or replays eagerly)
            buf.step = 16
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                for _ in range(16):
                    step()
            buf.step = 16
            graph.replay(); s.synchronize()
            reps = max(1, args.steps // 16)
            e0.record(s)
            for _ in range(reps):
                graph.replay()
            e1.record(s); s.synchronize()
            graph_ms = e0.elapsed_time(e1) / (reps * 16)
        finite = bool(torch.isfinite(buf.next_observations[:32]).all())
        n_steps = 1 + 64 + args.steps + 16 + 16 + reps * 16
        out[variant] = {"resets_per_env_step": int(eng.tensor("reset_count").sum()) / float(N * n_steps),"eager_ms_per_step": eager_ms, "eager_env_steps_per_s": N / (eager_ms * 1e-3),
                        "graph_ms_per_step": graph_ms, "graph_env_steps_per_s": N / (graph_ms * 1e-3), "finite": finite}
        eng.bind_obs_out(None); eng.bind_rollout_out(None, None)
        del graph
        if args.algo == "sac" and variant == "bound":
            out["target_pi"] = time_target_pi(ac, buf, args.steps)
            out["target_q"] = time_target_q(ac, buf, args.steps)
        eng.close()
    print(json.dumps(out), flush=True)


def with_layers(module, layers):
    """A deepcopy of `module` with every sub-module's `layers` set (the same parameters' values on the other layer kernel)."""
    import copy
    m = copy.deepcopy(module)
    for sub in m.modules():
        if hasattr(sub, "layers"):
            sub.layers = layers
    return m


def time_target_pi(ac, buf, steps):
    """pi(o2) under no_grad with logp on an [8, N, W] gather of the ring (sac.py:374-376), fused and library alternating (5 rounds)."""
    import torch
    pi = ac.pi
    o2 = buf.next_observations[torch.arange(8, device=buf.next_observations.device)]
    paths = {"fused": lambda x: type(pi).forward(pi, x), "library": pi.torch_forward}     # (whatever --library-actor set for the loop)
    if pi.layers != "fp32":
        pi32 = with_layers(pi, "fp32")
        paths["fused_fp32"] = lambda x: type(pi32).forward(pi32, x)
    res = {k: [] for k in paths}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = max(8, steps // 8)
    with torch.no_grad():
        for f in paths.values():
            for _ in range(4):
                a2, logp = f(o2)
        torch.cuda.synchronize()
        for _ in range(5):
            for k, f in paths.items():
                e0.record()
                for _ in range(reps):
                    a2, logp = f(o2)
                e1.record(); e1.synchronize()
                res[k].append(e0.elapsed_time(e1) / reps)
    rows = o2.shape[0] * o2.shape[1]
    out = {"shape": list(o2.shape), "rows": rows, "calls_per_round": reps, "finite": bool(torch.isfinite(a2).all() and torch.isfinite(logp).all())}
    for k, v in res.items():
        out[k + "_ms_per_call"] = float(np.median(v))
        out[k + "_ms_rounds"] = v
        out[k + "_ms_spread"] = float(max(v) - min(v))
    out["speedup"] = out["library_ms_per_call"] / out["fused_ms_per_call"]
    if "fused_fp32" in res:
        out["speedup_over_fused_fp32"] = out["fused_fp32_ms_per_call"] / out["fused_ms_per_call"]
    return out


def time_target_q(ac, buf, steps, gamma=0.99, alpha=0.2):
    """The Q target behind pi(o2) (sac.py:379-382) on the same [8, N, .] gather, a2 and logp from one pi(o2) call: the torch modules,
    the reference's four lines over the fused MLPQFunction.forward, and q_backup -- warm-up of every path, then five rounds alternating
    the paths, medians and all rounds kept."""
    import copy

    import torch
    idx = torch.arange(8, device=buf.next_observations.device)
    o2, r, d = buf.next_observations[idx], buf.rewards[idx], buf.dones[idx]
    targ = copy.deepcopy(ac)                                       # sac.py:104: actor_critic_targ
    for m in (targ, targ.q1, targ.q2):
        m.fused_q = True
    lib = copy.deepcopy(targ)
    for m in (lib, lib.q1, lib.q2):
        m.fused_q = False

    def four_lines(t):
        def f():
            q1_pi_targ = t.q1(o2, a2)
            q2_pi_targ = t.q2(o2, a2)
            q_pi_targ = torch.min(q1_pi_targ, q2_pi_targ)
            return r + gamma * (1 - d) * (q_pi_targ - alpha * logp_a2)
        return f

    paths = {"library": four_lines(lib), "fused_separate": four_lines(targ), "fused_backup": lambda: targ.q_backup(o2, a2, r, d, gamma, alpha, logp_a2)}
    if targ.layers != "fp32":
        targ32 = with_layers(targ, "fp32")
        paths["fused_backup_fp32"] = lambda: targ32.q_backup(o2, a2, r, d, gamma, alpha, logp_a2)
    res = {k: [] for k in paths}
    last = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = max(8, steps // 8)
    with torch.no_grad():
        a2, logp_a2 = ac.pi(o2)
        for f in paths.values():
            for _ in range(4):
                f()
        torch.cuda.synchronize()
        for _ in range(5):
            for k, f in paths.items():
                e0.record()
                for _ in range(reps):
                    last[k] = f()
                e1.record(); e1.synchronize()
                res[k].append(e0.elapsed_time(e1) / reps)
    M, H, G = o2.shape[0] * o2.shape[1], targ.q1.q[-2].in_features, 2
    scale = float(1 + last["library"].abs().max())
    out = {"shape": list(o2.shape), "rows": M, "hidden": [l.out_features for l in list(targ.q1.q)[:-2:2]], "dones_dtype": str(d.dtype).replace("torch.", ""),
           "calls_per_round": reps, "finite": bool(all(torch.isfinite(v).all() for v in last.values())),
           "max_diff_vs_library": {k: float((last[k] - last["library"]).abs().max()) / scale for k in last if k != "library"},
           # what mms_q_heads_backup must move: both hidden activations, r (4) + d (1) + logp (4) in and the backup (4) out per row, the weights once
           "tail_kernel_bytes": 4 * G * M * H + 13 * M + 4 * G * (H + 1)}
    for k, v in res.items():
        out[k + "_ms_per_call"] = float(np.median(v))
        out[k + "_ms_rounds"] = v
        out[k + "_ms_spread"] = float(max(v) - min(v))
    out["speedup_fused_backup"] = out["library_ms_per_call"] / out["fused_backup_ms_per_call"]
    out["speedup_fused_separate"] = out["library_ms_per_call"] / out["fused_separate_ms_per_call"]
    if "fused_backup_fp32" in res:
        out["speedup_over_fused_backup_fp32"] = out["fused_backup_fp32_ms_per_call"] / out["fused_backup_ms_per_call"]
    return out


if __name__ == "__main__":
    main()

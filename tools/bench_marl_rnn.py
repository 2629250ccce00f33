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

--rnn-format f16x2 (or both) adds the opt-in plane route of GroupedPolicyInference(rnn_format="f16x2") to the same alternating rounds,
against the grouped fp32 pass of the same process:

  grouped16_ms   the same get_actions of an object built with rnn_format="f16x2" (rnn_route says which route the calls took: envs
                 that are no multiple of 128 stay on the fp32 route), f16x2_speedup_median = grouped_ms / grouped16_ms
  rnn16_stages_us  what the route adds per GRU layer, each stage alone for all 20 networks (`--calls` back-to-back launches between
                 two device events): the splits of x and of the state, the two products (N = 3H) and mms_gru_gates_group with the
                 bytes it moves per second (gi, gh and h read, h_out and y written)
  error_vs_f64   rms error of the values and of the actors' / critics' new states against float64 copies of the modules: the fp32
                 route, the f16x2 route and the per-agent torch fp32 modules

Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_marl_rnn.py --envs 4096 --profile-passes 20`
runs nothing but 20 passes of the f16x2 route (after 3 of warm-up); `--kernel-stats DIR/.../*kernel_stats.csv --envs 4096 --profile-passes 20`
then prints (and appends to --out) one JSON line with every kernel's calls per pass and average time.

    python tools/bench_marl_rnn.py [--envs 4096,80] [--rounds 5] [--calls 20] [--rnn-format fp32|f16x2|both] [--out profiles/marl_rnn_bench.jsonl]
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
    ap.add_argument("--rnn-format", default="fp32", choices=["fp32", "f16x2", "both"])
    ap.add_argument("--profile-passes", type=int, default=0, help="only this many passes of the f16x2 route: the run to put under rocprofv3")
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 kernel_stats.csv of such a run: print its per-kernel times and exit")
    args = ap.parse_args()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if args.kernel_stats:
        import csv
        passes = max(args.profile_passes, 1) + 3
        rows = [r for r in csv.DictReader(open(args.kernel_stats))]
        kernels = [{"name": r["Name"].split("(")[0][-60:], "calls_per_pass": round(int(r["Calls"]) / passes, 2), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                    "us_per_pass": round(int(r["Calls"]) * float(r["AverageNs"]) / 1e3 / passes, 2)} for r in rows if int(r["Calls"]) >= passes and "mms::" in r["Name"]]        # (the engine's kernels: not the constructor's torch copies)
        emit({"bench": "marl_rnn_kernels", "rnn_format": "f16x2", "envs": int(args.envs.split(",")[0]), "passes": passes, "source": "rocprofv3 --kernel-trace --stats",
              "kernels": kernels, "us_per_pass_total": round(sum(k["us_per_pass"] for k in kernels), 1)})
        return
    with16 = args.rnn_format != "fp32" or args.profile_passes > 0
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
    grouped16 = GroupedPolicyInference(actors, critics, seed=3, rnn_format="f16x2") if with16 else None

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

        def run_grouped16():
            grouped16.get_actions(sobs_l, obs_l, **kw)
        if args.profile_passes:
            for _ in range(3 + args.profile_passes):
                run_grouped16()
            torch.cuda.synchronize()
            print("profile passes: %d + 3 at %d envs, route %s" % (args.profile_passes, envs, grouped16.rnn_route))
            continue

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
        if with16:
            ts["grouped16_ms"] = []
            for _ in range(3):
                run_grouped16()
        for _ in range(args.rounds):
            ts["grouped_ms"].append(a_round(run_grouped))
            if with16:
                ts["grouped16_ms"].append(a_round(run_grouped16))
            ts["per_agent_ms"].append(a_round(run_per_agent))
        stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res = {"bench": "marl_rnn", "agents": N, "obs": OBS, "share_obs": SOBS, "act": ACT, "hidden": H, "layer_N": LAYER_N, "recurrent_N": R, "envs": envs,
               "rounds": args.rounds, "calls": args.calls, "device": torch.cuda.get_device_name(0), "agree": agree}
        res.update({k: stat(v) for k, v in ts.items()})
        res["speedup_median"] = round(res["per_agent_ms"]["median"] / res["grouped_ms"]["median"], 3)
        if with16:
            res["rnn_route"] = grouped16.rnn_route
            res["f16x2_speedup_median"] = round(res["grouped_ms"]["median"] / res["grouped16_ms"]["median"], 3)
            res["error_vs_f64"] = errors_vs_f64(torch, rm, actors, critics, obs, sobs, states, states_c, masks, values, run_grouped, run_grouped16, run_per_agent)
            if grouped16.rnn_route == "f16x2":
                res["rnn16_stages_us"] = stage_times(torch, _lib, L, idx, stream, envs, args, rnd, masks)

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
        emit(res)
        del x, h_in, h_out, y, wi, wh
        torch.cuda.empty_cache()


def errors_vs_f64(torch, rm, actors, critics, obs, sobs, states, states_c, masks, values, run_fp32, run_f16x2, run_torch):
    """rms error of (values, actors' new states, critics' new states) against float64 copies of the modules, per path"""
    import copy
    truth = []
    for k in range(N):
        a, c = copy.deepcopy(actors[k]).double(), copy.deepcopy(critics[k]).double()
        _, _, v, na, nc = rm.torch_forward(a, c, obs[:, k].double(), sobs.double(), states[0][:, k].double(), states_c[0][:, k].double(), masks.double())
        truth.append((v[:, 0], na, nc))
        del a, c
    tv, ta, tc = (torch.stack([t[i] for t in truth], 1) for i in range(3))
    rms = lambda t: float(t.pow(2).mean().sqrt())
    out = {"truth_rms": {"values": rms(tv), "rnn_states": rms(ta), "rnn_states_critic": rms(tc)}}
    for name, fn in (("fp32", run_fp32), ("f16x2", run_f16x2), ("torch_fp32", run_torch)):
        fn()
        torch.cuda.synchronize()
        out[name] = {"values": rms(values.double() - tv), "rnn_states": rms(states[1].double() - ta), "rnn_states_critic": rms(states_c[1].double() - tc)}
    return out


def stage_times(torch, _lib, L, idx, stream, envs, args, rnd, masks):
    """the five launches the plane route adds per GRU layer, each alone for 20 networks at M = envs, K = H: median us (min - max)"""
    G, M = 2 * N, envs
    tab = lambda ts_: (ctypes.c_void_p * len(ts_))(*[t.data_ptr() for t in ts_])
    u8 = lambda rows: [torch.empty(_lib.h32_bytes(rows, H), dtype=torch.uint8, device="cuda:0") for _ in range(G)]
    f32 = lambda *s: torch.empty(*s, device="cuda:0")
    x, h_in = [rnd(M, H) for _ in range(G)], torch.tanh(rnd(G, M, R, H))
    h_out, y = f32(G, M, R, H), f32(G, M, H)
    w = [rnd(3 * H, H) * H ** -0.5 for _ in range(G)]
    bi, bh = [rnd(3 * H) * 0.1 for _ in range(G)], [rnd(3 * H) * 0.1 for _ in range(G)]
    px, ph, pw = u8(M), u8(M), u8(3 * H)
    xs, xi, hs, hi, ws, wi = f32(G, M), f32(G, M), f32(G, M), f32(G, M), f32(G, 3 * H), f32(G, 3 * H)
    gi, gh = f32(G, M, 3 * H), f32(G, M, 3 * H)
    ub = lambda t: tab(list(t.unbind(0)))
    _lib.check(L.mms_weight_planes16_group(idx, G, (ctypes.c_int64 * G)(*[3 * H] * G), (ctypes.c_int32 * G)(*[H] * G), tab(w), tab(pw), ub(ws), ub(wi), None, stream),
               None, "mms_weight_planes16_group", L)
    none6 = (None,) * 6
    stages = {
        "split_x": (L.mms_split_planes16_group, (idx, G, M, H, H, tab(x), tab(px), ub(xs), ub(xi), 0, 0, None, None, None, None, 1e-5, stream)),
        "split_h": (L.mms_split_planes16_group, (idx, G, M, H, R * H, ub(h_in), tab(ph), ub(hs), ub(hi), 0, 0, None, None, None, None, 1e-5, stream)),
        "product_gi": (L.mms_linear_group_act_split16, (idx, G, M, 3 * H, H, tab(px), tab(pw), tab(bi), ub(gi), ub(xi), ub(wi), None, 0, 0) + none6 + (stream,)),
        "product_gh": (L.mms_linear_group_act_split16, (idx, G, M, 3 * H, H, tab(ph), tab(pw), tab(bi), ub(gh), ub(hi), ub(wi), None, 0, 0) + none6 + (stream,)),
        "gates": (L.mms_gru_gates_group, (idx, G, M, H, ub(gi), ub(gh), 3 * H, ub(h_in), R * H, tab([masks] * G), 1, tab(bh), ub(h_out), R * H, ub(y), stream)),
    }
    out = {}
    for name, (fn, a) in stages.items():
        us = []
        for _ in range(args.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                _lib.check(fn(*a), None, name, L)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000 / args.calls)
        us = us[1:]
        out[name] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    gbytes = 4.0 * G * M * (2 * 3 * H + H + 2 * H) / 1e9
    out["gates"]["GB"] = round(gbytes, 3)
    out["gates"]["TB_per_s"] = round(gbytes / out["gates"]["median"] * 1e3, 2)
    out["product_gi"]["TFLOPs"] = round(2.0 * G * M * 3 * H * H / out["product_gi"]["median"] / 1e6, 1)
    return out


if __name__ == "__main__":
    main()

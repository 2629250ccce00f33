#!/usr/bin/env python3
"""The feed-forward MAPPO update at TenAnt's shapes (obs 46, share_obs 388, 8 actions, hidden 512, layer_N 2: three
`Linear + ELU + LayerNorm` blocks per network; modules of tests/marl_modules.py, FusedAdam optimizers) on the HIP device: the trainers'
opt-in `fused_block_update` route (algorithms/marl/blocks.py: per block level one library product per network, mms_elu_ln_group forward,
mms_elu_ln_grad_group backward) against the default torch route (addmm, elu, layer_norm and autograd's backward of them), both measured
in this process.  Per number of rows of a minibatch (default 640 = 80 x 8, the configs' rollout, and 32768 = 4096 x 8), in alternating
rounds (torch, fused, torch, ...), each round `--calls` passes between two host-clock reads that end in a device synchronise, after
warm-up passes of the same shape; reported as the median round with (min - max), in ms per pass:

  blocks_*_ms   MLPBase.forward of the actor and of the critic + backward of a weighted sum of their outputs: `torch` the modules' own
                layers one network after the other, `fused` mlp_base for both in grouped calls
  update_*_ms   one whole MAPPO.ppo_update (bases, heads, mms_marl_ppo_loss, backward, mms_param_step) on a gathered sample, with the
                config key off and on

`verdict` compares the two windows: "faster" / "slower" when they do not overlap, else "no result at that size".  The worst
difference of the two routes' outputs is printed as a check that they compute the same thing.  One JSON line per size on stdout (and
appended to --out when given).

`--products {library,f16x2,both}` measures the forward products of the fused route instead (the trainers' `block_products`): the same
two series with `fused_block_update` on in every column, `library` (the route above) against `f16x2` (the two-plane fp16 layer kernel
and mms_elu_ln_planes16_group) in alternating rounds of this process, the same verdict rule, and per route the relative Frobenius error
of the bases' outputs and of their parameter gradients against a float64 evaluation of the modules on the device ("bench":
"marl_block_products").  Rows must be multiples of 128 there.

Kernel times are not taken here: `--trace ROUTE` runs warm-up and `--calls` passes of the blocks series of one route (torch | fused |
f16x2: fused with the plane products) at the first size of --rows and nothing else, for a kernel-trace run of its own (rocprofv3
--kernel-trace --stats -- python tools/bench_marl_block_update.py --rows 32768 --trace fused).  `--trace compose` runs, for two
networks' [rows, 512] blocks, mms_elu_ln_group followed by mms_split_planes16_group on its y, and mms_elu_ln_planes16_group, which
writes the same bytes in one launch: the three kernels' times at one shape in one trace.

    python tools/bench_marl_block_update.py [--rows 640,32768] [--rounds 5] [--calls 10] [--products both]
                                            [--out profiles/marl_block_update_bench.jsonl]
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

OBS, SOBS, ACT, H, LAYER_N = 46, 388, 8, 512, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="640,32768")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", default="", choices=["", "torch", "fused", "f16x2", "compose"])
    ap.add_argument("--products", default="", choices=["", "library", "f16x2", "both"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import marl_loss_check as mlc
    import marl_modules as mm
    from massive_marl_benchmark_amd.algorithms.marl import trainer as tr
    from massive_marl_benchmark_amd.algorithms.marl.blocks import mlp_base
    from massive_marl_benchmark_amd.optim import FusedAdam
    if not torch.cuda.is_available():
        sys.exit("bench_marl_block_update.py needs a HIP device")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(1)
    torch.manual_seed(1)
    actor, critic = mm.Actor(OBS, ACT, H, LAYER_N), mm.Critic(SOBS, H, LAYER_N)
    for m in (actor, critic):
        mm.randomize(m, gen)
        m.to(dev).train()

    class Policy:
        def __init__(self):
            self.actor, self.critic = copy.deepcopy(actor), copy.deepcopy(critic)
            self.actor_optimizer = FusedAdam(self.actor.parameters(), lr=5e-4, eps=1e-5)
            self.critic_optimizer = FusedAdam(self.critic.parameters(), lr=5e-4, eps=1e-5)

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

    def products_series(rows, obs, sobs, wa, wc, rnd, blocks_fused, params, timed, verdict, win):
        """the --products record of one size: both series per route with fused_block_update on, and the routes' errors against float64"""
        routes = ["library", "f16x2"] if args.products == "both" else [args.products]
        config = mlc.trainer_config(hidden_size=H, fused_block_update=True)
        trainers = {r: tr.MAPPO(dict(config, block_products=r), Policy(), dev) for r in routes}
        with torch.no_grad():
            mu, std, v = mm.torch_forward(actor, critic, obs, sobs)
        act = mu + std * rnd(rows, ACT)
        sample = (sobs, obs, None, None, act, v + 0.3 * rnd(rows, 1), v + rnd(rows, 1), None, torch.ones(rows, 1, device=dev),
                  mm.log_prob(mu, std, act) + 0.1 * rnd(rows, ACT), rnd(rows, 1), None, None)
        blk = timed({r: (lambda r=r: blocks_fused(r, r)) for r in routes})
        upd = timed({r: (lambda t=t: t.ppo_update(sample)) for r, t in trainers.items()})
        res = {"bench": "marl_block_products", "rows": rows, "hidden": H, "blocks": LAYER_N + 1, "rounds": args.rounds, "calls": args.calls}
        for r in routes:
            res["blocks_%s_ms" % r], res["update_%s_ms" % r] = win(blk[r]), win(upd[r])
        # float64 on the device: the modules' own layers on the same fp32 values
        bases64 = [copy.deepcopy(actor.base).double(), copy.deepcopy(critic.base).double()]
        ys64 = [tr._base(b, x.double()) for b, x in zip(bases64, (obs, sobs))]
        ((ys64[0] * wa.double()).sum() + (ys64[1] * wc.double()).sum()).backward()
        g64 = torch.cat([p.grad.reshape(-1) for b in bases64 for p in b.parameters()])
        y64 = torch.cat([y.detach().reshape(-1) for y in ys64])
        for r in routes:
            for p in params:
                p.grad = None
            ys = mlp_base([obs, sobs], [actor.base, critic.base], r)
            ((ys[0] * wa).sum() + (ys[1] * wc).sum()).backward()
            y = torch.cat([t.detach().reshape(-1) for t in ys]).double()
            gr = torch.cat([p.grad.reshape(-1) for p in params]).double()
            res["y_err_f64_%s" % r], res["grad_err_f64_%s" % r] = float((y - y64).norm() / y64.norm()), float((gr - g64).norm() / g64.norm())
        if len(routes) == 2:
            for series, w in (("blocks", blk), ("update", upd)):
                res[series + "_speedup_median"] = round(w["library"][0] / w["f16x2"][0], 3)
                res[series + "_verdict"] = verdict(w["library"], w["f16x2"])
            res["max_abs_diff_y"], res["max_abs_diff_dw1"] = [float((a - b).abs().max()) for a, b in zip(seen["library"], seen["f16x2"])]
        return res

    for rows in [int(v) for v in args.rows.split(",")]:
        g = torch.Generator(device=dev).manual_seed(rows)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
        obs, sobs = rnd(rows, OBS), rnd(rows, SOBS)
        wa, wc = rnd(rows, H), rnd(rows, H)
        seen = {}
        params = list(actor.base.parameters()) + list(critic.base.parameters())

        def blocks_torch():
            for p in params:
                p.grad = None
            ya, yc = tr._base(actor.base, obs), tr._base(critic.base, sobs)
            ((ya * wa).sum() + (yc * wc).sum()).backward()
            seen["torch"] = (ya.detach(), actor.base.mlp.fc1[0].weight.grad.clone())

        def blocks_fused(products="library", key="fused"):
            for p in params:
                p.grad = None
            ya, yc = mlp_base([obs, sobs], [actor.base, critic.base], products)
            ((ya * wa).sum() + (yc * wc).sum()).backward()
            seen[key] = (ya.detach(), actor.base.mlp.fc1[0].weight.grad.clone())

        if args.trace == "compose":
            import ctypes
            from massive_marl_benchmark_amd import _lib
            L, idx, stream = _lib.for_device(dev)
            tab = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
            two = lambda *shape, **kw: [torch.empty(*shape, device=dev, **kw) for _ in range(2)]
            z, par = [rnd(rows, H), rnd(rows, H)], [[rnd(H), rnd(H)] for _ in range(3)]
            y, stat, planes, inv = two(rows, H), two(rows, 2), two(_lib.h32_bytes(rows, H), dtype=torch.uint8), two(rows)
            head = (idx, 2, rows, H, 1e-5, tab(z), H, tab(par[0]), tab(par[1]), tab(par[2]), tab(y), H, tab(stat))
            for _ in range(args.warmup + args.calls):
                _lib.check(L.mms_elu_ln_group(*head, stream), None, "mms_elu_ln_group", L)
                _lib.check(L.mms_split_planes16_group(idx, 2, rows, H, H, tab(y), tab(planes), tab([None, None]), tab(inv), 0, 0, None, None, None, None, 0.0,
                                                      stream), None, "mms_split_planes16_group", L)
                _lib.check(L.mms_elu_ln_planes16_group(*head, tab(planes), tab([None, None]), tab(inv), stream), None, "mms_elu_ln_planes16_group", L)
            torch.cuda.synchronize()
            return
        if args.trace:
            fn = {"torch": blocks_torch, "fused": blocks_fused, "f16x2": lambda: blocks_fused("f16x2")}[args.trace]
            for _ in range(args.warmup + args.calls):
                fn()
            torch.cuda.synchronize()
            return
        win = lambda w: {"median": round(w[0], 3), "min": round(w[1], 3), "max": round(w[2], 3)}
        if args.products:
            res = products_series(rows, obs, sobs, wa, wc, rnd, blocks_fused, params, timed, verdict, win)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            continue
        config = mlc.trainer_config(hidden_size=H)
        trainers = {"torch": tr.MAPPO(config, Policy(), dev), "fused": tr.MAPPO(dict(config, fused_block_update=True), Policy(), dev)}
        with torch.no_grad():
            mu, std, v = mm.torch_forward(actor, critic, obs, sobs)
        act = mu + std * rnd(rows, ACT)
        sample = (sobs, obs, None, None, act, v + 0.3 * rnd(rows, 1), v + rnd(rows, 1), None, torch.ones(rows, 1, device=dev),
                  mm.log_prob(mu, std, act) + 0.1 * rnd(rows, ACT), rnd(rows, 1), None, None)
        blk = timed({"torch": blocks_torch, "fused": blocks_fused})
        diff = [float((a - b).abs().max()) for a, b in zip(seen["torch"], seen["fused"])]
        upd = timed({k: (lambda t=t: t.ppo_update(sample)) for k, t in trainers.items()})
        res = {"bench": "marl_block_update", "rows": rows, "hidden": H, "blocks": LAYER_N + 1, "rounds": args.rounds, "calls": args.calls,
               "blocks_torch_ms": win(blk["torch"]), "blocks_fused_ms": win(blk["fused"]), "blocks_speedup_median": round(blk["torch"][0] / blk["fused"][0], 3),
               "blocks_verdict": verdict(blk["torch"], blk["fused"]),
               "update_torch_ms": win(upd["torch"]), "update_fused_ms": win(upd["fused"]), "update_speedup_median": round(upd["torch"][0] / upd["fused"][0], 3),
               "update_verdict": verdict(upd["torch"], upd["fused"]), "max_abs_diff_y": diff[0], "max_abs_diff_dw1": diff[1]}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()

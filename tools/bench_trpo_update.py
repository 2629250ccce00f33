#!/usr/bin/env python3
"""TRPO's update (agents/algorithms/rl/trpo/trpo.py:258-351) at the shipped shape, this build's ActorCritic with the actor's backward and
R-op on the HIP kernels (fused_grad=True) against the same module with torch autograd (fused_grad=False).

Synthetic storage: TenAnt (obs 388, 80 actions), cfg/trpo/config.yaml (actor and critic [1024, 1024, 512] ELU, 4096 envs x nsteps 8,
nminibatches 4: 8192-row minibatches, cg_nsteps 3, noptepochs 5, damping 0.1, max_kl 0.1, max_num_backtrack 10, accept_ratio 0.01,
step_fraction 0.1, value_loss_coef unused by TRPO, Adam 1e-3 on the critic).  The minibatch below follows trpo.py step by step: actor
gradient (:290), KL (:294-298), conjugate gradient with kl_hessian_times_vector (:300, :417-435), sAs (:303), line search (:384-415),
set_pi_flat_params, the value loss and its Adam step (:318-340).  The actor is moved off `old_mu` before timing, as after a first
minibatch.

  (a) one HVP shaped like kl_hessian_times_vector (both autograd.grad calls), from a standing evaluate;
  (b) one whole minibatch;
  (c) one update(): noptepochs x nminibatches minibatches.
Each: warm-up, then the median of --repeats timings between HIP events ((c): 3); (b) and (c) restore the parameters and the optimizer
state before every call, and record the line search's backtracking steps per timing.  One JSON line per path, then the ratios.

    python tools/bench_trpo_update.py [--rows 8192] [--repeats 10] [--only fused|torch] [--skip-update]
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = {"pi_hid_sizes": [1024, 1024, 512], "vf_hid_sizes": [1024, 1024, 512], "activation": "elu"}
HP = dict(damping=0.1, cg_nsteps=3, max_kl=0.1, max_num_backtrack=10, accept_ratio=0.01, step_fraction=0.1, max_grad_norm=10.0,
          clip_param=0.2, epochs=5, minibatches=4)


class Learner:
    """The parts of the reference's TRPO update that run on the device, written out for synthetic storage."""

    def __init__(self, ac, lr=1e-3):
        import torch
        self.ac = ac
        self.opt = torch.optim.Adam(ac.parameters(), lr=lr)
        self.line_search_calls = 0

    def flat(self):
        import torch
        return torch.cat([p.data.view(-1) for p in self.ac.actor.parameters()])

    def set_flat(self, x):
        i = 0
        for p in self.ac.actor.parameters():
            n = p.numel()
            p.data.copy_(x[i:i + n].view(p.size()))
            i += n

    def hvp(self, v, kl):
        import torch
        g = torch.autograd.grad(kl, self.ac.actor.parameters(), create_graph=True)
        fg = torch.cat([t.view(-1) for t in g])
        gg = torch.autograd.grad((fg * v).sum(), self.ac.actor.parameters(), retain_graph=True)
        return torch.cat([t.contiguous().view(-1) for t in gg]).detach() + HP["damping"] * v

    @staticmethod
    def kl(mu, sigma, old_mu, old_sigma):
        import torch
        return torch.sum(sigma - old_sigma + (torch.square(old_sigma.exp()) + torch.square(old_mu - mu)) / (2.0 * torch.square(sigma.exp())) - 0.5,
                         axis=-1, keepdim=True).mean()

    def cg(self, Av, b):
        import torch
        x, r, p = torch.zeros_like(b), b.clone(), b.clone()
        rr = torch.dot(r, r)
        for _ in range(HP["cg_nsteps"]):
            av = Av(p)
            alpha = rr / torch.dot(p, av)
            x += alpha * p
            r -= alpha * av
            nrr = torch.dot(r, r)
            if nrr < 1e-10:
                break
            p = r + nrr / rr * p
            rr = nrr
        return x

    def aloss(self, mb, old_logp):
        import torch
        with torch.no_grad():
            logp, _, _, _, _ = self.ac.evaluate(mb["obs"], None, mb["act"])
            loss = (-mb["adv"].squeeze() * torch.exp(logp - old_logp.squeeze())).mean()
        return loss, logp.unsqueeze(-1)

    def minibatch(self, mb):
        import torch
        logp, _, value, mu, sigma = self.ac.evaluate(mb["obs"], None, mb["act"])
        a_loss = (-mb["adv"].squeeze() * torch.exp(logp - mb["old_logp"].squeeze())).mean()
        g = torch.autograd.grad(a_loss, self.ac.actor.parameters(), retain_graph=True)
        flat_g = torch.cat([t.view(-1) for t in g]).detach()
        kl = self.kl(mu, sigma, mb["old_mu"], mb["old_sigma"])
        Av = lambda v: self.hvp(v, kl)                          # noqa: E731
        step = self.cg(Av, -flat_g)
        sAs = (step * Av(step)).sum(0)
        full = (torch.sqrt(2 * HP["max_kl"] / sAs) * step).data
        x0 = self.flat()
        f0, olp = self.aloss(mb, mb["old_logp"])
        expected = HP["accept_ratio"] * (-full * flat_g).sum(0, keepdim=True)
        alpha, new = HP["step_fraction"], x0
        for _ in range(HP["max_num_backtrack"]):
            self.line_search_calls += 1
            xn = x0 + alpha * full
            self.set_flat(xn)
            fn, olp = self.aloss(mb, olp)
            if (f0 - fn) > 0 and (f0 - fn) > alpha * expected:
                new = xn
                break
            alpha *= 0.5
        self.set_flat(new)
        self.aloss(mb, mb["old_logp"])
        for p in self.ac.actor.parameters():
            p.requires_grad = False
        vc = mb["values"] + (value - mb["values"]).clamp(-HP["clip_param"], HP["clip_param"])
        vloss = torch.max((value - mb["returns"]).pow(2), (vc - mb["returns"]).pow(2)).mean()
        self.opt.zero_grad()
        vloss.backward()
        torch.nn.utils.clip_grad_norm_(self.ac.critic.parameters(), HP["max_grad_norm"])
        self.opt.step()
        for p in self.ac.actor.parameters():
            p.requires_grad = True
        return step


def storage(rows, dev, seed=0):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)           # noqa: E731
    return {"obs": r(rows, 388).clamp(-5, 5), "act": r(rows, 80).clamp(-1, 1), "adv": r(rows, 1), "old_logp": r(rows, 1) - 60.0,
            "values": r(rows, 1), "returns": r(rows, 1)}


def timed(fn, warmup, repeats, reset=None):
    """Median of `repeats` timings of fn() between HIP events, after `warmup` untimed calls; reset() (untimed) before every call."""
    import torch
    for _ in range(warmup):
        if reset:
            reset()
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        if reset:
            reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("fused", "torch"), default=None)
    ap.add_argument("--skip-update", action="store_true", help="leave out (c)")
    args = ap.parse_args()
    import torch
    from massive_marl_benchmark_amd.algorithms.rl.trpo import ActorCritic

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    base = ActorCritic((388,), (388,), (80,), 0.8, CFG, fused_grad=True).to(dev)
    mb = storage(args.rows, dev)
    with torch.no_grad():
        old_mu = base.actor(mb["obs"])
        mb["old_mu"], mb["old_sigma"] = old_mu + 0.05 * torch.randn_like(old_mu), base.log_std.repeat(args.rows, 1).detach()
    results = {}
    for name in ("fused", "torch"):
        if args.only and name != args.only:
            continue
        ac = copy.deepcopy(base)
        ac.fused_grad = name == "fused"
        ln = Learner(ac)
        logp, _, _, mu, sigma = ac.evaluate(mb["obs"], None, mb["act"])
        kl = ln.kl(mu, sigma, mb["old_mu"], mb["old_sigma"])
        n = sum(p.numel() for p in ac.actor.parameters())
        v = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        hvp_ms, hvp_all = timed(lambda: ln.hvp(v, kl), args.warmup, args.repeats)
        del kl, logp, mu, sigma
        # every timed minibatch / update starts from the same parameters and optimizer state, so that the line searches repeat
        # the same number of backtracking steps (recorded per timing)
        state, opt_state = copy.deepcopy(ac.state_dict()), copy.deepcopy(ln.opt.state_dict())
        searches = []

        def reset():
            ac.load_state_dict(state)
            ln.opt.load_state_dict(opt_state)
            searches.append(ln.line_search_calls)

        mb_ms, mb_all = timed(lambda: ln.minibatch(mb), 1, max(3, args.repeats // 2), reset)
        mb_ls = [b - a for a, b in zip(searches, searches[1:] + [ln.line_search_calls])][1:]
        rec = {"path": name, "rows": args.rows, "hvp_ms": round(hvp_ms, 3), "minibatch_ms": round(mb_ms, 3),
               "hvp_all_ms": [round(t, 3) for t in hvp_all], "minibatch_all_ms": [round(t, 3) for t in mb_all], "minibatch_line_search_steps": mb_ls}
        if not args.skip_update:
            searches.clear()
            upd = lambda: [ln.minibatch(mb) for _ in range(HP["epochs"] * HP["minibatches"])]     # noqa: E731
            up_ms, up_all = timed(upd, 1, 3, reset)
            up_ls = [b - a for a, b in zip(searches, searches[1:] + [ln.line_search_calls])][1:]
            rec.update(update_ms=round(up_ms, 3), update_all_ms=[round(t, 3) for t in up_all], update_line_search_steps=up_ls)
        ac.load_state_dict(state)
        rec["device"] = torch.cuda.get_device_name(0)
        results[name] = rec
        print(json.dumps(rec), flush=True)
        del ac, ln
        torch.cuda.empty_cache()
    if len(results) == 2:
        f, t = results["fused"], results["torch"]
        ratio = {"metric": "trpo_update_speedup_torch_over_fused", "hvp": round(t["hvp_ms"] / f["hvp_ms"], 3),
                 "minibatch": round(t["minibatch_ms"] / f["minibatch_ms"], 3)}
        if "update_ms" in f:
            ratio["update"] = round(t["update_ms"] / f["update_ms"], 3)
        print(json.dumps(ratio), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for one `update()` of the REFERENCE's own PPO learner (agents/algorithms/rl/ppo/ppo.py), its ActorCritic and
RolloutStorage, imported in place with make_trpo_update_fixture.py's scaffolding (which is make_td3_update_fixture.py's).  Nothing of
the reference is copied.  CPU.

Setup: make_trpo_update_fixture.py's sizes, behaviour policy, rollout and start (obs 12, act 4, hidden (64, 64) ELU, 16 envs x 4 steps,
2 epochs x 2 minibatches; the start is the behaviour policy plus seeded noise, in bf16 values), cfg/ppo/config.yaml's values otherwise
but max_grad_norm (the script ASSERTS a clip coefficient below 1 in every step) and an entropy coefficient that is not zero.  The
minibatches' kl_mean lie near 0.033: with the config's desired_kl 0.016 the schedule lowers the step size or keeps it, with 0.068 it
raises or keeps it (both ASSERTED), so the two variants take the schedule's three branches between them.

Each variant runs the same update in fp32 and in float64 (`torch.set_default_dtype(torch.float64)` around construction and update):
  ref        the adaptive schedule, the plain value loss
  clipped    use_clipped_value_loss on, desired_kl 0.068

The schedule decides by comparison: per minibatch the script recomputes the reference's kl_mean from what its `evaluate` returned (the
same torch expression in the run's precision) and ASSERTS that none lies within a relative 1e-3 of either threshold (2 desired_kl,
desired_kl / 2), that none is 0, and that fp32 and float64 take the same step sizes.

Stored (ppo_learner_update.npz): the start, the rollout's tensors, the index lists, and per run `<variant><32|64>_`: loss (what backward() was
called on), kl, step_size (after every minibatch), norms (what clip_grad_norm_ returned), means; `_proj`, `_norm` and `<variant>_err`
as in trpo_learner_update.npz.

    MMS_REFERENCE=<reference tree> python tests/golden/make_ppo_update_fixture.py
"""
import os
import sys

import numpy as np
import torch

import make_trpo_update_fixture as mt

HERE = mt.HERE
LEARN = dict(optim_stepsize=3e-4, nsteps=mt.T, cliprange=0.2, ent_coef=0.01, noptepochs=2, nminibatches=2, max_grad_norm=0.5, gamma=0.96, lam=0.95,
             init_noise_std=0.8, desired_kl=0.016, schedule="adaptive")
VARIANTS = {"ref": {}, "clipped": dict(use_clipped_value_loss=True, desired_kl=0.068)}
BAND = 1e-3


def run(Learner, env, variant, start, rollout, double):
    learn = dict(LEARN, **VARIANTS[variant])
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    try:
        agent = mt.prepare(Learner, env, learn, "ppo", start, rollout, double)
        rec = dict(loss=[], norms=[], kl=[], step_size=[], batch=None, evaluated=[])
        gen, ev, opt_step = agent.storage.mini_batch_generator, agent.actor_critic.evaluate, agent.optimizer.step

        def batches(n):
            rec["batch"] = [list(b) for b in gen(n)]
            return rec["batch"]

        def evaluate(*a, **k):
            r = ev(*a, **k)
            rec["evaluated"].append((r[3].detach().clone(), r[4].detach().clone()))
            return r

        def step(*a, **k):
            rec["step_size"].append(float(agent.step_size))
            assert all(g["lr"] == agent.step_size for g in agent.optimizer.param_groups)
            return opt_step(*a, **k)

        agent.storage.mini_batch_generator, agent.actor_critic.evaluate, agent.optimizer.step = batches, evaluate, step
        clip, backward = torch.nn.utils.clip_grad_norm_, torch.Tensor.backward
        torch.nn.utils.clip_grad_norm_ = lambda params, max_norm: (lambda v: (rec["norms"].append(v.detach().clone()), v)[1])(clip(params, max_norm))

        def recorded_backward(self, *a, **k):
            rec["loss"].append(self.detach().clone())
            return backward(self, *a, **k)
        torch.Tensor.backward = recorded_backward
        try:
            means = agent.update()
        finally:
            torch.nn.utils.clip_grad_norm_, torch.Tensor.backward = clip, backward
        after = list(agent.actor_critic.state_dict().items())
        # kl_mean of every minibatch, as the schedule saw it
        old_mu, old_sigma = agent.storage.mu.view(-1, mt.A), agent.storage.sigma.view(-1, mt.A)
        order = rec["batch"] * learn["noptepochs"]
        for idx, (mu, sigma) in zip(order, rec["evaluated"]):
            om, os_ = old_mu[idx], old_sigma[idx]
            rec["kl"].append(torch.sum(sigma - os_ + (torch.square(os_.exp()) + torch.square(om - mu)) / (2.0 * torch.square(sigma.exp())) - 0.5,
                                       axis=-1).mean())
    finally:
        torch.set_default_dtype(torch.float32)
    steps = learn["noptepochs"] * learn["nminibatches"]
    assert len(rec["loss"]) == len(rec["norms"]) == len(rec["kl"]) == len(rec["step_size"]) == steps
    coef = [learn["max_grad_norm"] / (float(v) + 1e-6) for v in rec["norms"]]
    assert max(coef) < 1.0, ("a step does not clip", coef)
    d = learn["desired_kl"]
    for kl in rec["kl"]:
        kl = float(kl)
        assert kl > 0.0 and abs(kl / (2.0 * d) - 1.0) > BAND and abs(kl / (d / 2.0) - 1.0) > BAND, ("a kl_mean the schedule cannot decide by", kl)
    return dict(rec=rec, means=means, after=after, coef=coef)


def main():
    if not mt.REF or not os.path.isdir(mt.REF):
        sys.exit("set MMS_REFERENCE to the reference tree")
    mt.setup_imports()
    env = mt.make_env()
    # the rollout and the start are TRPO's: one behaviour policy, one data set for both learners (the two modules are the same file)
    start, rollout = mt.collect(mt.learner_class("trpo"), env, mt.LEARN, "trpo")
    Learner = mt.learner_class("ppo")
    runs = {(v, d): run(Learner, env, v, start, rollout, d) for v in VARIANTS for d in (False, True)}
    out = {}
    mt.start_arrays(start, rollout, out)
    out["batch"] = np.array(runs[("ref", False)]["rec"]["batch"], np.int64)
    out["variants"] = np.array(list(VARIANTS))
    for (variant, double), r in runs.items():
        tag, rec = variant + ("64" if double else "32"), r["rec"]
        assert rec["batch"] == runs[("ref", False)]["rec"]["batch"]
        for k in ("loss", "norms", "kl"):
            out[tag + "_" + k] = torch.stack(rec[k]).numpy()
        out[tag + "_step_size"] = np.array(rec["step_size"], np.float64)
        out[tag + "_means"] = np.array(r["means"], np.float64)
        mt.after_arrays(tag, r["after"], out)
    for variant in VARIANTS:
        r32, r64 = runs[(variant, False)], runs[(variant, True)]
        assert r32["rec"]["step_size"] == r64["rec"]["step_size"], ("fp32 and float64 take different step sizes", variant)
        sizes = r32["rec"]["step_size"]
        moves = {(b > a) - (b < a) for a, b in zip([LEARN["optim_stepsize"]] + sizes[:-1], sizes)}
        assert moves == ({-1, 0} if variant == "ref" else {1, 0}), ("the schedule lost a branch", variant, sizes)
        out[variant + "_err"] = np.array([float((x.double() - y).norm() / y.norm()) for (_, x), (_, y) in zip(r32["after"], r64["after"])])
        out[variant + "_learn_keys"] = np.array(list(VARIANTS[variant].keys()))
        out[variant + "_learn_values"] = np.array([float(v) for v in VARIANTS[variant].values()])
        print("ppo", variant, "kl", ["%.4g" % float(k) for k in r32["rec"]["kl"]], "step sizes", ["%.3g" % s for s in sizes], "clip coefficients",
              ["%.3f" % c for c in r32["coef"]], "worst fp32 error %.3g" % out[variant + "_err"].max())
    out["learn_keys"] = np.array([k for k, v in LEARN.items() if not isinstance(v, str)])
    out["learn_values"] = np.array([float(v) for v in LEARN.values() if not isinstance(v, str)])
    out["seeds"] = np.array([mt.SEED_INIT, mt.SEED_DATA, mt.SEED_START, mt.SEED_SIGNS, mt.PROJ])
    out["meta"] = np.array("one update() of the reference's PPO (rl/ppo/ppo.py) imported in place, fp32 and float64, per variant of "
                           "make_ppo_update_fixture.py")
    path = os.path.join(HERE, "ppo_learner_update.npz")
    np.savez_compressed(path, **out)
    print("wrote ppo_learner_update.npz (%d arrays, %d bytes)" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for one TRPO minibatch: the REFERENCE's own agents/algorithms/rl/trpo/trpo.py and module.py, imported in place with
the name-only stubs of run_reference_learners.py (nothing copied), on the CPU in fp32.  The actor obs 20 -> [32, 24, 16] ELU -> 6 is
constructed after torch.manual_seed(3); 40 rows of observations / actions / advantages; old_mu, old_sigma and the old log-probabilities
come from that actor, and then its parameters are moved (N(0, 0.02 mean|p|) per tensor) so that mu != old_mu, as in every minibatch
after the first.  The TRPO methods run on an instance whose __init__ is skipped (no vec_env), with cfg/trpo's damping, cg_nsteps,
max_kl, max_num_backtrack, accept_ratio and step_fraction.  Stored: the moved state_dict, the minibatch, flat_g (trpo.py:290), a
direction v and kl_hessian_times_vector(v) (:417-435), the CG step_dir (:300), sAs and full_step (:303-305), the line search's
outcome and the actor's flat parameters after set_pi_flat_params (:309-313).  Writes tests/golden/trpo_update.npz.

    python tests/golden/make_trpo_fixture.py
"""
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import run_reference_learners as rrl  # noqa: E402

OBS, ACT, HIDDEN, ROWS, SEED = 20, 6, [32, 24, 16], 40, 3


def main():
    if not os.path.isdir(rrl.REF):
        sys.exit("reference tree not present")
    rrl.setup_imports()
    pkg = types.ModuleType("agents.algorithms.rl.trpo")
    pkg.__path__ = [os.path.join(rrl.REF, "agents/algorithms/rl/trpo")]
    sys.modules["agents.algorithms.rl.trpo"] = pkg
    st = rrl.load("agents.algorithms.rl.trpo.storage", "agents/algorithms/rl/trpo/storage.py")
    mod = rrl.load("agents.algorithms.rl.trpo.module", "agents/algorithms/rl/trpo/module.py")
    pkg.RolloutStorage, pkg.ActorCritic = st.RolloutStorage, mod.ActorCritic
    trpo = rrl.load("agents.algorithms.rl.trpo.trpo", "agents/algorithms/rl/trpo/trpo.py")
    learn = yaml.safe_load(open(os.path.join(rrl.REF, "cfg", "trpo", "config.yaml")))["learn"]
    cfg = {"pi_hid_sizes": HIDDEN, "vf_hid_sizes": HIDDEN, "activation": "elu"}
    torch.manual_seed(SEED)
    ac = mod.ActorCritic((OBS,), (OBS,), (ACT,), learn["init_noise_std"], cfg)
    g = torch.Generator().manual_seed(100 + SEED)
    obs, act, adv = torch.randn(ROWS, OBS, generator=g), torch.randn(ROWS, ACT, generator=g), torch.randn(ROWS, 1, generator=g)
    with torch.no_grad():
        old_logp, _, _, old_mu, old_sigma = ac.evaluate(obs, None, act)
        old_logp = old_logp.unsqueeze(-1)
        for p in ac.actor.parameters():
            p.add_(0.02 * p.abs().mean() * torch.randn(p.shape, generator=g))
    sd = {k: v.clone() for k, v in ac.state_dict().items()}
    t = trpo.TRPO.__new__(trpo.TRPO)
    t.actor_critic, t.device = ac, "cpu"
    for k in ("damping", "cg_nsteps", "max_kl", "max_num_backtrack", "accept_ratio", "step_fraction"):
        setattr(t, k, learn[k])
    # trpo.py:283-313, step by step
    logp, _, _, mu, sigma = ac.evaluate(obs, None, act)
    a_loss = (-torch.squeeze(adv) * torch.exp(logp - torch.squeeze(old_logp))).mean()
    grads = torch.autograd.grad(a_loss, ac.actor.parameters(), retain_graph=True)
    flat_g = torch.cat([x.view(-1) for x in grads]).detach()
    kl = torch.mean(torch.sum(sigma - old_sigma + (torch.square(old_sigma.exp()) + torch.square(old_mu - mu)) / (2.0 * torch.square(sigma.exp())) - 0.5,
                              axis=-1, keepdim=True))
    Av = lambda x: t.kl_hessian_times_vector(x, kl)          # noqa: E731
    v = torch.randn(flat_g.numel(), generator=g)
    hv = Av(v)
    step_dir = t.conjugate_gradient(Av, -flat_g, nsteps=t.cg_nsteps)
    sAs = (step_dir * Av(step_dir)).sum(0)
    full_step = (torch.sqrt(2 * t.max_kl / sAs) * step_dir).data
    evaluate_policy = lambda x: t.get_aloss_logp(obs, None, act, adv, old_actions_log_prob_batch=x)   # noqa: E731
    success, new_params = t.line_search(evaluate_policy, full_step, old_logp, flat_g, max_num_backtrack=t.max_num_backtrack,
                                        accept_ratio=t.accept_ratio, step_fraction=t.step_fraction)
    t.set_pi_flat_params(new_params)
    out = {"keys": np.array(list(sd.keys())), "obs": obs.numpy(), "actions": act.numpy(), "advantages": adv.numpy(), "old_logp": old_logp.numpy(),
           "old_mu": old_mu.numpy(), "old_sigma": old_sigma.numpy(), "v": v.numpy(), "flat_g": flat_g.numpy(), "hv": hv.detach().numpy(),
           "step_dir": step_dir.detach().numpy(), "sAs": sAs.detach().numpy(), "full_step": full_step.numpy(), "success": np.bool_(success),
           "params_after": t.get_pi_flat_params().numpy(), "shape": np.array([OBS, *HIDDEN, ACT]),
           "hyper": np.array([learn[k] for k in ("init_noise_std", "damping", "cg_nsteps", "max_kl", "max_num_backtrack", "accept_ratio", "step_fraction")],
                             dtype=np.float64)}
    for i, x in enumerate(sd.values()):
        out["sd%d" % i] = x.numpy()
    out["meta"] = np.array("reference TRPO (agents/algorithms/rl/trpo/trpo.py) one minibatch in fp32 on the CPU: ELU actor obs 20 -> [32, 24, 16] "
                           "-> 6, 40 rows, parameters moved off old_mu; hyper = init_noise_std, damping, cg_nsteps, max_kl, max_num_backtrack, "
                           "accept_ratio, step_fraction (cfg/trpo/config.yaml)")
    np.savez_compressed(os.path.join(HERE, "trpo_update.npz"), **out)
    print("wrote trpo_update.npz (%d arrays), line search %s" % (len(out), "accepted" if success else "failed"))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the HATRPO trainer: the REFERENCE's own HATRPO.trpo_update (agents/algorithms/marl/hatrpo_trainer.py:181-319,
imported in place, CPU, fp32) on its own HATRPO_Policy (hatrpo_policy.py: the reference's Actor and Critic with Adam), one minibatch of
256 rows, obs 46 -> 64 x 3 -> 8 actions, share_obs 60, parameters perturbed (tests/marl_modules.randomize).  Two cases, named in
CASES below: one whose line search accepts at its third try (accept_ratio 0.965: this seed's improvement ratio is 0.946, 0.955, 0.973 --
the KL at the full step stays under kl_threshold for every seed tried, because the step is scaled with the damped product), one that
it rejects (accept_ratio 2: the improvement ratio tends to 1).
Stored per case: the config as JSON, both state_dicts before the update, the sample, the seven returned values, the number of
line-search tries (counted through update_model) and the actor's and the critic's parameters afterwards.  Before writing, the float64
statement of the same update (tests/hatrpo_check.actor_update) is run on the same inputs and its decision margins are printed: a seed is
kept only when they are far from the thresholds.  Runs where the reference tree is; writes tests/golden/hatrpo_update.npz (plain arrays).

    python tests/golden/make_hatrpo_fixture.py
"""
import io
import contextlib
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import run_reference_learners as rrl          # the import scaffolding (name-only gym / isaacgym / tensorboard stand-ins)
import hatrpo_check as hc
from marl_modules import randomize

M, OBS, SHARE, ACT, HIDDEN = 256, 46, 60, 8, 64
# name: (seed, config overrides, advantage scale)
CASES = {"later": (11, {"accept_ratio": 0.965}, 1.0),
         "rejected": (4, {"accept_ratio": 2.0}, 1.0)}
KEEP = ("kl_threshold", "ls_step", "accept_ratio", "clip_param", "num_mini_batch", "data_chunk_length", "value_loss_coef", "entropy_coef", "max_grad_norm",
        "huber_delta", "use_recurrent_policy", "use_naive_recurrent_policy", "use_max_grad_norm", "use_clipped_value_loss", "use_huber_loss", "use_popart",
        "use_value_active_masks", "use_policy_active_masks", "lr", "critic_lr", "opti_eps", "weight_decay", "hidden_size", "layer_N", "std_x_coef",
        "std_y_coef")


def main():
    if not os.path.isdir(rrl.REF):
        sys.exit("reference tree not present")
    rrl.setup_imports()
    rrl.load("agents.algorithms.marl.actor_critic", "agents/algorithms/marl/actor_critic.py")
    pol = rrl.load("agents.algorithms.marl.hatrpo_policy", "agents/algorithms/marl/hatrpo_policy.py")
    trn = rrl.load("agents.algorithms.marl.hatrpo_trainer", "agents/algorithms/marl/hatrpo_trainer.py")
    from gym import spaces                   # the name-only stand-in: Box with .shape
    out = {"cases": np.array(list(CASES))}
    for name, (seed, over, adv_scale) in CASES.items():
        conf = yaml.safe_load(open(os.path.join(rrl.REF, "cfg", "hatrpo", "config.yaml")))
        conf.update(hidden_size=HIDDEN, algorithm_name="hatrpo", data_chunk_length=1, **over)
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        policy = pol.HATRPO_Policy(conf, spaces.Box(low=-np.inf, high=np.inf, shape=(OBS,)), spaces.Box(low=-np.inf, high=np.inf, shape=(SHARE,)),
                                   spaces.Box(low=-1.0, high=1.0, shape=(ACT,)), torch.device("cpu"))
        randomize(policy.actor, gen)
        randomize(policy.critic, gen)
        sample = hc.make_sample(policy.actor, policy.critic, M, OBS, SHARE, seed + 100, adv_scale=adv_scale)
        for k, v in policy.actor.state_dict().items():
            out["%s.actor.%s" % (name, k)] = v.numpy().copy()
        for k, v in policy.critic.state_dict().items():
            out["%s.critic.%s" % (name, k)] = v.numpy().copy()
        # the float64 statement's margins on the same inputs
        cfg = {k: conf[k] for k in KEEP}
        r64 = hc.actor_update(hc.to_dtype(policy.actor, torch.float64), sample, cfg)
        r32 = hc.actor_update(policy.actor, sample, cfg)
        print("%s (seed %d): float64 tries %d accepted %s, margin %.3g, fp32 deviation %.3g; kl %s, ratio %s" % (
            name, seed, r64["tries"], r64["accepted"], hc.margins(r64, cfg), hc.deviation(r64, r32, cfg),
            ["%.4g" % k for k in r64["kl"]], ["%.3g" % (a / b) for a, b in zip(r64["loss_improve"], r64["expected_improve"])]))
        trainer = trn.HATRPO(conf, policy, torch.device("cpu"))
        tries = [0]
        update_model = trainer.update_model

        def counting(model, new_params, tries=tries, update_model=update_model, actor=policy.actor):
            tries[0] += model is actor
            update_model(model, new_params)
        trainer.update_model = counting
        rnn = np.zeros((M, 1, HIDDEN), np.float32)
        ref_sample = (sample[0].numpy(), sample[1].numpy(), rnn, rnn, sample[4].numpy(), sample[5].numpy(), sample[6].numpy(), np.ones((M, 1), np.float32),
                      sample[8].numpy(), sample[9].numpy(), sample[10].numpy(), None, sample[12].numpy())
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            value_loss, critic_grad_norm, kl, loss_improve, expected_improve, dist_entropy, ratio = trainer.trpo_update(ref_sample)
        accepted = "does not impove" not in said.getvalue()
        n_tries = tries[0] - (0 if accepted else 1)                   # the restore is one more update_model of the actor
        print("   reference: tries %d accepted %s kl %.5g loss_improve %.5g expected_improve %.5g" % (n_tries, accepted, float(kl), float(loss_improve),
                                                                                                     float(expected_improve[0])))
        for key, t in zip(("share_obs", "obs", "actions", "value_preds", "returns", "active_masks", "old_logp", "adv", "factor"),
                          (sample[0], sample[1], sample[4], sample[5], sample[6], sample[8], sample[9], sample[10], sample[12])):
            out["%s.%s" % (name, key)] = t.numpy().copy()
        out["%s.config" % name] = np.array(json.dumps(cfg))
        out["%s.returned" % name] = np.array([float(value_loss), float(critic_grad_norm), float(kl), float(loss_improve), float(expected_improve[0]),
                                              float(dist_entropy)], np.float64)
        out["%s.ratio" % name] = ratio.detach().numpy().copy()
        out["%s.tries" % name] = np.array(n_tries)
        out["%s.accepted" % name] = np.array(accepted)
        for k, v in policy.actor.state_dict().items():
            out["%s.actor_after.%s" % (name, k)] = v.numpy().copy()
        for k, v in policy.critic.state_dict().items():
            out["%s.critic_after.%s" % (name, k)] = v.numpy().copy()
    out["meta"] = np.array("reference HATRPO.trpo_update (hatrpo_trainer.py:181-319) on HATRPO_Policy, CPU fp32; <case>.returned = value_loss, "
                           "critic_grad_norm, kl, loss_improve, expected_improve, dist_entropy (last line-search try); <case>.ratio [M, 1]; "
                           "<case>.tries = line-search evaluations; <case>.config = the settings as JSON")
    np.savez_compressed(os.path.join(HERE, "hatrpo_update.npz"), **out)
    print("wrote hatrpo_update.npz (%d arrays)" % len(out))


if __name__ == "__main__":
    main()

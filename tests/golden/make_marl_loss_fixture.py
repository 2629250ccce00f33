#!/usr/bin/env python3
"""Golden vectors for the MAPPO / HAPPO update's loss head: the REFERENCE's own trainers (agents/algorithms/marl/mappo_trainer.py: MAPPO,
happo_trainer.py: HAPPO, imported in place, CPU) run on one minibatch of M = 64 rows and A = 8 actions over the flag combinations

    MAPPO: popart / valuenorm / neither  x  huber / mse  x  clipped value on / off  x  each mask flag on / off          (48 cases)
    HAPPO: popart / neither  x  each mask flag on / off, huber and clipped value on, with a factor                      (8 cases)

with huber_delta 0.5 (so that all three Huber branches occur) and an active mask that has zeros.  Each case calls the trainer's
`ppo_update` -- its surrogate lines and `cal_value_loss`, `huber_loss` / `mse_loss` -- on a stub policy whose `evaluate_actions` is the
reference's ACTLayer.evaluate_actions on a Box space (DiagGaussian with fc_mean = identity, so that its input is mu) next to a leaf
tensor of values; the stub's optimizers do nothing, so after the call the leaves hold autograd's gradients of
policy_loss - entropy_coef dist_entropy with respect to mu and log_std and of value_loss_coef value_loss with respect to values.
Stored: the inputs, per case the four returned scalars, imp_weights.mean() and the three gradients, and the state of a PopArt and a
ValueNorm after three cal_value_loss calls of a MAPPO trainer.  Runs where the reference tree is; writes tests/golden/marl_ppo_loss.npz
(plain arrays).

    python tests/golden/make_marl_loss_fixture.py
"""
import itertools
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MMS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
M, A = 64, 8
CLIP, DELTA, VALUE_COEF, ENTROPY_COEF = 0.2, 0.5, 0.7, 0.01


class Box:                                                            # ACTLayer looks at the class name and .shape
    def __init__(self, n):
        self.shape = (n,)


def cases():
    out = []
    for norm, huber, clipped, pm, vm in itertools.product(("none", "popart", "valuenorm"), (1, 0), (1, 0), (0, 1), (0, 1)):
        out.append(("mappo", norm, huber, clipped, pm, vm))
    for norm, pm, vm in itertools.product(("none", "popart"), (0, 1), (0, 1)):
        out.append(("happo", norm, 1, 1, pm, vm))
    return out


def config(norm, huber, clipped, pm, vm):
    return {"clip_param": CLIP, "ppo_epoch": 1, "num_mini_batch": 1, "data_chunk_length": 1, "value_loss_coef": VALUE_COEF, "entropy_coef": ENTROPY_COEF,
            "max_grad_norm": 10.0, "huber_delta": DELTA, "use_valuenorm": norm == "valuenorm", "use_popart": norm == "popart",
            "use_recurrent_policy": False, "use_naive_recurrent_policy": False, "use_max_grad_norm": True, "use_clipped_value_loss": bool(clipped),
            "use_huber_loss": bool(huber), "use_value_active_masks": bool(vm), "use_policy_active_masks": bool(pm),
            "actor_gain": 0.01, "std_x_coef": 1.0, "std_y_coef": 0.5}


def main():
    if not os.path.exists(os.path.join(REF, "agents", "algorithms", "marl", "mappo_trainer.py")):
        sys.exit("reference tree not present")
    sys.path.insert(0, REF)
    for name in ("agents", "agents.utils", "agents.algorithms", "agents.algorithms.utils", "agents.algorithms.marl", "agents.algorithms.marl.utils"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]             # namespace only: the packages' own __init__ (isaacgym) never runs
        sys.modules[name] = m
    from agents.algorithms.marl.happo_trainer import HAPPO
    from agents.algorithms.marl.mappo_trainer import MAPPO
    from agents.algorithms.utils.act import ACTLayer

    g = torch.Generator().manual_seed(20)
    rn = lambda *s: torch.randn(*s, generator=g)
    log_std = 0.2 * rn(A) + 1.0
    std = 0.5 * torch.sigmoid(log_std)
    mu, v = rn(M, A), rn(M, 1)
    actions = mu + std * rn(M, A)
    old_logp = torch.distributions.Normal(mu, std).log_prob(actions) + 0.3 / A ** 0.5 * rn(M, A)
    adv, vp, ret = rn(M, 1), v + 0.3 * rn(M, 1), v + rn(M, 1)
    masks = (torch.rand(M, 1, generator=g) > 0.25).float()
    factor = torch.exp(0.3 * rn(M, 1))
    assert 0 < int(masks.sum()) < M
    out = {"mu": mu, "log_std": log_std, "std": std, "value": v, "actions": actions, "old_logp": old_logp, "adv": adv, "value_preds": vp, "returns": ret,
           "active_masks": masks, "factor": factor}
    out = {k: t.numpy().copy() for k, t in out.items()}
    names, flags = [], []
    for i, (algo, norm, huber, clipped, pm, vm) in enumerate(cases()):
        cfg = config(norm, huber, clipped, pm, vm)
        act = ACTLayer(Box(A), A, True, 0.01, cfg)
        with torch.no_grad():
            act.action_out.fc_mean.weight.copy_(torch.eye(A))
            act.action_out.fc_mean.bias.zero_()
            act.action_out.log_std.copy_(log_std)
        mu_leaf, v_leaf = mu.clone().requires_grad_(True), v.clone().requires_grad_(True)

        def evaluate_actions(share_obs, obs, rnn_states, rnn_states_critic, action, masks_, available_actions, active_masks, pm=pm, act=act):
            logp, ent = act.evaluate_actions(mu_leaf, action, available_actions, active_masks=active_masks if pm else None)   # actor_critic.py:99-116
            return v_leaf, logp, ent

        nothing = types.SimpleNamespace(zero_grad=lambda: None, step=lambda: None)
        net = types.SimpleNamespace(parameters=lambda: [mu_leaf])
        policy = types.SimpleNamespace(evaluate_actions=evaluate_actions, actor_optimizer=nothing, critic_optimizer=nothing, actor=net, critic=net)
        cfg["max_grad_norm"] = 1e30                                    # the clip must not scale the recorded gradients
        trainer = (MAPPO if algo == "mappo" else HAPPO)(cfg, policy, torch.device("cpu"))
        sample = (None, None, None, None, actions, vp, ret, None, masks, old_logp, adv, None, factor if algo == "happo" else None)
        value_loss, _, policy_loss, dist_entropy, _, imp = trainer.ppo_update(sample, True)
        names.append("%s/%s/huber%d/clipped%d/pm%d/vm%d" % (algo, norm, huber, clipped, pm, vm))
        flags.append([algo == "happo", ("none", "popart", "valuenorm").index(norm), huber, clipped, pm, vm])
        out.update({"c%d_scalars" % i: np.array([policy_loss.item(), value_loss.item(), dist_entropy.item(), imp.mean().item()], np.float32),
                    "c%d_dmu" % i: mu_leaf.grad.numpy().copy(), "c%d_dlog_std" % i: act.action_out.log_std.grad.numpy().copy(),
                    "c%d_dvalue" % i: v_leaf.grad.numpy().copy()})
        if norm == "popart":
            n = trainer.value_normalizer
            out["c%d_norm_state" % i] = np.array([n.running_mean.item(), n.running_mean_sq.item(), n.debiasing_term.item()], np.float32)
    out["case_names"], out["case_flags"] = np.array(names), np.array(flags, np.int32)
    # the normalisers' state after three cal_value_loss calls on three different return batches
    batches = [ret, 1.5 * ret + 0.3, ret - 1.0]
    out["norm_batches"] = torch.stack(batches).numpy()
    for norm in ("popart", "valuenorm"):
        trainer = MAPPO(config(norm, 1, 1, 0, 0), None, torch.device("cpu"))
        for b in batches:
            trainer.cal_value_loss(v, vp, b, masks)
        n = trainer.value_normalizer
        mean, var = n.running_mean_var()
        out[norm + "_state3"] = np.array([n.running_mean.item(), n.running_mean_sq.item(), n.debiasing_term.item(), mean.item(), var.item()], np.float32)
    out["constants"] = np.array([CLIP, DELTA, VALUE_COEF, ENTROPY_COEF], np.float64)
    out["meta"] = np.array("reference MAPPO / HAPPO ppo_update (mappo_trainer.py:106-179, happo_trainer.py:89-170) with ACTLayer(Box).evaluate_actions on "
                           "DiagGaussian (fc_mean = identity, std_x_coef 1, std_y_coef 0.5), M 64, A 8; c<i>_scalars = policy_loss, value_loss, dist_entropy, "
                           "imp_weights.mean(); gradients of policy_loss - entropy_coef dist_entropy (mu, log_std) and value_loss_coef value_loss (value); "
                           "constants = clip, huber_delta, value_loss_coef, entropy_coef; case_flags = happo, norm (0 none, 1 popart, 2 valuenorm), huber, "
                           "clipped, policy masks, value masks")
    np.savez_compressed(os.path.join(HERE, "marl_ppo_loss.npz"), **out)
    print("wrote marl_ppo_loss.npz (%d arrays, %d cases)" % (len(out), len(names)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for recurrent MAPPO / HAPPO policies: the REFERENCE's own Actor and Critic (agents/algorithms/marl/actor_critic.py with
use_recurrent_policy = True, imported in place, CPU) with perturbed parameters -- two agents of TenAnt's shapes (obs 46, share_obs 388,
8 actions; hidden 64, layer_N 2, recurrent_N 2), each parameter then cut to 12 significant bits (still an fp32 number: the reference
runs on exactly what is stored; the zero low bits compress, which keeps the file under the repository's size limit).  Stored per
agent: both state_dicts; twelve input rows with states in (-1, 1) and masks with some zeros; the deterministic action, the value and
both new states of the single-step forward; and, over a [T = 4, N = 3] sequence whose masks have a zero at t = 2 (RNNLayer's has_zeros
branch, utils/rnn.py:43-69), evaluate_actions' log-probabilities and the critic's values.  Runs in the build container only; writes
tests/golden/marl_rnn_policy.npz (plain arrays).

    python tests/golden/make_marl_rnn_fixture.py
"""
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import run_reference_learners as rrl          # the import scaffolding (name-only gym / isaacgym / tensorboard stand-ins)
from marl_modules import randomize


def keep_12_bits(module):
    with torch.no_grad():
        for p in module.parameters():
            p.view(torch.int32).bitwise_and_(~0xFFF)


def main():
    if not os.path.isdir(rrl.REF):
        sys.exit("reference tree not present")
    rrl.setup_imports()
    ac = rrl.load("agents.algorithms.marl.actor_critic", "agents/algorithms/marl/actor_critic.py")
    from gym import spaces                   # the name-only stand-in: Box with .shape
    conf = yaml.safe_load(open(os.path.join(rrl.REF, "cfg", "mappo", "config.yaml")))
    conf.update(hidden_size=64, layer_N=2, algorithm_name="mappo", use_recurrent_policy=True, use_naive_recurrent_policy=False, recurrent_N=2)
    obs_space = spaces.Box(low=-np.inf, high=np.inf, shape=(46,))
    sobs_space = spaces.Box(low=-np.inf, high=np.inf, shape=(388,))
    act_space = spaces.Box(low=-1.0, high=1.0, shape=(8,))
    gen = torch.Generator().manual_seed(20261019)
    M, T, N, H, R = 12, 4, 3, 64, 2
    out = {"agents": np.array(2), "hidden": np.array(H), "layer_N": np.array(conf["layer_N"]), "recurrent_N": np.array(R), "T": np.array(T), "N": np.array(N)}
    uni = lambda *s: torch.rand(*s, generator=gen) * 1.98 - 0.99
    for i in range(2):
        torch.manual_seed(200 + i)
        actor = ac.Actor(conf, obs_space, act_space, torch.device("cpu"))
        critic = ac.Critic(conf, sobs_space, torch.device("cpu"))
        randomize(actor, gen)
        randomize(critic, gen)
        keep_12_bits(actor)
        keep_12_bits(critic)
        obs = torch.randn(M, 46, generator=gen) * 2.0
        sobs = torch.randn(M, 388, generator=gen) * 2.0
        rnn_a, rnn_c = uni(M, R, H), uni(M, R, H)
        masks = torch.ones(M, 1)
        masks[[1, 4, 5, 10]] = 0.0
        # the sequence: rows time-major ([T, N] flattened), one initial state per sequence, a zero mask at t = 2 (and one at t = 0)
        seq_obs = torch.randn(T * N, 46, generator=gen) * 2.0
        seq_sobs = torch.randn(T * N, 388, generator=gen) * 2.0
        seq_actions = torch.randn(T * N, 8, generator=gen)
        seq_rnn_a, seq_rnn_c = uni(N, R, H), uni(N, R, H)
        seq_masks = torch.ones(T, N, 1)
        seq_masks[2, 1] = 0.0
        seq_masks[0, 2] = 0.0
        seq_masks = seq_masks.reshape(T * N, 1)
        with torch.no_grad():
            action, _, new_a = actor(obs, rnn_a, masks, None, deterministic=True)
            value, new_c = critic(sobs, rnn_c, masks)
            seq_logp, _ = actor.evaluate_actions(seq_obs, seq_rnn_a, seq_actions, seq_masks)
            seq_values, _ = critic(seq_sobs, seq_rnn_c, seq_masks)
        for k, v in actor.state_dict().items():
            out["a%d.actor.%s" % (i, k)] = v.numpy()
        for k, v in critic.state_dict().items():
            out["a%d.critic.%s" % (i, k)] = v.numpy()
        put = {"obs": obs, "share_obs": sobs, "rnn_states": rnn_a, "rnn_states_critic": rnn_c, "masks": masks, "action": action, "value": value,
               "new_rnn_states": new_a, "new_rnn_states_critic": new_c, "seq_obs": seq_obs, "seq_share_obs": seq_sobs, "seq_actions": seq_actions,
               "seq_rnn_states": seq_rnn_a, "seq_rnn_states_critic": seq_rnn_c, "seq_masks": seq_masks, "seq_logp": seq_logp, "seq_values": seq_values}
        out.update({"a%d.%s" % (i, k): v.contiguous().numpy() for k, v in put.items()})
    np.savez_compressed(os.path.join(HERE, "marl_rnn_policy.npz"), **out)
    print("wrote marl_rnn_policy.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()

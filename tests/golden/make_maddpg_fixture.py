#!/usr/bin/env python3
"""Golden vectors for MADDPG: the REFERENCE's own `MADDPG_policy`, `MADDPG.cal_value_loss`, `cal_pi_loss`, `ddpg_update`, `train`
(agents/algorithms/marl/maddpg/module.py) and `ReplayBuffer` (storage.py), imported in place and run on the CPU.  (Its `Runner.run`
cannot execute -- train.py:25 says so -- and is not part of the fixture.)

Three agents, obs 10, share_obs 18, act 2 (critic input 18 + 3 * 2 = 24), hidden [64, 64], elu, 5 envs, replay_size 6, batch_size 4,
polyak 0.5, learning_rate 1e-2, gamma 0.99, max_grad_norm 1, num_learning_epochs 2 with one mini-batch (`train` breaks when
learn_ep >= num_learning_epochs: one update).  The small polyak and the large step are deliberate: inside `ddpg_update` agent nid's
target sees the target actors of agents < nid AFTER their polyak update, and these hyperparameters make that visible.

Stored: every policy's parameters (actor, critic, actor_targ, critic_targ; the targets are perturbed copies; everything rounded to 8
significant bits before anything is evaluated and stored as the upper 16 bits of the fp32 words); the eight transitions per agent
given to `ReplayBuffer.add_transitions` (replay_size 6: an overflow) and the rings they leave; the index list; per agent
`cal_value_loss` and `cal_pi_loss` at the initial parameters; the two loss lists `ddpg_update` returns; after that update each
agent's `actor_targ` and `critic` first-layer weight row 0 and last-layer bias; `train`'s returned dicts (same index list: the same
`random.seed`); and `value_loss_pre`, the value losses with ALL target actions taken before the loop (the reference's modules,
evaluated by this script: the critics' state at their own iteration, the target actors' initial state).

Nothing of the reference is copied: its modules are imported from where they lie (the tree named by MMS_REFERENCE) with
namespace-only `agents.*` packages and the name-only `gym.spaces` stand-in of tests/golden/_isaacgym_stub.  Writes
tests/golden/maddpg_update.npz (plain arrays).

    MMS_REFERENCE=<reference tree> python tests/golden/make_maddpg_fixture.py
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MMS_REFERENCE", "")
N_AGENTS, OBS, SOBS, ACT, HIDDEN, ENVS, RING, BATCH, STEPS = 3, 10, 18, 2, [64, 64], 5, 6, 4, 8
CONFIG = {"learning_rate": 1e-2, "hidden_size": HIDDEN, "activation": "elu", "act_noise": 0.1, "num_learning_epochs": 2, "num_mini_batch": 1,
          "gamma": 0.99, "polyak": 0.5, "max_grad_norm": 1.0, "n_rollout_threads": ENVS, "replay_size": RING, "batch_size": BATCH, "sampler": "random"}
NETS = ("actor", "critic", "actor_targ", "critic_targ")
SAMPLE_SEED = 5


def setup_imports():
    sys.path.insert(0, os.path.join(HERE, "_isaacgym_stub"))
    for name in ("agents", "agents.algorithms", "agents.algorithms.marl", "agents.algorithms.marl.maddpg", "agents.utils"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]         # namespace only: the packages' own __init__ never runs
        sys.modules[name] = m
    try:
        load("agents.utils.util", "agents/utils/util.py")
    except Exception:                                              # imported by module.py, used by nothing below
        util = types.ModuleType("agents.utils.util")
        util.get_gard_norm = lambda it: 0.0
        sys.modules["agents.utils.util"] = util


def load(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


def build(module):
    """The same policies and trainer on every call."""
    torch.manual_seed(21)
    g = torch.Generator().manual_seed(121)
    obs_space = types.SimpleNamespace(shape=(OBS,))
    sobs_space = types.SimpleNamespace(shape=(SOBS,))
    act_space = types.SimpleNamespace(shape=(ACT,), high=np.ones(ACT, np.float32))
    policies = [module.MADDPG_policy(CONFIG, obs_space, sobs_space, act_space, [act_space] * N_AGENTS) for _ in range(N_AGENTS)]
    with torch.no_grad():
        for po in policies:
            for online, targ in ((po.actor, po.actor_targ), (po.critic, po.critic_targ)):
                for p, pt in zip(online.parameters(), targ.parameters()):
                    pt.add_(0.05 * torch.randn(p.shape, generator=g))
                    p.copy_(p.bfloat16().float())                 # 8 significant bits: the stored parameters compress to half
                    pt.copy_(pt.bfloat16().float())
    return policies, module.MADDPG(CONFIG, policies, N_AGENTS)


def bf16_words(net):
    flat = torch.cat([v.reshape(-1) for v in net.state_dict().values()]).numpy()
    bits = flat.view(np.uint32)
    assert not (bits & 0xffff).any()
    return (bits >> 16).astype(np.uint16)


def samples_of(buffers, indices):
    """What MADDPG.train hands to ddpg_update (module.py:315-334)."""
    return [{"obs": b.obs[indices], "sobs": b.share_obs[indices], "act": b.actions[indices], "jact": b.joint_actions[indices], "r": b.rewards[indices],
             "obs2": b.next_observations[indices], "sobs2": b.next_share_obs[indices], "done": b.dones[indices]} for b in buffers]


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set MMS_REFERENCE to the reference tree")
    setup_imports()
    storage = load("agents.algorithms.marl.maddpg.storage", "agents/algorithms/marl/maddpg/storage.py")
    module = load("agents.algorithms.marl.maddpg.module", "agents/algorithms/marl/maddpg/module.py")
    out = {}

    policies, trainer = build(module)
    out["actor_keys"] = np.array(list(policies[0].actor.state_dict().keys()))
    out["critic_keys"] = np.array(list(policies[0].critic.state_dict().keys()))
    for i, po in enumerate(policies):
        for name in NETS:
            out["agent%d_%s_bf16" % (i, name)] = bf16_words(getattr(po, name))

    # the ring: eight transitions per agent into six rows
    g = torch.Generator().manual_seed(122)
    act_space = types.SimpleNamespace(shape=(ACT,))
    buffers = [storage.ReplayBuffer(CONFIG, (OBS,), (SOBS,), (ACT,), [act_space] * N_AGENTS) for _ in range(N_AGENTS)]
    fed = {k: [] for k in ("obs", "share_obs", "actions", "joint_actions", "rewards", "next_observations", "next_share_obs", "dones")}
    for t in range(STEPS):
        joint = torch.rand(ENVS, N_AGENTS * ACT, generator=g) * 2 - 1
        row = {k: [] for k in fed}
        for i in range(N_AGENTS):
            tr = {"obs": torch.randn(ENVS, OBS, generator=g), "share_obs": torch.randn(ENVS, SOBS, generator=g), "actions": joint[:, i * ACT:(i + 1) * ACT].clone(),
                  "joint_actions": joint, "rewards": torch.randn(ENVS, generator=g), "next_observations": torch.randn(ENVS, OBS, generator=g),
                  "next_share_obs": torch.randn(ENVS, SOBS, generator=g), "dones": (torch.rand(ENVS, generator=g) < 0.3).to(torch.uint8)}
            buffers[i].add_transitions(tr["obs"], tr["share_obs"], tr["actions"], tr["joint_actions"], tr["rewards"], tr["next_observations"], tr["next_share_obs"],
                                       tr["dones"])
            for k, v in tr.items():
                row[k].append(v)
        for k in fed:
            fed[k].append(torch.stack(row[k]))
    for k in fed:
        out["fed_" + k] = torch.stack(fed[k]).numpy()                # [STEPS, agents, ENVS, ...]
        out["ring_" + k] = torch.stack([getattr(b, k) for b in buffers]).numpy()      # [agents, RING, ENVS, ...]
    out["ring_step"] = np.array([b.step for b in buffers])
    out["ring_fullfill"] = np.array([b.fullfill for b in buffers])
    assert all(b.fullfill for b in buffers)
    d = out["ring_dones"]
    assert d.any() and not d.all()

    random.seed(SAMPLE_SEED)
    indices = buffers[0].mini_batch_generator(CONFIG["num_mini_batch"])[0]
    out["indices"] = np.array(indices)
    samples = samples_of(buffers, indices)

    # the two losses per agent at the initial parameters
    out["value_loss_init"] = np.array([trainer.cal_value_loss(samples, i).item() for i in range(N_AGENTS)], np.float64)
    out["pi_loss_init"] = np.array([trainer.cal_pi_loss(samples, i).item() for i in range(N_AGENTS)], np.float64)

    # ddpg_update; the value losses with all target actions taken BEFORE the loop ride along: critic nid is still at its initial
    # state when its loss is taken (it changes in its own iteration only), the target actors are the initial ones
    with torch.no_grad():
        jact2_pre = torch.cat([policies[v].actor_targ.pi(samples[v]["obs2"]) for v in range(N_AGENTS)], dim=-1)
    pre = []
    real = trainer.cal_value_loss

    def cal_value_loss(data, nid):
        with torch.no_grad():
            q = policies[nid].critic.q(data[nid]["sobs"], data[nid]["jact"])
            backup = data[nid]["r"] + CONFIG["gamma"] * (1 - data[nid]["done"]) * policies[nid].critic.q(data[nid]["sobs2"], jact2_pre)
            pre.append(((q - backup) ** 2).mean().item())
        return real(data, nid)
    trainer.cal_value_loss = cal_value_loss
    value_loss, policy_loss = trainer.ddpg_update(samples)
    out["value_loss_update"] = np.array([v.item() for v in value_loss], np.float64)
    out["pi_loss_update"] = np.array([v.item() for v in policy_loss], np.float64)
    out["value_loss_pre"] = np.array(pre, np.float64)
    for name in ("actor_targ", "critic"):
        nets = [list(getattr(po, name).state_dict().values()) for po in policies]
        out["post_%s_w0_row0" % name] = torch.stack([sd[0][0] for sd in nets]).numpy()
        out["post_%s_last_bias" % name] = torch.stack([sd[-1] for sd in nets]).numpy()

    # train on fresh, identical policies: the same index list
    policies, trainer = build(module)
    random.seed(SAMPLE_SEED)
    infos = trainer.train(buffers)
    assert len(infos) == N_AGENTS
    out["train_value_loss"] = np.array([d["value_loss"] for d in infos], np.float64)
    out["train_policy_loss"] = np.array([d["policy_loss"] for d in infos], np.float64)

    out["config"] = np.array(repr(CONFIG))
    out["shape"] = np.array([N_AGENTS, OBS, SOBS, ACT, *HIDDEN, ENVS, RING, BATCH])
    out["meta"] = np.array("reference MADDPG (agents/algorithms/marl/maddpg/module.py, storage.py) imported in place, CPU; parameters in state_dict key order, "
                           "flattened, fp32 word >> 16; targets = online + 0.05 N(0,1) before the rounding; act_limit 1; done stored uint8")
    np.savez_compressed(os.path.join(HERE, "maddpg_update.npz"), **out)
    print("wrote maddpg_update.npz (%d arrays)" % len(out))
    for k in ("value_loss_init", "value_loss_update", "value_loss_pre", "pi_loss_init", "pi_loss_update", "train_value_loss", "train_policy_loss"):
        print(k, out[k])


if __name__ == "__main__":
    main()

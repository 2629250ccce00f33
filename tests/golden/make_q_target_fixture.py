#!/usr/bin/env python3
"""Golden vectors for the off-policy Q target: the REFERENCE's own `SAC.compute_loss_q` (agents/algorithms/rl/sac/sac.py:367-389)
and `TD3.compute_loss_q` (td3/td3.py:353-380), imported in place and called unbound on a stub object that carries what the two
methods read: `actor_critic` and `actor_critic_targ` (the reference's own MLPActorCritics, default initialisation after
torch.manual_seed, the target a perturbed copy), `gamma`, and `entropy_coef` (SAC) / `target_noise = 0`, `noise_clip`, `act_limit`
(TD3: no draw enters the result).  For SAC the stub's online `pi` is replaced by a function returning the recorded `(a2, logp_a2)`,
so the sampled action is part of the fixture.  obs 12 / act 4 / hidden (64, 64), a batch of 4 x 16 rows; `r` float [4,16,1], `d`
uint8 [4,16,1] with both values present.

Stored per algorithm: the target's state dict (its keys, and all tensors flattened in key order as the upper 16 bits of their fp32
words: every parameter of both networks is rounded to 8 significant bits before anything is evaluated, so that the file stays
small), the batch, `a2` (and `logp_a2`), the online `q1`,
`q2` and the returned `loss_q`.  Nothing of the reference is copied: its modules are imported from where they lie (the tree named
by MMS_REFERENCE), with namespace-only `agents.*` packages, the name-only `gym.spaces` stand-in of tests/golden/_isaacgym_stub and a
name-only SummaryWriter.  Writes tests/golden/q_target.npz (plain arrays).

    MMS_REFERENCE=<reference tree> python tests/golden/make_q_target_fixture.py
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MMS_REFERENCE", "")
W, A, HIDDEN, LEAD = 12, 4, (64, 64), (4, 16)
GAMMA, ALPHA = 0.99, 0.2


def setup_imports():
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    sys.path.insert(0, os.path.join(HERE, "_isaacgym_stub"))
    for name in ("agents", "agents.algorithms", "agents.algorithms.rl", "agents.algorithms.rl.sac", "agents.algorithms.rl.td3"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]         # namespace only: the packages' own __init__ never runs
        sys.modules[name] = m
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None, "__getattr__": lambda self, n: (lambda *a, **k: None)})
    sys.modules["torch.utils.tensorboard"] = tb
    torch.utils.tensorboard = tb


def load(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


def learner_class(algo):
    pkg = sys.modules["agents.algorithms.rl.%s" % algo]
    storage = load("agents.algorithms.rl.%s.storage" % algo, "agents/algorithms/rl/%s/storage.py" % algo)
    module = load("agents.algorithms.rl.%s.module" % algo, "agents/algorithms/rl/%s/module.py" % algo)
    pkg.ReplayBuffer, pkg.MLPActorCritic = storage.ReplayBuffer, module.MLPActorCritic
    learner = load("agents.algorithms.rl.%s.%s" % (algo, algo), "agents/algorithms/rl/%s/%s.py" % (algo, algo))
    return getattr(learner, algo.upper()), module.MLPActorCritic


def perturbed_copy(ac, g):
    targ = copy.deepcopy(ac)
    with torch.no_grad():
        for p in targ.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
        for p in (*ac.parameters(), *targ.parameters()):
            p.copy_(p.bfloat16().float())                         # 8 significant bits: the stored parameters compress to half
    return targ


def batch(g):
    d = (torch.rand(*LEAD, 1, generator=g) < 0.3).to(torch.uint8)
    assert bool(d.any()) and not bool(d.all())
    return {"obs": torch.randn(*LEAD, W, generator=g), "act": torch.rand(*LEAD, A, generator=g) * 2 - 1, "r": torch.randn(*LEAD, 1, generator=g),
            "obs2": torch.randn(*LEAD, W, generator=g), "done": d}


def store(out, tag, ac, targ, data, extra):
    sd = targ.state_dict()                                        # the online network enters through its recorded q1, q2 (and a2) only
    out["%s_targ_keys" % tag] = np.array(list(sd.keys()))
    flat = torch.cat([v.reshape(-1) for v in sd.values()]).numpy()
    bits = flat.view(np.uint32)
    assert not (bits & 0xffff).any()
    out["%s_targ_bf16" % tag] = (bits >> 16).astype(np.uint16)    # every tensor in key order, flattened: the upper halves of the fp32 words
    for k, v in {**data, **extra}.items():
        out["%s_%s" % (tag, k)] = v.detach().numpy()


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set MMS_REFERENCE to the reference tree")
    setup_imports()
    obs_space = types.SimpleNamespace(shape=(W,))
    act_space = types.SimpleNamespace(shape=(A,), high=np.ones(A, np.float32))
    out = {}

    SAC, SacAC = learner_class("sac")
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(111)
    ac = SacAC(obs_space, act_space, hidden_sizes=HIDDEN)
    targ = perturbed_copy(ac, g)
    data = batch(g)
    with torch.no_grad():
        a2, logp_a2 = ac.pi(data["obs2"])
        q1, q2 = ac.q1(data["obs"], data["act"]), ac.q2(data["obs"], data["act"])
    online = types.SimpleNamespace(q1=ac.q1, q2=ac.q2, pi=lambda o2: (a2, logp_a2))          # the recorded draw
    stub = types.SimpleNamespace(actor_critic=online, actor_critic_targ=targ, gamma=GAMMA, entropy_coef=ALPHA)
    loss = SAC.compute_loss_q(stub, {**data, "done": data["done"].float()})
    store(out, "sac", ac, targ, data, {"a2": a2, "logp_a2": logp_a2, "q1": q1, "q2": q2, "loss_q": loss})

    TD3, Td3AC = learner_class("td3")
    torch.manual_seed(12)
    g = torch.Generator().manual_seed(112)
    ac = Td3AC(obs_space, act_space, 0.1, "cpu", hidden_sizes=HIDDEN)
    targ = perturbed_copy(ac, g)
    data = batch(g)
    with torch.no_grad():
        a2 = torch.clamp(targ.pi(data["obs2"]), -1.0, 1.0)          # what td3.py:361-367 gives with target_noise = 0
        q1, q2 = ac.q1(data["obs"], data["act"]), ac.q2(data["obs"], data["act"])
    stub = types.SimpleNamespace(actor_critic=ac, actor_critic_targ=targ, gamma=GAMMA, target_noise=0.0, noise_clip=0.5, act_limit=1.0)
    loss = TD3.compute_loss_q(stub, {**data, "done": data["done"].float()})
    store(out, "td3", ac, targ, data, {"a2": a2, "q1": q1, "q2": q2, "loss_q": loss})

    out["gamma"], out["alpha"], out["shape"] = np.float64(GAMMA), np.float64(ALPHA), np.array([W, A, *HIDDEN])
    out["meta"] = np.array("reference SAC.compute_loss_q (rl/sac/sac.py:367-389) and TD3.compute_loss_q (rl/td3/td3.py:353-380), the learner files "
                           "imported in place and the methods called unbound on a stub; the reference's MLPActorCritics (ELU / ReLU, act_limit 1), "
                           "target = copy + 0.05 N(0,1), all parameters rounded to bf16 values before "
                           "evaluation; only the target's state dict is stored (<tag>_targ_bf16: fp32 word >> 16, key order, flattened); SAC: online pi replaced by the recorded (a2, logp_a2); TD3: target_noise 0; gamma 0.99, "
                           "entropy_coef 0.2; done stored uint8, given to the reference as float")
    np.savez_compressed(os.path.join(HERE, "q_target.npz"), **out)
    print("wrote q_target.npz (%d arrays)" % len(out))


if __name__ == "__main__":
    main()

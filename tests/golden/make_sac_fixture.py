#!/usr/bin/env python3
"""Golden vectors for SAC's MLPActorCritic: the REFERENCE's own module (agents/algorithms/rl/sac/module.py, imported in place,
CPU) at two small shapes, obs 52 / act 24 / hidden (64, 64) and obs 60 / act 8 / hidden (128, 128), constructed right after
torch.manual_seed(seed) with its default initialisation.  Stored per shape: the state_dict (key names and tensors), 64 observation
rows (40 N(0, 1) rows, then 24 rows scaled by 30 .. 3000 that push log_std past both clamp bounds and saturate tanh), the
deterministic pi(o) outputs (action and logp), act(o, deterministic=True) and q1 / q2 on (o, deterministic action).  Runs in the
build container only; writes tests/golden/sac_actor.npz (plain arrays).

    python tests/golden/make_sac_fixture.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MMS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = (("a", 52, 24, (64, 64), 5), ("b", 60, 8, (128, 128), 6))      # tag, obs, act, hidden, torch seed


def main():
    path = os.path.join(REF, "agents", "algorithms", "rl", "sac", "module.py")
    if not os.path.exists(path):
        sys.exit("reference tree not present")
    spec = importlib.util.spec_from_file_location("ref_sac_module", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for tag, W, A, hidden, seed in SHAPES:
        torch.manual_seed(seed)
        ac = mod.MLPActorCritic(types.SimpleNamespace(shape=(W,)), types.SimpleNamespace(shape=(A,), high=np.ones(A, np.float32)),
                                hidden_sizes=hidden)
        g = torch.Generator().manual_seed(100 + seed)
        o = torch.randn(64, W, generator=g)
        o[40:] *= torch.tensor([30.0, 300.0, 3000.0]).repeat(8)[:, None]
        with torch.no_grad():
            a, logp = ac.pi(o, deterministic=True)
            act = ac.act(o, deterministic=True)
            q1, q2 = ac.q1(o, a), ac.q2(o, a)
            ls = ac.pi.log_std_layer(ac.pi.net(o))
            mu = ac.pi.mu_layer(ac.pi.net(o))
        assert (ls < mod.LOG_STD_MIN).any() and (ls > mod.LOG_STD_MAX).any() and (mu.abs() > 10).any(), tag
        sd = ac.state_dict()
        out[tag + "_keys"] = np.array(list(sd.keys()))
        for i, v in enumerate(sd.values()):
            out["%s_sd%d" % (tag, i)] = v.numpy()
        out.update({tag + "_seed": np.int64(seed), tag + "_shape": np.array([W, A, *hidden]), tag + "_obs": o.numpy(), tag + "_action": a.numpy(),
                    tag + "_logp": logp.numpy(), tag + "_act": act.numpy(), tag + "_q1": q1.numpy(), tag + "_q2": q2.numpy()})
    out["meta"] = np.array("reference SquashedGaussianMLPActor / MLPActorCritic (agents/algorithms/rl/sac/module.py), ELU, act_limit 1, "
                           "default init after torch.manual_seed(<tag>_seed); pi(o, deterministic=True) with logp, act(o, True), q1 / q2")
    np.savez_compressed(os.path.join(HERE, "sac_actor.npz"), **out)
    print("wrote sac_actor.npz (%d arrays)" % len(out))


if __name__ == "__main__":
    main()

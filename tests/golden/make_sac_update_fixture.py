#!/usr/bin/env python3
"""Golden vectors for one `update()` of the REFERENCE's own SAC learner (agents/algorithms/rl/sac/sac.py), its MLPActorCritic and its
ReplayBuffer, imported in place with make_q_target_fixture.py's scaffolding (namespace-only `agents.*` packages, the name-only gym of
tests/golden/_isaacgym_stub, a name-only SummaryWriter).  Nothing of the reference is copied.  CPU.

Setup: obs 12, act 4, hidden (64, 64), 16 envs; replay_size 6 filled with 8 transitions (an overflow: the cursor goes 6 -> 1, 2);
batch_size 4, nminibatches 2, noptepochs 2; polyak 0.5, learning_rate 1e-2, ent_coef 0.2, gamma 0.99; max_grad_norm 0.05, for which
the script ASSERTS a clip coefficient below 1 in both steps of every minibatch.  Parameters are rounded to 8 significant bits (bf16
values) before anything is evaluated and stored as the upper 16 bits of their fp32 words, as the other fixtures do.

The noise is recorded: a `Normal` subclass is assigned to the reference module's `Normal` name; its `rsample` draws eps from a seeded
generator in the first run, keeps it, and replays it in the others (cast to the run's dtype).

Four runs of the same update, each from a freshly constructed learner:
  ref      the reference as it is (the freeze loops iterate an exhausted chain), fp32
  freeze   `sac.q_params = list(...)` assigned on the constructed object: the freeze loops do what the comments say, fp32
  and each of the two again in float64 -- the yardstick: `actor_critic.double()`, `actor_critic_targ.double()` and the rings
  assigned as double tensors on the reference's own objects, the recorded eps cast to double.

Stored: the transitions and the rings they leave (with the cursor and `fullfill`), the index lists (`random.seed(SEED_BATCH)` before
`update()`), every eps, and per run the per-minibatch loss_q and loss_pi, the norms that both
clip_grad_norm_ calls of every minibatch return, and the two returned means.

What is NOT stored element by element is the parameters after the update: 32276 values per run (actor_critic and actor_critic_targ)
in four runs, two of them in double, are 775 KB against the 162 KB this file may have (maddpg_update.npz).  Instead, per tensor of
both state dicts and per run: `<run>_proj` -- PROJ float64 inner products of the tensor with seeded +-1 vectors (`signs`: the test
regenerates them) -- and `<run>_norm`, its float64 2-norm; and per tensor `<variant>_err`, the reference's own fp32 error against its
float64 run as a relative norm.  A test evaluates this package's default route in float64 on the recorded eps, anchors that run to
the reference's float64 run through the projections (a difference d in a tensor moves a projection by about |d|, so 1e-9 relative
pins every element that matters), and then has the element-wise yardstick the tolerance rule needs.

    MMS_REFERENCE=<reference tree> python tests/golden/make_sac_update_fixture.py
"""
import importlib.util
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MMS_REFERENCE", "")
W, A, HIDDEN, ENVS = 12, 4, (64, 64), 16
REPLAY, FILLED = 6, 8
LEARN = dict(learning_rate=1e-2, replay_size=REPLAY, batch_size=4, nsteps=2, hidden_nodes=HIDDEN[0], hidden_layer=len(HIDDEN), noptepochs=2,
             nminibatches=2, ent_coef=0.2, gamma=0.99, polyak=0.5, max_grad_norm=0.05, reward_scale=1.0)
SEED_INIT, SEED_DATA, SEED_EPS, SEED_BATCH, SEED_SIGNS, PROJ = 21, 22, 23, 24, 25, 8


def setup_imports():
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    sys.path.insert(0, os.path.join(HERE, "_isaacgym_stub"))
    for name in ("agents", "agents.algorithms", "agents.algorithms.rl", "agents.algorithms.rl.sac"):
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


def signs(numel, index):
    """The PROJ +-1 vectors of tensor `index` (its place in the concatenated state dicts)."""
    return np.random.RandomState(1000 * SEED_SIGNS + index).randint(0, 2, (PROJ, numel)).astype(np.float64) * 2 - 1


def transitions():
    g = torch.Generator().manual_seed(SEED_DATA)
    out = []
    for t in range(FILLED):
        done = (torch.rand(ENVS, generator=g) < 0.3).to(torch.uint8)
        out.append(dict(obs=torch.randn(ENVS, W, generator=g), states=torch.randn(ENVS, W, generator=g), act=torch.rand(ENVS, A, generator=g) * 2 - 1,
                        rew=torch.randn(ENVS, generator=g), obs2=torch.randn(ENVS, W, generator=g), done=done))
    return out


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set MMS_REFERENCE to the reference tree")
    setup_imports()
    import gym.spaces as spaces
    pkg = sys.modules["agents.algorithms.rl.sac"]
    storage = load("agents.algorithms.rl.sac.storage", "agents/algorithms/rl/sac/storage.py")
    module = load("agents.algorithms.rl.sac.module", "agents/algorithms/rl/sac/module.py")
    pkg.ReplayBuffer, pkg.MLPActorCritic = storage.ReplayBuffer, module.MLPActorCritic
    learner = load("agents.algorithms.rl.sac.sac", "agents/algorithms/rl/sac/sac.py")
    SAC = learner.SAC

    recorded, cursor = [], [0]
    eps_gen = torch.Generator().manual_seed(SEED_EPS)
    mode = {"record": True}

    class RecordedNormal(module.Normal):
        def rsample(self, sample_shape=torch.Size()):
            if mode["record"]:
                recorded.append(torch.randn(self.loc.shape, generator=eps_gen))
            eps = recorded[cursor[0]]
            cursor[0] += 1
            assert eps.shape == self.loc.shape
            return self.loc + eps.to(self.loc.dtype) * self.scale

    module.Normal = RecordedNormal

    env = types.SimpleNamespace(observation_space=spaces.Box(-np.inf, np.inf, (W,)), state_space=spaces.Box(-np.inf, np.inf, (W,)),
                                action_space=spaces.Box(-1.0, 1.0, (A,)), num_envs=ENVS, task=types.SimpleNamespace(cfg={"seed": 0}))
    trans = transitions()
    out = {}

    def run(freeze, double):
        torch.manual_seed(SEED_INIT)
        sac = SAC(env, {"learn": dict(LEARN)}, device="cpu", log_dir=os.path.join(tempfile.gettempdir(), "sac_fixture"), print_log=False)
        with torch.no_grad():
            for p in sac.actor_critic.parameters():
                p.copy_(p.bfloat16().float())
            sac.actor_critic_targ.load_state_dict(sac.actor_critic.state_dict())
        init = {k: v.clone() for k, v in sac.actor_critic.state_dict().items()}
        if freeze:
            sac.q_params = list(sac.actor_critic.q1.parameters()) + list(sac.actor_critic.q2.parameters())
        for t in trans:
            sac.storage.add_transitions(t["obs"], t["states"], t["act"], t["rew"], t["obs2"], t["done"])
        rings = {k: getattr(sac.storage, k).clone() for k in ("observations", "states", "actions", "rewards", "next_observations", "dones")}
        if double:
            sac.actor_critic.double()
            sac.actor_critic_targ.double()
            for k in ("observations", "states", "actions", "rewards", "next_observations"):
                setattr(sac.storage, k, getattr(sac.storage, k).double())
        rec = dict(loss_q=[], loss_pi=[], norms=[], batch=None)
        lq, lp, gen = sac.compute_loss_q, sac.compute_loss_pi, sac.storage.mini_batch_generator
        sac.compute_loss_q = lambda data: (lambda v: (rec["loss_q"].append(v.detach().clone()), v)[1])(lq(data))
        sac.compute_loss_pi = lambda data: (lambda v: (rec["loss_pi"].append(v.detach().clone()), v)[1])(lp(data))

        def batches(n):
            rec["batch"] = gen(n)
            return rec["batch"]
        sac.storage.mini_batch_generator = batches
        clip = torch.nn.utils.clip_grad_norm_
        torch.nn.utils.clip_grad_norm_ = lambda params, max_norm: (lambda v: (rec["norms"].append(v.detach().clone()), v)[1])(clip(params, max_norm))
        mode["record"] = not recorded
        cursor[0] = 0
        random.seed(SEED_BATCH)
        try:
            means = sac.update()
        finally:
            torch.nn.utils.clip_grad_norm_ = clip
        assert cursor[0] == len(recorded) == 2 * LEARN["noptepochs"] * LEARN["nminibatches"]
        coef = [LEARN["max_grad_norm"] / (float(v) + 1e-6) for v in rec["norms"]]
        assert len(coef) == 8 and max(coef) < 1.0, coef             # both steps of every minibatch clip
        after = list(sac.actor_critic.state_dict().items()) + [("targ." + k, v) for k, v in sac.actor_critic_targ.state_dict().items()]
        return dict(init=init, rings=rings, step=sac.storage.step, fullfill=sac.storage.fullfill, rec=rec, means=means, after=after, coef=coef)

    runs = {(f, d): run(f, d) for f in (False, True) for d in (False, True)}
    base = runs[(False, False)]
    for r in runs.values():                                         # the same start, data and index lists in every run
        assert r["rec"]["batch"] == base["rec"]["batch"] and all(torch.equal(r["init"][k], v) for k, v in base["init"].items())

    sd = base["init"]
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(n) for n in v.shape) for v in sd.values()])
    bits = torch.cat([v.reshape(-1) for v in sd.values()]).numpy().view(np.uint32)
    assert not (bits & 0xffff).any()
    out["init_bf16"] = (bits >> 16).astype(np.uint16)
    for k in ("obs", "states", "act", "rew", "obs2", "done"):
        out["trans_" + k] = torch.stack([t[k] for t in trans]).numpy()
    for k, v in base["rings"].items():
        out["ring_" + k] = v.numpy()
    out["ring_step"], out["ring_fullfill"] = np.int64(base["step"]), np.bool_(base["fullfill"])
    out["batch"] = np.array(base["rec"]["batch"], np.int64)
    out["eps"] = torch.stack(recorded).numpy()
    out["after_keys"] = np.array([k for k, _ in base["after"]])
    for (freeze, double), r in runs.items():
        tag = ("freeze" if freeze else "ref") + ("64" if double else "32")
        out[tag + "_loss_q"] = torch.stack(r["rec"]["loss_q"]).numpy()
        out[tag + "_loss_pi"] = torch.stack(r["rec"]["loss_pi"]).numpy()
        out[tag + "_norms"] = torch.stack(r["rec"]["norms"]).numpy()
        out[tag + "_means"] = np.array(r["means"], np.float64)
        out[tag + "_proj"] = np.stack([signs(v.numel(), i) @ v.double().reshape(-1).numpy() for i, (_, v) in enumerate(r["after"])])
        out[tag + "_norm"] = np.array([float(v.double().norm()) for _, v in r["after"]])
    for freeze in (False, True):
        tag = "freeze" if freeze else "ref"
        a32, a64 = runs[(freeze, False)]["after"], runs[(freeze, True)]["after"]
        out[tag + "_err"] = np.array([float((x.double() - y).norm() / y.norm()) for (_, x), (_, y) in zip(a32, a64)])
        print(tag, "clip coefficients", ["%.3f" % c for c in runs[(freeze, False)]["coef"]], "worst fp32 error %.3g" % out[tag + "_err"].max())
    out["learn_keys"], out["learn_values"] = np.array(list(LEARN.keys())), np.array([float(v) for v in LEARN.values()])
    out["seeds"] = np.array([SEED_INIT, SEED_DATA, SEED_EPS, SEED_BATCH, SEED_SIGNS, PROJ])
    out["meta"] = np.array("one update() of the reference's SAC (rl/sac/sac.py) imported in place, fp32 and float64, as it is (ref) and with "
                           "sac.q_params assigned a list (freeze); see make_sac_update_fixture.py")
    path = os.path.join(HERE, "sac_update.npz")
    np.savez_compressed(path, **out)
    print("wrote sac_update.npz (%d arrays, %d bytes)" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "maddpg_update.npz"))


if __name__ == "__main__":
    main()

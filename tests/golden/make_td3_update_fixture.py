#!/usr/bin/env python3
"""Golden vectors for one `update()` of the REFERENCE's own TD3 and DDPG learners (agents/algorithms/rl/td3/td3.py, ddpg/ddpg.py), their
MLPActorCritic and ReplayBuffer, imported in place with make_sac_update_fixture.py's scaffolding (namespace-only `agents.*` packages,
the name-only gym of tests/golden/_isaacgym_stub, a name-only SummaryWriter).  Nothing of the reference is copied.  CPU.

Setup (make_sac_update_fixture.py's sizes): obs 12, act 4, hidden (64, 64), 16 envs; replay_size 6 filled with 8 transitions (an
overflow: the cursor goes 6 -> 1, 2); batch_size 4, nminibatches 2, noptepochs 2; polyak 0.5, learning_rate 1e-2, gamma 0.99,
target_noise 0.2, noise_clip 0.5, act_noise 0.1; max_grad_norm 0.002, for which the script ASSERTS a clip coefficient below 1 in every
step.  Parameters are rounded to 8 significant bits (bf16 values) before anything is evaluated and stored as the upper 16 bits of their
fp32 words.

The smoothing noise is recorded: `torch.randn_like` is replaced for the duration of `update()`, the way clip_grad_norm_ is; the
replacement draws the normals from a seeded generator in the first run of an algorithm, keeps them, and replays them in the others
(cast to the run's dtype).

Runs of the same update per algorithm, each from a freshly constructed learner, each in fp32 and in float64 (the yardstick:
`actor_critic.double()`, `actor_critic_targ.double()` and the rings assigned as double tensors on the reference's own objects):
  ref      the reference as it is: policy_delay 2 divides nminibatches, so TD3's policy step runs in every epoch; the freeze loops
           iterate an exhausted chain / generator
  freeze   `q_params = list(...)` assigned on the constructed object: the freeze loops do what the comments say
  skip     TD3 only: policy_delay 3 does not divide nminibatches, so no policy step runs and the mean surrogate loss is 0

Stored per file (td3_update.npz, ddpg_update.npz): the transitions and the rings they leave (with the cursor and `fullfill`), the index
lists (`random.seed(SEED_BATCH)` before `update()`), every recorded normal, and per run the losses of every step, the norms that every
clip_grad_norm_ call returns and the two returned means; the parameters after the update as in sac_update.npz -- per tensor of both
state dicts `<run>_proj` (PROJ float64 inner products with seeded +-1 vectors), `<run>_norm`, and per variant `<variant>_err`, the
reference's own fp32 error against its float64 run as a relative norm.

    MMS_REFERENCE=<reference tree> python tests/golden/make_td3_update_fixture.py
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
             nminibatches=2, gamma=0.99, polyak=0.5, max_grad_norm=0.002, reward_scale=1.0, policy_delay=2, target_noise=0.2, act_noise=0.1,
             noise_clip=0.5)
SKIP_DELAY = 3
SEED_INIT, SEED_DATA, SEED_EPS, SEED_BATCH, SEED_SIGNS, PROJ = 31, 32, 33, 34, 35, 8


def setup_imports():
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    sys.path.insert(0, os.path.join(HERE, "_isaacgym_stub"))
    for name in ("agents", "agents.algorithms", "agents.algorithms.rl", "agents.algorithms.rl.td3", "agents.algorithms.rl.ddpg"):
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


def make(algo, env, trans):
    """All runs of one algorithm; writes <algo>_update.npz."""
    pkg = sys.modules["agents.algorithms.rl." + algo]
    storage = load("agents.algorithms.rl.%s.storage" % algo, "agents/algorithms/rl/%s/storage.py" % algo)
    module = load("agents.algorithms.rl.%s.module" % algo, "agents/algorithms/rl/%s/module.py" % algo)
    pkg.ReplayBuffer, pkg.MLPActorCritic = storage.ReplayBuffer, module.MLPActorCritic
    learner = load("agents.algorithms.rl.%s.%s" % (algo, algo), "agents/algorithms/rl/%s/%s.py" % (algo, algo))
    Learner = getattr(learner, algo.upper())

    recorded, cursor = [], [0]
    eps_gen = torch.Generator().manual_seed(SEED_EPS)
    mode = {"record": True}

    def recorded_randn_like(t, **kw):
        assert not kw
        if mode["record"]:
            recorded.append(torch.randn(t.shape, generator=eps_gen))
        eps = recorded[cursor[0]]
        cursor[0] += 1
        assert eps.shape == t.shape
        return eps.to(t.dtype)

    def run(variant, double):
        torch.manual_seed(SEED_INIT)
        learn = dict(LEARN, policy_delay=SKIP_DELAY if variant == "skip" else LEARN["policy_delay"])
        agent = Learner(env, {"learn": learn}, device="cpu", log_dir=os.path.join(tempfile.gettempdir(), algo + "_fixture"), print_log=False)
        with torch.no_grad():
            for p in agent.actor_critic.parameters():
                p.copy_(p.bfloat16().float())
            agent.actor_critic_targ.load_state_dict(agent.actor_critic.state_dict())
        init = {k: v.clone() for k, v in agent.actor_critic.state_dict().items()}
        critics = [agent.actor_critic.q] if algo == "ddpg" else [agent.actor_critic.q1, agent.actor_critic.q2]
        if variant == "freeze":
            agent.q_params = [p for q in critics for p in q.parameters()]
        for t in trans:
            agent.storage.add_transitions(t["obs"], t["states"], t["act"], t["rew"], t["obs2"], t["done"])
        rings = {k: getattr(agent.storage, k).clone() for k in ("observations", "states", "actions", "rewards", "next_observations", "dones")}
        if double:
            agent.actor_critic.double()
            agent.actor_critic_targ.double()
            for k in ("observations", "states", "actions", "rewards", "next_observations"):
                setattr(agent.storage, k, getattr(agent.storage, k).double())
        rec = dict(loss_q=[], loss_pi=[], norms=[], batch=None)
        lq, lp, gen = agent.compute_loss_q, agent.compute_loss_pi, agent.storage.mini_batch_generator
        agent.compute_loss_q = lambda data: (lambda v: (rec["loss_q"].append(v.detach().clone()), v)[1])(lq(data))
        agent.compute_loss_pi = lambda data: (lambda v: (rec["loss_pi"].append(v.detach().clone()), v)[1])(lp(data))

        def batches(n):
            rec["batch"] = gen(n)
            return rec["batch"]
        agent.storage.mini_batch_generator = batches
        clip, randn_like = torch.nn.utils.clip_grad_norm_, torch.randn_like
        torch.nn.utils.clip_grad_norm_ = lambda params, max_norm: (lambda v: (rec["norms"].append(v.detach().clone()), v)[1])(clip(params, max_norm))
        torch.randn_like = recorded_randn_like
        mode["record"] = not recorded
        cursor[0] = 0
        random.seed(SEED_BATCH)
        try:
            means = agent.update()
        finally:
            torch.nn.utils.clip_grad_norm_, torch.randn_like = clip, randn_like
        epochs = LEARN["noptepochs"]
        pi_steps = 0 if variant == "skip" else epochs
        assert cursor[0] == len(recorded) == epochs and len(rec["loss_q"]) == epochs and len(rec["loss_pi"]) == pi_steps
        coef = [LEARN["max_grad_norm"] / (float(v) + 1e-6) for v in rec["norms"]]
        assert len(coef) == epochs + pi_steps and max(coef) < 1.0, coef       # every step clips
        if variant == "skip":
            assert means[1] == 0
        after = list(agent.actor_critic.state_dict().items()) + [("targ." + k, v) for k, v in agent.actor_critic_targ.state_dict().items()]
        return dict(init=init, rings=rings, step=agent.storage.step, fullfill=agent.storage.fullfill, rec=rec, means=means, after=after, coef=coef)

    variants = ("ref", "freeze") + (("skip",) if algo == "td3" else ())
    runs = {(v, d): run(v, d) for v in variants for d in (False, True)}
    base = runs[("ref", False)]
    for r in runs.values():                                         # the same start, data and index lists in every run
        assert r["rec"]["batch"] == base["rec"]["batch"] and all(torch.equal(r["init"][k], v) for k, v in base["init"].items())

    out = {}
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
    out["variants"] = np.array(variants)
    for (variant, double), r in runs.items():
        tag = variant + ("64" if double else "32")
        out[tag + "_loss_q"] = torch.stack(r["rec"]["loss_q"]).numpy()
        out[tag + "_loss_pi"] = torch.stack(r["rec"]["loss_pi"]).numpy() if r["rec"]["loss_pi"] else np.zeros(0, np.float64 if double else np.float32)
        out[tag + "_norms"] = torch.stack(r["rec"]["norms"]).numpy()
        out[tag + "_means"] = np.array(r["means"], np.float64)
        out[tag + "_proj"] = np.stack([signs(v.numel(), i) @ v.double().reshape(-1).numpy() for i, (_, v) in enumerate(r["after"])])
        out[tag + "_norm"] = np.array([float(v.double().norm()) for _, v in r["after"]])
    for variant in variants:
        a32, a64 = runs[(variant, False)]["after"], runs[(variant, True)]["after"]
        out[variant + "_err"] = np.array([float((x.double() - y).norm() / y.norm()) for (_, x), (_, y) in zip(a32, a64)])
        print(algo, variant, "clip coefficients", ["%.3f" % c for c in runs[(variant, False)]["coef"]], "worst fp32 error %.3g" % out[variant + "_err"].max())
    learn = dict(LEARN, skip_policy_delay=SKIP_DELAY)
    out["learn_keys"], out["learn_values"] = np.array(list(learn.keys())), np.array([float(v) for v in learn.values()])
    out["seeds"] = np.array([SEED_INIT, SEED_DATA, SEED_EPS, SEED_BATCH, SEED_SIGNS, PROJ])
    out["meta"] = np.array("one update() of the reference's %s (rl/%s/%s.py) imported in place, fp32 and float64, per variant of "
                           "make_td3_update_fixture.py" % (algo.upper(), algo, algo))
    path = os.path.join(HERE, algo + "_update.npz")
    np.savez_compressed(path, **out)
    print("wrote %s_update.npz (%d arrays, %d bytes)" % (algo, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "maddpg_update.npz"))


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set MMS_REFERENCE to the reference tree")
    setup_imports()
    import gym.spaces as spaces
    env = types.SimpleNamespace(observation_space=spaces.Box(-np.inf, np.inf, (W,)), state_space=spaces.Box(-np.inf, np.inf, (W,)),
                                action_space=spaces.Box(-1.0, 1.0, (A,)), num_envs=ENVS, task=types.SimpleNamespace(cfg={"seed": 0}))
    trans = transitions()
    for algo in ("td3", "ddpg"):
        make(algo, env, trans)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for one `update()` of the REFERENCE's own TRPO learner (agents/algorithms/rl/trpo/trpo.py), its ActorCritic and
RolloutStorage, imported in place with make_td3_update_fixture.py's scaffolding (namespace-only `agents.*` packages, the name-only gym
of tests/golden/_isaacgym_stub, a name-only SummaryWriter; `matplotlib.pyplot`, which trpo.py imports, is stubbed only if its import
fails).  Nothing of the reference is copied.  CPU.  make_ppo_update_fixture.py imports this file's scaffolding.

Setup: obs 12, act 4, hidden (64, 64) ELU, 16 envs x 4 steps, 2 epochs x 2 minibatches (the sequential sampler: rows 0..31 and 32..63),
cfg/trpo/config.yaml's values otherwise but max_grad_norm, for which the script ASSERTS a clip coefficient below 1 in every critic step.
The rollout is collected in fp32 by a behaviour policy (the freshly constructed module, its parameters rounded to bf16 values) through
the reference's own `evaluate`, `add_transitions` and `compute_returns`; the update starts from parameters that are the behaviour's
plus seeded noise, rounded to bf16 values again and stored as the upper 16 bits of their fp32 words -- so mu != old_mu from the first
minibatch on and the curvature term of the KL's Hessian is live everywhere.

Each variant runs the same update in fp32 and in float64 from the same start and the same stored rollout.  The float64 run is made with
`torch.set_default_dtype(torch.float64)` around construction and the update: otherwise conjugate_gradient's `torch.zeros(b.size())`
keeps x in fp32 and the yardstick is not one.
  ref        the config's step_fraction 0.1, max_kl 0.1, accept_ratio 0.01, cg_nsteps 3
  backtrack  step_fraction 1.0, max_kl 0.05, accept_ratio 0.9: trials that hand their log-probabilities on and (ASSERTED) acceptance
             after more than two trials in every minibatch
  clipped    use_clipped_value_loss on, max_kl 0.02, cg_nsteps 5

What the script asserts, per variant and precision:
  * every v . Av of kl_hessian_times_vector is positive (once the policy has moved the KL's Hessian can be indefinite, and the
    reference then takes the square root of a negative number);
  * over the variants the line search takes every branch: acceptance at the first trial, acceptance after backtracking, and a failure
    after max_num_backtrack trials, which keeps x0 (with this data the `ref` variant has one);
  * the line search decides by comparison: the decision and the number of trials agree between fp32 and float64, and every trial's
    |margin|, margin = (f0 - fnew) - alpha expected_improve, exceeds 1e-4 in both.

Stored (trpo_learner_update.npz): the start (`keys`, `shapes`, `init_bf16`), the rollout's tensors, the index lists, and per run
`<variant><32|64>_`: value_loss, norms (what clip_grad_norm_ returned), surrogate (every a_loss get_aloss_logp returned, in call order),
success, trials, margins (flat, in trial order), vAv (flat), means; the parameters after the update as in td3_update.npz -- `_proj`
(PROJ float64 inner products with seeded +-1 vectors per tensor), `_norm` -- and per variant `<variant>_err`, the reference's own fp32
error against its float64 run as a relative norm per tensor (0 for log_std, which the update leaves untouched).

    MMS_REFERENCE=<reference tree> python tests/golden/make_trpo_update_fixture.py
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MMS_REFERENCE", "")
W, A, HIDDEN, ENVS, T = 12, 4, (64, 64), 16, 4
POLICY = {"pi_hid_sizes": list(HIDDEN), "vf_hid_sizes": list(HIDDEN), "activation": "elu"}
LEARN = dict(optim_stepsize=1e-3, nsteps=T, cliprange=0.2, noptepochs=2, nminibatches=2, max_grad_norm=0.5, gamma=0.99, lam=0.95, init_noise_std=0.8,
             damping=0.1, cg_nsteps=3, max_kl=0.1, max_num_backtrack=10, accept_ratio=0.01, step_fraction=0.1, schedule="adaptive")
VARIANTS = {"ref": {}, "backtrack": dict(step_fraction=1.0, max_kl=0.05, accept_ratio=0.9),
            "clipped": dict(use_clipped_value_loss=True, max_kl=0.02, cg_nsteps=5)}
NOISE = 0.02                  # the start's distance from the behaviour policy, per parameter element
SEED_INIT, SEED_DATA, SEED_START, SEED_SIGNS, PROJ = 31, 32, 36, 35, 8
MARGIN = 1e-4
FIELDS = ("observations", "states", "rewards", "actions", "dones", "actions_log_prob", "values", "returns", "advantages", "mu", "sigma")


def setup_imports(algos=("trpo", "ppo")):
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    sys.path.insert(0, os.path.join(HERE, "_isaacgym_stub"))
    for name in ("agents", "agents.algorithms", "agents.algorithms.rl") + tuple("agents.algorithms.rl." + a for a in algos):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]         # namespace only: the packages' own __init__ never runs
        sys.modules[name] = m
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None, "__getattr__": lambda self, n: (lambda *a, **k: None)})
    sys.modules["torch.utils.tensorboard"] = tb
    torch.utils.tensorboard = tb
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:                                               # trpo.py imports one name from it and never uses it
        mp, pp = types.ModuleType("matplotlib"), types.ModuleType("matplotlib.pyplot")
        pp.step, mp.pyplot = None, pp
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mp, pp


def load(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


def learner_class(algo):
    pkg = sys.modules["agents.algorithms.rl." + algo]
    storage = load("agents.algorithms.rl.%s.storage" % algo, "agents/algorithms/rl/%s/storage.py" % algo)
    module = load("agents.algorithms.rl.%s.module" % algo, "agents/algorithms/rl/%s/module.py" % algo)
    pkg.RolloutStorage, pkg.ActorCritic = storage.RolloutStorage, module.ActorCritic
    return getattr(load("agents.algorithms.rl.%s.%s" % (algo, algo), "agents/algorithms/rl/%s/%s.py" % (algo, algo)), algo.upper())


def make_env():
    import gym.spaces as spaces
    return types.SimpleNamespace(observation_space=spaces.Box(-np.inf, np.inf, (W,)), state_space=spaces.Box(-np.inf, np.inf, (0,)),
                                 action_space=spaces.Box(-1.0, 1.0, (A,)), num_envs=ENVS)


def signs(numel, index):
    """The PROJ +-1 vectors of tensor `index` (its place in the state dict)."""
    return np.random.RandomState(1000 * SEED_SIGNS + index).randint(0, 2, (PROJ, numel)).astype(np.float64) * 2 - 1


def construct(Learner, env, learn, algo):
    torch.manual_seed(SEED_INIT)
    return Learner(env, {"policy": POLICY, "learn": learn}, device="cpu", log_dir=os.path.join(tempfile.gettempdir(), algo + "_fixture"), print_log=False)


def collect(Learner, env, learn, algo):
    """(the behaviour policy's state dict, the update's start, the stored rollout), all fp32: see the module docstring."""
    agent = construct(Learner, env, learn, algo)
    ac = agent.actor_critic
    with torch.no_grad():
        for p in ac.parameters():
            p.copy_(p.bfloat16().float())
    g = torch.Generator().manual_seed(SEED_DATA)
    for t in range(T):
        obs, eps = torch.randn(ENVS, W, generator=g), torch.randn(ENVS, A, generator=g)
        with torch.no_grad():
            act = ac.actor(obs) + (2 * ac.log_std).exp() * eps
            logp, _, value, mu, sigma = ac.evaluate(obs, None, act)
        rew, done = torch.randn(ENVS, generator=g), torch.rand(ENVS, generator=g) < 0.2
        agent.storage.add_transitions(obs, torch.zeros(ENVS, 0), act, rew, done, value, logp, mu, sigma)
    agent.storage.compute_returns(torch.zeros(ENVS, 1), learn["gamma"], learn["lam"])
    rollout = {k: getattr(agent.storage, k).clone() for k in FIELDS}
    g = torch.Generator().manual_seed(SEED_START)
    start = {k: (v + NOISE * torch.randn(v.shape, generator=g)).bfloat16().float() for k, v in ac.state_dict().items()}
    return start, rollout


def prepare(Learner, env, learn, algo, start, rollout, double):
    """A freshly constructed learner at `start` with `rollout` stored, in the run's precision (the caller has set the default dtype)."""
    agent = construct(Learner, env, learn, algo)
    dtype = torch.float64 if double else torch.float32
    agent.actor_critic.load_state_dict({k: v.to(dtype) for k, v in start.items()})
    for k in FIELDS:
        setattr(agent.storage, k, rollout[k].clone() if k == "dones" else rollout[k].to(dtype))
    agent.storage.step = T
    assert all(p.dtype == dtype for p in agent.actor_critic.parameters())
    return agent


def after_arrays(tag, after, out):
    out[tag + "_proj"] = np.stack([signs(v.numel(), i) @ v.double().reshape(-1).numpy() for i, (_, v) in enumerate(after)])
    out[tag + "_norm"] = np.array([float(v.double().norm()) for _, v in after])


def start_arrays(start, rollout, out):
    out["keys"] = np.array(list(start.keys()))
    out["shapes"] = np.array([",".join(str(n) for n in v.shape) for v in start.values()])
    bits = torch.cat([v.reshape(-1) for v in start.values()]).numpy().view(np.uint32)
    assert not (bits & 0xffff).any()
    out["init_bf16"] = (bits >> 16).astype(np.uint16)
    for k, v in rollout.items():
        out["rollout_" + k] = v.numpy()


def run(Learner, env, variant, start, rollout, double):
    learn = dict(LEARN, **VARIANTS[variant])
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    try:
        agent = prepare(Learner, env, learn, "trpo", start, rollout, double)
        rec = dict(value_loss=[], norms=[], surrogate=[], search=[], vAv=[], batch=None)
        gen, ls, hv, gl = agent.storage.mini_batch_generator, agent.line_search, agent.kl_hessian_times_vector, agent.get_aloss_logp

        def batches(n):
            rec["batch"] = [list(b) for b in gen(n)]
            return rec["batch"]

        def line_search(evaluate_policy, full_step, olp, grad, **kw):
            losses = []

            def ev(x):
                r = evaluate_policy(x)
                losses.append(r[0].detach().clone())
                return r
            ok, xn = ls(ev, full_step, olp, grad, **kw)
            expected = kw["accept_ratio"] * (-full_step * grad).sum()
            margins = [float((losses[0] - f) - kw["step_fraction"] * 0.5 ** i * expected) for i, f in enumerate(losses[1:])]
            rec["search"].append(dict(ok=bool(ok), trials=len(margins), margins=margins))
            return ok, xn

        def hvp(v, kl):
            r = hv(v, kl)
            rec["vAv"].append(float((v * r).sum()))
            return r

        def aloss(*a, **k):
            r = gl(*a, **k)
            rec["surrogate"].append(r[0].detach().clone())
            return r

        agent.storage.mini_batch_generator, agent.line_search, agent.kl_hessian_times_vector, agent.get_aloss_logp = batches, line_search, hvp, aloss
        clip, backward = torch.nn.utils.clip_grad_norm_, torch.Tensor.backward
        torch.nn.utils.clip_grad_norm_ = lambda params, max_norm: (lambda v: (rec["norms"].append(v.detach().clone()), v)[1])(clip(params, max_norm))

        def recorded_backward(self, *a, **k):                       # the update's one backward(): the value loss
            rec["value_loss"].append(self.detach().clone())
            return backward(self, *a, **k)
        torch.Tensor.backward = recorded_backward
        try:
            before = agent.actor_critic.log_std.detach().clone()
            means = agent.update()
        finally:
            torch.nn.utils.clip_grad_norm_, torch.Tensor.backward = clip, backward
        assert torch.equal(before, agent.actor_critic.log_std.detach()), "the update moved log_std"
        after = list(agent.actor_critic.state_dict().items())
    finally:
        torch.set_default_dtype(torch.float32)
    steps = learn["noptepochs"] * learn["nminibatches"]
    assert len(rec["search"]) == len(rec["norms"]) == len(rec["value_loss"]) == steps
    assert min(rec["vAv"]) > 0.0, ("a curvature product is not positive", variant, double, rec["vAv"])
    coef = [learn["max_grad_norm"] / (float(v) + 1e-6) for v in rec["norms"]]
    assert max(coef) < 1.0, ("a critic step does not clip", coef)
    assert all(abs(m) > MARGIN for s in rec["search"] for m in s["margins"]), ("a margin is too small to decide by", rec["search"])
    return dict(rec=rec, means=means, after=after, coef=coef)


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set MMS_REFERENCE to the reference tree")
    setup_imports()
    env = make_env()
    Learner = learner_class("trpo")
    start, rollout = collect(Learner, env, LEARN, "trpo")
    runs = {(v, d): run(Learner, env, v, start, rollout, d) for v in VARIANTS for d in (False, True)}
    out = {}
    start_arrays(start, rollout, out)
    out["batch"] = np.array(runs[("ref", False)]["rec"]["batch"], np.int64)
    out["variants"] = np.array(list(VARIANTS))
    for (variant, double), r in runs.items():
        tag, rec = variant + ("64" if double else "32"), r["rec"]
        assert rec["batch"] == runs[("ref", False)]["rec"]["batch"]
        out[tag + "_norms"] = torch.stack(rec["norms"]).numpy()
        out[tag + "_value_loss"] = torch.stack(rec["value_loss"]).numpy()
        out[tag + "_surrogate"] = torch.stack(rec["surrogate"]).numpy()
        out[tag + "_success"] = np.array([s["ok"] for s in rec["search"]])
        out[tag + "_trials"] = np.array([s["trials"] for s in rec["search"]], np.int64)
        out[tag + "_margins"] = np.array([m for s in rec["search"] for m in s["margins"]], np.float64)
        out[tag + "_vAv"] = np.array(rec["vAv"], np.float64)
        out[tag + "_means"] = np.array(r["means"], np.float64)
        after_arrays(tag, r["after"], out)
    for variant in VARIANTS:
        r32, r64 = runs[(variant, False)], runs[(variant, True)]
        s32, s64 = r32["rec"]["search"], r64["rec"]["search"]
        assert [(s["ok"], s["trials"]) for s in s32] == [(s["ok"], s["trials"]) for s in s64], ("fp32 and float64 decide differently", variant)
        out[variant + "_err"] = np.array([float((x.double() - y).norm() / y.norm()) for (_, x), (_, y) in zip(r32["after"], r64["after"])])
        out[variant + "_learn_keys"] = np.array(list(VARIANTS[variant].keys()))
        out[variant + "_learn_values"] = np.array([float(v) for v in VARIANTS[variant].values()])
        print("trpo", variant, "decisions", [(s["ok"], s["trials"]) for s in s32], "smallest |margin| %.3g" % min(abs(m) for s in s32 + s64 for m in s["margins"]),
              "smallest vAv %.3g" % min(r32["rec"]["vAv"] + r64["rec"]["vAv"]), "clip coefficients", ["%.3f" % c for c in r32["coef"]],
              "worst fp32 error %.3g" % out[variant + "_err"].max(), "margin 32-64 diff %.3g" %
              max(abs(a - b) for x, y in zip(s32, s64) for a, b in zip(x["margins"], y["margins"])))
    searches = [s for v in VARIANTS for s in runs[(v, False)]["rec"]["search"]]
    assert any(not s["ok"] for s in searches) and any(s["ok"] and s["trials"] == 1 for s in searches), "a branch is not covered: change a seed or settings"
    assert all(s["ok"] and s["trials"] > 2 for s in runs[("backtrack", False)]["rec"]["search"]), "the backtrack variant accepts too early"
    out["learn_keys"] = np.array([k for k, v in LEARN.items() if not isinstance(v, str)])
    out["learn_values"] = np.array([float(v) for v in LEARN.values() if not isinstance(v, str)])
    out["seeds"] = np.array([SEED_INIT, SEED_DATA, SEED_START, SEED_SIGNS, PROJ])
    out["meta"] = np.array("one update() of the reference's TRPO (rl/trpo/trpo.py) imported in place, fp32 and float64, per variant of "
                           "make_trpo_update_fixture.py")
    path = os.path.join(HERE, "trpo_learner_update.npz")
    np.savez_compressed(path, **out)
    print("wrote trpo_learner_update.npz (%d arrays, %d bytes)" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()

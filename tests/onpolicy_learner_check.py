"""Checks of the PPO and TRPO learners (algorithms/rl/ppo/ppo.py, trpo/trpo.py), shared by test_onpolicy_learner.py (CPU build) and
test_onpolicy_learner_gpu.py.  The method is td3_learner_check.py's.

The fixtures (tests/golden/ppo_learner_update.npz, trpo_learner_update.npz; make_ppo_update_fixture.py, make_trpo_update_fixture.py) hold one update()
of the reference's own learners, fp32 and float64, per variant.  `fixture_update` evaluates this package's default route in float64
(torch's default dtype set around construction and update, as the makers do), ANCHORS it to the reference's float64 run -- every
projection and norm to 1e-9 of the tensor's norm; losses, clip norms, kl, margins and curvature products to 1e-9 relative; decisions,
trial counts and step sizes equal -- and then applies the rule: per tensor, the fp32 default route's relative-norm error against that
yardstick is at most 2 x the reference's own fp32 error (test_sac_learner.py's margin; a tensor the update leaves exactly as it was,
log_std under TRPO, has error 0 on both sides).

`route_errors` compares the opt-in routes with the default route from the same start on the same rollout, next to a float64 replay:
the same decisions and trial counts (TRPO) or step sizes (PPO), and td3_learner_check.route_errors' rule per tensor -- the default
route's own error below 1e-3, the opt-in route's at most 2 x the default route's."""
import copy
import os
import tempfile
import types

import numpy as np
import torch

import sac_learner_check as sl
import trpo_check as tk
from conftest import load_golden
from massive_marl_benchmark_amd.algorithms.rl.ppo import PPO
from massive_marl_benchmark_amd.algorithms.rl.trpo import TRPO
from massive_marl_benchmark_amd.algorithms.rl.trpo.heads import StoredRows, trpo_heads
from massive_marl_benchmark_amd.algorithms.rl.trpo.module import grad_flat
from massive_marl_benchmark_amd.spaces import Box

LEARNERS = {"ppo": PPO, "trpo": TRPO}
VARIANTS = [("ppo", "ref"), ("ppo", "clipped"), ("trpo", "ref"), ("trpo", "backtrack"), ("trpo", "clipped")]
INT_KEYS = ("nsteps", "noptepochs", "nminibatches", "cg_nsteps", "max_num_backtrack")
FIELDS = ("observations", "states", "rewards", "actions", "dones", "actions_log_prob", "values", "returns", "advantages", "mu", "sigma")
_err = sl._err
ADAM_EPS = sl.ADAM_EPS


def stub_env(W, A, envs, S=0):
    return types.SimpleNamespace(observation_space=Box(-np.inf, np.inf, (W,)), state_space=Box(-np.inf, np.inf, (S,)), action_space=Box(-1.0, 1.0, (A,)),
                                 num_envs=envs)


class default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


def _learn(fx, variant, **more):
    learn = {str(k): float(v) for k, v in zip(fx["learn_keys"], fx["learn_values"])}
    learn.update({str(k): float(v) for k, v in zip(fx[variant + "_learn_keys"], fx[variant + "_learn_values"])})
    for k in INT_KEYS:
        if k in learn:
            learn[k] = int(learn[k])
    learn["use_clipped_value_loss"] = bool(learn.get("use_clipped_value_loss", 0.0))
    learn["schedule"] = "adaptive"
    learn.update(more)
    return learn


def _policy(hidden=(64, 64)):
    return {"pi_hid_sizes": list(hidden), "vf_hid_sizes": list(hidden), "activation": "elu"}


def _trace_arrays(algo, trace):
    t = lambda k: torch.stack([r[k].detach().double().cpu().reshape(()) for r in trace])
    if algo == "ppo":
        return dict(loss=t("loss"), norms=t("norm"), kl=t("kl"), step_size=torch.tensor([r["step_size"] for r in trace], dtype=torch.float64))
    return dict(value_loss=t("value_loss"), norms=t("norm"), new_surrogate=t("surrogate_loss"), success=[bool(r["success"]) for r in trace],
                trials=[int(r["trials"]) for r in trace], margins=torch.tensor([m for r in trace for m in r["margins"]], dtype=torch.float64),
                vAv=torch.tensor([v for r in trace for v in r["vAv"]], dtype=torch.float64))


# ---- the default route against the reference's update ------------------------------------------------------------------------------------

def fixture_run(algo, fx, variant, double, **more):
    """One update() from the fixture's start on its rollout, on "cpu".  Returns what the fixture records."""
    T, envs, W = fx["rollout_observations"].shape
    A = fx["rollout_actions"].shape[-1]
    dtype = torch.float64 if double else torch.float32
    with default_dtype(dtype):
        torch.manual_seed(0)
        agent = LEARNERS[algo](stub_env(W, A, envs), {"policy": _policy(), "learn": _learn(fx, variant, **more)}, device="cpu",
                               log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)
        sd = agent.actor_critic.state_dict()
        assert list(sd.keys()) == [str(k) for k in fx["keys"]]                   # the reference's state_dict keys, in its order
        words = torch.from_numpy((fx["init_bf16"].astype(np.uint32) << 16).view(np.float32).copy())
        at = 0
        for k, v in sd.items():
            v.copy_(words[at:at + v.numel()].view(v.shape))
            at += v.numel()
        assert at == words.numel() and all(p.dtype == dtype for p in agent.actor_critic.parameters())
        for k in FIELDS:
            t = torch.from_numpy(fx["rollout_" + k])
            setattr(agent.storage, k, t.clone() if k == "dones" else t.to(dtype))
        agent.storage.step = T
        agent.trace = []
        lists = []
        gen = agent.storage.mini_batch_generator
        agent.storage.mini_batch_generator = lambda n: (lambda b: (lists.append([list(x) for x in b]), b)[1])(gen(n))
        means = agent.update()
    out = _trace_arrays(algo, agent.trace)
    out.update(batch=lists[0], means=means, after=list(agent.actor_critic.state_dict().items()))
    return out


def _signs(fx, numel, index):
    seed, proj = int(fx["seeds"][3]), int(fx["seeds"][4])
    return np.random.RandomState(1000 * seed + index).randint(0, 2, (proj, numel)).astype(np.float64) * 2 - 1


def _last_of_groups(values, trials):
    """The a_new_loss of every minibatch among the fixture's a_loss record: per minibatch a_old_loss, f0, one per trial, a_new_loss."""
    out, at = [], 0
    for n in trials:
        at += 3 + n
        out.append(values[at - 1])
    assert at == len(values)
    return np.array(out)


def fixture_update(algo, variant):
    """The default route against the fixture (module docstring); returns {tensor: (error, reference's error)}."""
    fx = load_golden(algo + "_learner_update")
    assert variant in [str(v) for v in fx["variants"]]
    y = fixture_run(algo, fx, variant, True)
    x = fixture_run(algo, fx, variant, False)
    tag = variant + "64_"
    close = lambda a, ref, what: (np.asarray(a).shape == np.asarray(ref).shape and np.allclose(np.asarray(a), np.asarray(ref), rtol=1e-9, atol=0)) or \
        (_ for _ in ()).throw(AssertionError((algo, variant, what, np.asarray(a), np.asarray(ref))))
    for r in (x, y):
        assert r["batch"] == fx["batch"].tolist()
    # the float64 run is the reference's float64 run
    close(y["norms"], fx[tag + "norms"], "norms")
    close(y["means"], fx[tag + "means"], "means")
    if algo == "ppo":
        close(y["loss"], fx[tag + "loss"], "loss")
        close(y["kl"], fx[tag + "kl"], "kl")
        for r in (x, y):
            assert r["step_size"].tolist() == fx[tag + "step_size"].tolist() == fx[variant + "32_step_size"].tolist(), (variant, r["step_size"])
    else:
        close(y["value_loss"], fx[tag + "value_loss"], "value_loss")
        close(y["margins"], fx[tag + "margins"], "margins")
        close(y["vAv"], fx[tag + "vAv"], "vAv")
        close(y["new_surrogate"], _last_of_groups(fx[tag + "surrogate"], fx[tag + "trials"]), "a_new_loss")
        for r in (x, y):
            assert r["success"] == fx[tag + "success"].tolist() and r["trials"] == fx[tag + "trials"].tolist(), (variant, r["success"], r["trials"])
    worst = 0.0
    for i, (k, v) in enumerate(y["after"]):
        norm = float(fx[tag + "norm"][i])
        proj = _signs(fx, v.numel(), i) @ v.double().reshape(-1).numpy()
        worst = max(worst, float(np.abs(proj - fx[tag + "proj"][i]).max()) / norm, abs(float(v.norm()) - norm) / norm)
        assert np.abs(proj - fx[tag + "proj"][i]).max() <= 1e-9 * norm and abs(float(v.norm()) - norm) <= 1e-9 * norm, (variant, k)
    print("%s %s: float64 default route against the reference's float64 run, worst projection difference / norm %.3g" % (algo, variant, worst))
    # the rule
    ratios = {}
    for i, ((k, v), (_, v64)) in enumerate(zip(x["after"], y["after"])):
        ratios[k] = (_err(v, v64), float(fx[variant + "_err"][i]))
    for k, (e, e_ref) in ratios.items():
        print("%-4s %-9s %-18s error %.3e reference %.3e ratio %s" % (algo, variant, k, e, e_ref, "%.3f" % (e / e_ref) if e_ref > 0 else "-"))
    if algo == "trpo":
        assert ratios["log_std"] == (0.0, 0.0)
    for k, (e, e_ref) in ratios.items():
        assert e <= 2 * e_ref, (algo, variant, k, e, e_ref)
    return ratios


# ---- the opt-in routes against the default route ------------------------------------------------------------------------------------------

ROUTE_LEARN = {"ppo": dict(optim_stepsize=3e-4, cliprange=0.2, ent_coef=0.01, noptepochs=2, nminibatches=2, max_grad_norm=0.5, gamma=0.96, lam=0.95,
                           init_noise_std=0.8, desired_kl=0.016, schedule="adaptive", use_clipped_value_loss=True),
               "trpo": dict(optim_stepsize=1e-3, cliprange=0.2, noptepochs=2, nminibatches=2, max_grad_norm=0.5, gamma=0.99, lam=0.95, init_noise_std=0.8,
                            damping=0.1, cg_nsteps=3, max_kl=0.1, max_num_backtrack=10, accept_ratio=0.01, step_fraction=0.1, schedule="adaptive")}
# (envs, steps, hidden): the fixture's size, and 256 rows per minibatch over (128, 128), where the GEMM core runs more than one tile
SIZES = {"small": (16, 4, (64, 64)), "tiles": (64, 8, (128, 128))}
W, A = 12, 4


def route_rollout(size, seed=7):
    """A seeded start and a rollout collected by a behaviour policy 0.02 per element away from it (make_trpo_update_fixture.py's layout),
    fp32 on the CPU, through this package's own module and storage: (start state dict, storage fields)."""
    envs, T, hidden = SIZES[size]
    torch.manual_seed(seed)
    agent = PPO(stub_env(W, A, envs), {"policy": _policy(hidden), "learn": dict(ROUTE_LEARN["ppo"], nsteps=T)}, device="cpu",
                log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)
    ac, g = agent.actor_critic, torch.Generator().manual_seed(seed + 1)
    for t in range(T):
        obs, eps = torch.randn(envs, W, generator=g), torch.randn(envs, A, generator=g)
        with torch.no_grad():
            act = ac.actor(obs) + (2 * ac.log_std).exp() * eps
            logp, _, value, mu, sigma = ac.evaluate(obs, None, act)
        rew, done = torch.randn(envs, generator=g), (torch.rand(envs, generator=g) < 0.2).to(torch.uint8)
        agent.storage.add_transitions(obs, torch.zeros(envs, 0), act, rew.view(-1, 1), done.view(-1, 1), value, logp.view(-1, 1), mu, sigma)
    agent.storage.compute_returns(torch.zeros(envs, 1), 0.99, 0.95)
    start = {k: (v + 0.02 * torch.randn(v.shape, generator=g)).clone() for k, v in ac.state_dict().items()}
    return start, {k: getattr(agent.storage, k).clone() for k in FIELDS}


def route_learner(algo, dev, size, start, rollout, dtype=torch.float32, **more):
    envs, T, hidden = SIZES[size]
    with default_dtype(dtype):
        torch.manual_seed(0)
        agent = LEARNERS[algo](stub_env(W, A, envs), {"policy": _policy(hidden), "learn": dict(ROUTE_LEARN[algo], nsteps=T, **more)}, device=dev,
                               log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)
        agent.actor_critic.load_state_dict({k: v.to(dtype) for k, v in start.items()})
        for k in FIELDS:
            setattr(agent.storage, k, (rollout[k].clone() if k == "dones" else rollout[k].to(dtype)).to(dev))
        agent.storage.step = T
    agent.optimizer.param_groups[0]["eps"] = ADAM_EPS
    agent.trace = []
    return agent


def one_update(agent):
    dtype = next(agent.actor_critic.parameters()).dtype
    with default_dtype(dtype):
        means = agent.update()
    return means


def route_errors(algo, dev, size="small", **learn):
    """One update() of every route from the same start on the same rollout, and a float64 replay of the default route (module docstring).
    Returns {route: {tensor: (route's error, default route's error)}}."""
    start, rollout = route_rollout(size)
    routes = {"fused": dict(fused_update=True)}
    if algo == "trpo":
        routes["fused+direct"] = dict(fused_update=True, fvp="direct")
        routes["direct"] = dict(fvp="direct")
    plain = route_learner(algo, dev, size, start, rollout, **learn)
    ref = route_learner(algo, dev, size, start, rollout, torch.float64, **learn)
    m_plain, m_ref = one_update(plain), one_update(ref)
    t_plain, t_ref = _trace_arrays(algo, plain.trace), _trace_arrays(algo, ref.trace)
    decided = (lambda t: t["step_size"].tolist()) if algo == "ppo" else (lambda t: (t["success"], t["trials"]))
    assert decided(t_plain) == decided(t_ref), ("the default route decides differently in fp32 and float64: not a case to compare routes on", decided(t_plain), decided(t_ref))
    assert type(plain.optimizer).__name__ == "Adam"
    out = {}
    for name, keys in routes.items():
        agent = route_learner(algo, dev, size, start, rollout, **dict(learn, **keys))
        assert type(agent.optimizer).__name__ == ("FusedAdam" if keys.get("fused_update") else "Adam")
        assert getattr(agent.actor_critic, "fused_grad", False) == (keys.get("fvp") == "direct")
        means = one_update(agent)
        t = _trace_arrays(algo, agent.trace)
        assert decided(t) == decided(t_ref), (algo, dev, name, decided(t), decided(t_ref))
        for i in range(2):
            assert np.isfinite(means[i]) and abs(means[i] - m_ref[i]) <= 1e-4 * (1 + abs(m_ref[i])), (name, means, m_plain, m_ref)
        errs = {}
        for (k, f), (_, p), (_, r) in zip(agent.actor_critic.state_dict().items(), plain.actor_critic.state_dict().items(), ref.actor_critic.state_dict().items()):
            errs[k] = (_err(f, r), _err(p, r))
        ratio = lambda v: v[0] / v[1] if v[1] > 0 else (0.0 if v[0] == 0 else float("inf"))
        worst = max(errs.items(), key=lambda kv: ratio(kv[1]))
        print("%s %s %s %s: worst route / default error ratio %.3f at %s (%.3e against %.3e); largest default error %.3e; decisions %s" %
              (algo, dev, size, name, ratio(worst[1]), worst[0], worst[1][0], worst[1][1], max(v[1] for v in errs.values()), decided(t)))
        for k, (e_f, e_p) in errs.items():
            assert e_p < 1e-3, (k, e_p)
            assert e_f <= 2 * e_p, (algo, name, k, e_f, e_p)
        out[name] = errs
    return out


# ---- the direct curvature product alone ----------------------------------------------------------------------------------------------------

def _parts(ac, obs, act, adv, old_logp, old_mu, old_sigma, v):
    """trpo_check.hvp_parts on given advantages and log-probabilities: (mu, flat surrogate gradient, flat KL gradient, flat HVP without
    damping) through ac.evaluate, as trpo.py computes them."""
    dt = ac.log_std.dtype
    logp, _, _, mu, sigma = ac.evaluate(obs.to(dt), None, act.to(dt))
    a_loss = (-adv.to(dt) * torch.exp(logp - old_logp.to(dt))).mean()
    params = list(ac.actor.parameters())
    flat_g = torch.cat([t.reshape(-1) for t in torch.autograd.grad(a_loss, params, retain_graph=True)]).detach()
    kl = tk.kl_of(mu, sigma, old_mu.to(dt), old_sigma.to(dt))
    fk = torch.cat([t.view(-1) for t in torch.autograd.grad(kl, params, create_graph=True)])
    hv = torch.cat([t.contiguous().view(-1) for t in torch.autograd.grad((fk * v.to(dt)).sum(), params, retain_graph=True)]).detach()
    return mu.detach(), flat_g, fk.detach(), hv


def check_direct_product(dev, rows=300, hidden=(128, 64), seed=0):
    """TRPO.kl_hessian_times_vector with fvp="direct" (mms_mlp_grad_rop, mms_trpo_heads' gn, mms_mlp_grad) and the two gradients of the fused
    route against the float64 double backward of the reference's KL at mu != old_mu and old_sigma != sigma, so the curvature term is
    live; trpo_check.within_torch as it stands, with torch's fp32 autograd over the plain module beside it."""
    cfg = {"pi_hid_sizes": list(hidden), "vf_hid_sizes": list(hidden), "activation": "elu"}
    ac, obs, act, old_mu, v = tk.make_actor((W,), A, cfg, rows, dev, moved=True, seed=seed)
    g = torch.Generator().manual_seed(seed + 5)
    adv = torch.randn(rows, generator=g).to(dev)
    with torch.no_grad():
        old_sigma = (ac.log_std.detach() + 0.05 * torch.randn(rows, A, generator=g).to(dev)).contiguous()
        old_logp = (ac.evaluate(obs, None, act)[0] + 0.1 * torch.randn(rows, generator=g).to(dev)).contiguous()
    plain = copy.deepcopy(ac)
    plain.fused_grad = False
    truth = _parts(copy.deepcopy(plain).double(), obs, act, adv, old_logp, old_mu, old_sigma, v)
    torch32 = _parts(plain, obs, act, adv, old_logp, old_mu, old_sigma, v)

    learner = types.SimpleNamespace(actor_critic=ac, fvp="direct", damping=0.0, _rec=None, _direct=None, storage=None)
    rows_ = StoredRows.__new__(StoredRows)
    rows_.indices, rows_.rows = torch.arange(rows, device=dev), rows
    rows_.actions, rows_.old_mu, rows_.old_sigma, rows_.old_logp, rows_.adv = act.contiguous(), old_mu.contiguous(), old_sigma, old_logp, adv
    mu, net = ac.mean_saved(obs)
    first = trpo_heads(ac.log_std.detach(), mu=mu, stored=rows_, want=("out", "logp", "gsur", "gkl"))
    flat_g, flat_k = grad_flat(net, first["gsur"]), grad_flat(net, first["gkl"])
    TRPO._prepare_direct(learner, obs, None, saved=(mu, net), gkl=first["gkl"])
    hv = TRPO.kl_hessian_times_vector(learner, v, None)
    errs = [(tk.rms(f.double() - t), tk.rms(y.double() - t), tk.rms(t)) for f, y, t in zip((mu, flat_g, flat_k, hv), torch32, truth)]
    for n, (ef, et, sc) in zip(("mu", "surrogate gradient", "KL gradient", "HVP"), errs):
        print("  %-20s direct %.3e  torch fp32 %.3e  float64 rms %.3e" % (n, ef, et, sc))
    # the curvature term is live: without it the product is off by far more than the gate
    gauss_newton = grad_flat(net, trpo_heads(ac.log_std.detach(), rmu=_jv(net, first["gkl"], v), want=("gn",))["gn"])
    assert tk.rms(gauss_newton.double() - truth[3]) > 100 * max(errs[3][0], errs[3][1])
    fails = tk.within_torch(errs)
    assert not fails, fails
    return errs


def _jv(net, gkl, v):
    from massive_marl_benchmark_amd.algorithms.rl.trpo.module import grad_saved, rop_flat
    d, e = grad_saved(net, gkl)
    return rop_flat(net, gkl, d, e, v.contiguous())[0]


# ---- the learners' contract ---------------------------------------------------------------------------------------------------------------

def check_contract(algo, dev):
    fx = load_golden(algo + "_learner_update")
    cls = LEARNERS[algo]
    start, rollout = route_rollout("small")
    agent = route_learner(algo, dev, "small", start, rollout)
    keys = [str(k) for k in fx["keys"]]
    assert list(agent.actor_critic.state_dict().keys()) == keys
    assert list(route_learner(algo, dev, "small", start, rollout, fused_update=True).actor_critic.state_dict().keys()) == keys
    methods = ["run", "update", "log", "save", "load", "test"]
    names = ["actor_critic", "storage", "optimizer", "num_learning_epochs", "num_mini_batches", "gamma", "lam", "max_grad_norm", "use_clipped_value_loss",
             "clip_param", "schedule", "step_size", "init_noise_std", "model_cfg", "cfg_train", "log_dir", "print_log", "writer", "tot_timesteps", "tot_time",
             "is_testing", "current_learning_iteration", "apply_reset", "learning_rate", "num_transitions_per_env", "asymmetric", "device",
             "observation_space", "action_space", "state_space", "vec_env"]
    if algo == "ppo":
        names += ["desired_kl", "value_loss_coef", "entropy_coef"]
    else:
        methods += ["conjugate_gradient", "line_search", "kl_hessian_times_vector", "set_pi_flat_params", "get_pi_flat_params", "get_aloss_logp"]
        names += ["damping", "cg_nsteps", "max_kl", "max_num_backtrack", "accept_ratio", "step_fraction"]
        assert agent.fvp == "autograd" and not agent.actor_critic.fused_grad
    for name in methods:
        assert callable(getattr(agent, name)), name
    for name in names:
        assert hasattr(agent, name), name
    assert agent.fused_update is False and agent.trace == [] and type(agent.optimizer).__name__ == "Adam"
    assert len(agent.optimizer.param_groups[0]["params"]) == len(list(agent.actor_critic.parameters()))
    assert agent.cfg_train["learn"] is not None and agent.log_dir.endswith("run")
    learn = dict(ROUTE_LEARN[algo], nsteps=4)
    for bad in ("observation_space", "state_space", "action_space"):
        env = stub_env(W, A, 16)
        setattr(env, bad, (12,))
        try:
            cls(env, {"policy": _policy(), "learn": learn})
            raise AssertionError("a non-Space %s was accepted" % bad)
        except TypeError as e:
            assert bad in str(e)
    if algo == "trpo":
        # fvp = "direct" needs an actor the kernels take: ELU layers, input widths multiples of 4
        for policy, w in ((dict(_policy(), activation="selu"), W), (_policy(), 10)):
            try:
                cls(stub_env(w, A, 16), {"policy": policy, "learn": dict(learn, fvp="direct")}, device=dev)
                raise AssertionError("fvp = 'direct' accepted an actor that does not qualify")
            except ValueError as e:
                assert "direct" in str(e)
        try:
            cls(stub_env(W, A, 16), {"policy": _policy(), "learn": dict(learn, fvp="exact")}, device=dev)
            raise AssertionError("an unknown fvp was accepted")
        except ValueError:
            pass
        assert cls(stub_env(W, A, 16), {"policy": _policy(), "learn": dict(learn, fvp="direct")}, device=dev).actor_critic.fused_grad
        # the flat layout is actor.parameters()'s, and log_std is not in it
        flat = agent.get_pi_flat_params()
        assert flat.numel() == sum(p.numel() for p in agent.actor_critic.actor.parameters())
        agent.set_pi_flat_params(flat * 0.5)
        assert torch.equal(agent.get_pi_flat_params(), flat * 0.5) and agent.old_log_prob is None
        agent.set_pi_flat_params(flat)
    # save / load / test round trip, and the iteration in the file name
    path = os.path.join(tempfile.mkdtemp(), "model_37.pt")
    agent.save(path)
    other_start = {k: v + 1.0 for k, v in start.items()}
    other = route_learner(algo, dev, "small", other_start, rollout)
    other.load(path)
    assert other.current_learning_iteration == 37 and other.actor_critic.training
    for (k, a), (_, b) in zip(agent.actor_critic.state_dict().items(), other.actor_critic.state_dict().items()):
        assert torch.equal(a, b), k
    third = route_learner(algo, dev, "small", other_start, rollout)
    third.test(path)
    assert not third.actor_critic.training and third.current_learning_iteration == 0
    assert torch.equal(third.actor_critic.actor[0].weight, agent.actor_critic.actor[0].weight)
    # one update: every minibatch of every epoch takes a step; log_std moves under PPO only
    before = agent.actor_critic.log_std.detach().clone()
    means = one_update(agent)
    assert len(agent.trace) == 4 and all(np.isfinite(m) for m in means)
    assert torch.equal(before, agent.actor_critic.log_std.detach()) == (algo == "trpo")
    return means


def check_run(algo, device_type, fused):
    """run(2) on a small OneAnt engine: two rollouts, two updates with finite losses, the models saved, the storage cleared."""
    import dropin_check as drop
    env = drop.make_env("OneAnt", 16, device_type, episode_length=4)
    dev = "cpu" if device_type == "cpu" else "cuda:0"
    learn = dict(ROUTE_LEARN[algo], nsteps=4, fused_update=fused)
    torch.manual_seed(0)
    agent = LEARNERS[algo](env, {"policy": _policy((32, 32)), "learn": learn}, device=dev, log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=True)
    updates, update = [], agent.update

    def counted():
        assert agent.storage.step == 4
        out = update()
        updates.append(out)
        return out
    agent.update = counted
    agent.run(2, log_interval=1)
    assert len(updates) == 2 and all(np.isfinite(v) for out in updates for v in out) and agent.storage.step == 0
    assert agent.tot_timesteps == 2 * 4 * 16
    for name in ("model_0.pt", "model_1.pt", "model_2.pt"):
        assert os.path.exists(os.path.join(agent.log_dir, name)), name
    assert all(bool(torch.isfinite(p).all()) for p in agent.actor_critic.parameters())
    return updates


def check_graph_capture():
    """The fused PPO minibatch up to the schedule's read -- the gather, both networks, mms_ppo_loss -- captured in a graph (a host read
    inside it would fail the capture) and replayed after the parameters have moved: the eager call's bits."""
    dev = torch.device("cuda:0")
    start, rollout = route_rollout("tiles")
    agent = route_learner("ppo", dev, "tiles", start, rollout, fused_update=True)
    indices = torch.as_tensor(list(agent.storage.mini_batch_generator(2))[1], dtype=torch.int64, device=dev)
    agent._fused_minibatch(indices)                             # the workspace and the optimizer state exist before the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            loss, info = agent._fused_loss(indices)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        eager_loss, eager_info = agent._fused_loss(indices)
        assert loss.requires_grad and torch.isfinite(loss) and torch.equal(loss, eager_loss) and all(torch.equal(info[k], eager_info[k]) for k in info)
        agent._fused_minibatch(indices)                         # the parameters move; the replay follows them

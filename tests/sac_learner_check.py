"""Checks of the SAC learner (algorithms/rl/sac/sac.py) and of the loss heads behind it (algorithms/rl/sac/loss.py, MLPActorCritic.q_loss /
pi_loss), shared by test_sac_learner.py (CPU build) and test_sac_learner_gpu.py.

The fixture (tests/golden/sac_update.npz, make_sac_update_fixture.py) holds one update() of the reference's own learner, fp32 and
float64, as it is ("ref") and with its freeze loops working ("freeze").  Its parameters after the update are stored as per-tensor
norms, seeded +-1 projections and the reference's own fp32 error; `fixture_update` therefore evaluates this package's default route
in float64 on the recorded eps, ANCHORS it to the reference's float64 run (every projection and norm to 1e-9 of the tensor's norm,
losses and clip norms to 1e-9 relative: a float64 run differs from another by roundings of 1e-16 which the update amplifies by at
most the 2e4 that the fp32 errors of 1e-3 show), and then applies the rule: per tensor, the fp32 default route's relative-norm
error against that yardstick is at most 2 x the reference's own fp32 error -- the only differences are summation order and the
restated log-density."""
import copy
import json
import os
import random
import tempfile
import types

import numpy as np
import torch

import sac_check as sc
from conftest import load_golden
from massive_marl_benchmark_amd import _lib
from massive_marl_benchmark_amd.algorithms.rl.sac import SAC, MLPActorCritic
from massive_marl_benchmark_amd.algorithms.rl.sac import loss as sac_loss
from massive_marl_benchmark_amd.spaces import Box


def stub_env(W, A, envs):
    return types.SimpleNamespace(observation_space=Box(-np.inf, np.inf, (W,)), state_space=Box(-np.inf, np.inf, (W,)), action_space=Box(-1.0, 1.0, (A,)),
                                 num_envs=envs, task=types.SimpleNamespace(cfg={"seed": 0}))


def _learn(fx, **more):
    learn = {k: float(v) for k, v in zip(fx["learn_keys"], fx["learn_values"])}
    for k in ("replay_size", "batch_size", "nsteps", "hidden_nodes", "hidden_layer", "noptepochs", "nminibatches"):
        learn[k] = int(learn[k])
    learn.update(more)
    return learn


def _err(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


# ---- the default route against the reference's update ------------------------------------------------------------------------------------

def fixture_run(fx, freeze, double):
    """One update() of the default route from the fixture's start, on "cpu", with the recorded eps.  Returns what the fixture records."""
    W, A = fx["trans_obs"].shape[-1], fx["trans_act"].shape[-1]
    envs = fx["trans_obs"].shape[1]
    torch.manual_seed(0)
    sac = SAC(stub_env(W, A, envs), {"learn": _learn(fx, freeze_q=freeze)}, device="cpu", log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=False)
    sd = sac.actor_critic.state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["keys"]]                       # the reference's state_dict keys, in its order
    words = torch.from_numpy((fx["init_bf16"].astype(np.uint32) << 16).view(np.float32).copy())
    at = 0
    for k, v in sd.items():
        v.copy_(words[at:at + v.numel()].view(v.shape))
        at += v.numel()
    assert at == words.numel()
    sac.actor_critic_targ.load_state_dict(sac.actor_critic.state_dict())
    for t in range(fx["trans_obs"].shape[0]):
        T = lambda k: torch.from_numpy(fx["trans_" + k][t])
        sac.storage.add_transitions(T("obs"), T("states"), T("act"), T("rew"), T("obs2"), T("done"))
    for k in ("observations", "states", "actions", "rewards", "next_observations", "dones"):
        assert torch.equal(getattr(sac.storage, k), torch.from_numpy(fx["ring_" + k])), k
    assert sac.storage.step == int(fx["ring_step"]) and sac.storage.fullfill == bool(fx["ring_fullfill"])
    if double:
        sac.actor_critic.double()
        sac.actor_critic_targ.double()
        for k in ("observations", "states", "actions", "rewards", "next_observations"):
            setattr(sac.storage, k, getattr(sac.storage, k).double())
    eps = [torch.from_numpy(e) for e in fx["eps"]]
    dtype = torch.float64 if double else torch.float32

    def source(shape):
        e = eps.pop(0)
        assert tuple(e.shape) == tuple(shape)
        return e.to(dtype)
    sac.eps_source = source
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
    random.seed(int(fx["seeds"][3]))
    try:
        means = sac.update()
    finally:
        torch.nn.utils.clip_grad_norm_ = clip
    assert not eps                                                                # every recorded draw was used
    after = list(sac.actor_critic.state_dict().items()) + [("targ." + k, v) for k, v in sac.actor_critic_targ.state_dict().items()]
    assert [k for k, _ in after] == [str(k) for k in fx["after_keys"]]
    return dict(batch=rec["batch"], loss_q=torch.stack(rec["loss_q"]), loss_pi=torch.stack(rec["loss_pi"]), norms=torch.stack(rec["norms"]),
                means=means, after=after)


def _signs(fx, numel, index):
    seed, proj = int(fx["seeds"][4]), int(fx["seeds"][5])
    return np.random.RandomState(1000 * seed + index).randint(0, 2, (proj, numel)).astype(np.float64) * 2 - 1


def fixture_update(freeze):
    """The default route against the fixture (module docstring); returns {tensor: (error, reference's error, ratio)}."""
    fx = load_golden("sac_update")
    tag = "freeze" if freeze else "ref"
    y = fixture_run(fx, freeze, True)
    x = fixture_run(fx, freeze, False)
    for r in (x, y):
        assert r["batch"] == fx["batch"].tolist()                                 # the index lists: drawn once, the reference's stream
    # the float64 run is the reference's float64 run
    for k in ("loss_q", "loss_pi", "norms"):
        ref = torch.from_numpy(fx[tag + "64_" + k])
        assert float((y[k] - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), (tag, k)
    assert np.allclose(np.array(y["means"]), fx[tag + "64_means"], rtol=1e-9, atol=0)
    worst = 0.0
    for i, (k, v) in enumerate(y["after"]):
        norm = float(fx[tag + "64_norm"][i])
        proj = _signs(fx, v.numel(), i) @ v.double().reshape(-1).numpy()
        worst = max(worst, float(np.abs(proj - fx[tag + "64_proj"][i]).max()) / norm, abs(float(v.norm()) - norm) / norm)
        assert np.abs(proj - fx[tag + "64_proj"][i]).max() <= 1e-9 * norm and abs(float(v.norm()) - norm) <= 1e-9 * norm, (tag, k)
    print("%s: float64 default route against the reference's float64 run, worst projection difference / norm %.3g" % (tag, worst))
    # the rule
    ratios = {}
    for k in ("loss_q", "loss_pi"):
        e, e_ref = _err(x[k], y[k]), _err(torch.from_numpy(fx[tag + "32_" + k]), y[k])
        ratios[k] = (e, e_ref, e / e_ref)
    for i, ((k, v), (_, v64)) in enumerate(zip(x["after"], y["after"])):
        e, e_ref = _err(v, v64), float(fx[tag + "_err"][i])
        ratios[k] = (e, e_ref, e / e_ref)
        # ... and the fp32 run is near the reference's fp32 run: both within their errors of the same yardstick
        proj = _signs(fx, v.numel(), i) @ v.double().reshape(-1).numpy()
        assert np.abs(proj - fx[tag + "32_proj"][i]).max() <= (e + e_ref) * float(fx[tag + "64_norm"][i]) * np.sqrt(v.numel()), (tag, k)
    for k, (e, e_ref, ratio) in ratios.items():
        print("%-6s %-28s error %.3e reference %.3e ratio %.3f" % (tag, k, e, e_ref, ratio))
    for k, (e, e_ref, ratio) in ratios.items():
        assert e <= 2 * e_ref, (tag, k, e, e_ref)
    return ratios


# ---- q_loss / pi_loss against q_heads_loss_torch and float64 ------------------------------------------------------------------------------

def _grads(loss, leaves):
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=False)
    out = {k: g.detach() for k, g in zip(leaves.keys(), gs)}
    out["loss"] = loss.detach()
    return out


def loss_head_ratios(dev, H, M=300, W=12, A=4, alpha=0.2):
    """{head: {tensor: {"fused", "torch_fp32", "ratio"}}} for MLPActorCritic.q_loss and the policy head on given (pi, logp): relative-norm
    errors against float64 of the fused path (asserted to be the one taken) and of the fp32 torch expression.  `assert_head_rule`
    applies the rule to them."""
    torch.manual_seed(5 + H)
    ac = MLPActorCritic(Box(-np.inf, np.inf, (W,)), Box(-1.0, 1.0, (A,)), hidden_sizes=(H, H)).to(dev)
    ac64 = copy.deepcopy(ac).double()
    g = torch.Generator().manual_seed(H)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev)
    base = dict(o=mk(M, W), a=torch.tanh(mk(M, A)), pi=torch.tanh(mk(M, A)), logp=mk(M) * 2 - 3, backup=mk(M, 1))

    def inputs(double):
        d = {k: (v.double() if double else v.clone()) for k, v in base.items()}
        for k in ("o", "a", "pi", "logp"):
            d[k].requires_grad_(True)
        return d

    def critics(net, x):
        return [q.q[:-2](x) for q in (net.q1, net.q2)], [net.q1.q[-2], net.q2.q[-2]]

    def leaves(net, d, names):
        out = {k: d[k] for k in names}
        out.update({k: p for k, p in net.named_parameters() if k.startswith("q")})
        return out

    def q_head(net, d, fused):
        if fused:
            return net.q_loss(d["o"], d["a"], d["backup"])
        hs, lasts = critics(net, torch.cat([d["o"], d["a"]], -1))
        return sac_loss.q_heads_loss_torch(hs, lasts, target=d["backup"], mode="mse")

    def pi_head(net, d, fused):
        hs, lasts = critics(net, torch.cat([d["o"], d["pi"]], -1))
        fn = sac_loss.q_heads_loss if fused else sac_loss.q_heads_loss_torch
        return fn(hs, lasts, logp=d["logp"], alpha=alpha, mode="pi")

    ratios = {}
    for name, head, names in (("q_loss", q_head, ("o", "a")), ("pi_loss head", pi_head, ("o", "pi", "logp"))):
        d = inputs(False)
        loss = head(ac, d, True)
        assert type(loss.grad_fn).__name__ == "_QHeadsLossBackward", (name, loss.grad_fn)      # the entry, not the torch expression
        fused = _grads(loss, leaves(ac, d, names))
        d = inputs(False)
        plain = _grads(head(ac, d, False), leaves(ac, d, names))
        d = inputs(True)
        ref = _grads(head(ac64, d, False), leaves(ac64, d, names))
        ratios[name] = {}
        for k, r in ref.items():
            e_f, e_t = _err(fused[k], r), _err(plain[k], r)
            ratios[name][k] = {"fused": e_f, "torch_fp32": e_t, "ratio": e_f / e_t if e_t > 0 else (0.0 if e_f == 0 else float("inf"))}
            print("H %4d %-13s %-14s fused %.3e torch %.3e ratio %.3f" % (H, name, k, e_f, e_t, ratios[name][k]["ratio"]))
    # pi_loss itself: the actor in front of the same head (fused_grad=False: torch draws the noise, so the same seed gives the expression)
    torch.manual_seed(1)
    got = ac.pi_loss(base["o"], alpha)
    torch.manual_seed(1)
    pi, logp = ac.pi(base["o"])
    want = (alpha * logp - torch.min(ac.q1(base["o"], pi), ac.q2(base["o"], pi))).mean()
    assert type(got.grad_fn).__name__ == "_QHeadsLossBackward" and abs(float(got.detach()) - float(want.detach())) <= 1e-5 * (1 + abs(float(want.detach())))
    return ratios


def assert_head_rule(ratios_by_h, head):
    """Every fused error against float64 is at most 2 x the fp32 torch expression's (sac_grad_check.module_gradient_ratios' rule)."""
    bad = {(H, k): v for H, r in ratios_by_h.items() for k, v in r[head].items() if not v["fused"] <= 2 * v["torch_fp32"]}
    assert not bad, bad


def record_head_ratios(build, ratios_by_h):
    """With MMS_RECORD_DIR set: the measured ratios into <that directory>/sac_loss_head_error.json, one entry per build, rewritten by the
    run that measured it (profiles/sac_loss_head_error.json is such a file).  Without it nothing is written."""
    out = os.environ.get("MMS_RECORD_DIR")
    if not out:
        return
    path = os.path.join(out, "sac_loss_head_error.json")
    os.makedirs(out, exist_ok=True)
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[build] = {"M": 300, "rule": "fused error against float64 <= 2 x the fp32 torch expression's (relative norms)",
                  "H": {str(h): r for h, r in ratios_by_h.items()}}
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)


def check_fallback(dev):
    """What the entry does not take runs the torch expression, chosen before anything is launched."""
    torch.manual_seed(2)
    for H, dtype in ((96, torch.float32), (1088, torch.float32), (64, torch.float64)):
        ac = MLPActorCritic(Box(-np.inf, np.inf, (12,)), Box(-1.0, 1.0, (4,)), hidden_sizes=(H,)).to(dev).to(dtype)
        o, a, b = (torch.randn(9, n, device=dev, dtype=dtype) for n in (12, 4, 1))
        loss = ac.q_loss(o, a, b)
        assert type(loss.grad_fn).__name__ != "_QHeadsLossBackward", (H, dtype)
        want = ((ac.q1(o, a) - b) ** 2).mean() + ((ac.q2(o, a) - b) ** 2).mean()
        assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * (1 + abs(float(want.detach())))
        loss.backward()
    # frozen critics get no weight gradient from the policy head, the actor and the input still do
    ac = MLPActorCritic(Box(-np.inf, np.inf, (12,)), Box(-1.0, 1.0, (4,)), hidden_sizes=(64, 64)).to(dev)
    for p in (*ac.q1.parameters(), *ac.q2.parameters()):
        p.requires_grad = False
    ac.pi_loss(torch.randn(9, 12, device=dev), 0.2).backward()
    assert all(p.grad is None for p in (*ac.q1.parameters(), *ac.q2.parameters())) and all(p.grad is not None for p in ac.pi.parameters())
    # once differentiable
    ac = MLPActorCritic(Box(-np.inf, np.inf, (12,)), Box(-1.0, 1.0, (4,)), hidden_sizes=(64, 64)).to(dev)
    o = torch.randn(9, 12, device=dev, requires_grad=True)
    try:
        (gx,) = torch.autograd.grad(ac.q_loss(o, torch.randn(9, 4, device=dev), torch.randn(9, 1, device=dev)), o, create_graph=True)
        raise AssertionError("a double backward through the fused head did not raise")
    except RuntimeError as e:
        assert "once differentiable" in str(e)


# ---- the fused route against the default route --------------------------------------------------------------------------------------------

ROUTE_LEARN = dict(learning_rate=1e-3, replay_size=6, batch_size=4, nsteps=2, hidden_nodes=64, hidden_layer=2, noptepochs=2, nminibatches=2, ent_coef=0.2,
                   gamma=0.99, polyak=0.5, max_grad_norm=0.5, reward_scale=1.0)
ADAM_EPS = 1e-3           # with lr 1e-3: gradients far below it move a parameter in proportion, so Adam's first steps do not turn a rounding
                          # error of a near-zero gradient into a step of +-lr; test_routes asserts the default route's own error < 1e-3


def _route_learner(dev, fused, dtype=torch.float32, W=12, A=4, envs=16, seed=7, freeze=False):
    torch.manual_seed(seed)
    sac = SAC(stub_env(W, A, envs), {"learn": dict(ROUTE_LEARN, fused_update=fused, freeze_q=freeze)}, device=dev, log_dir=os.path.join(tempfile.mkdtemp(), "run"),
              print_log=False)
    sac.actor_critic.pi.fused_grad = True                     # both routes: the head with a gradient draws the counter stream
    sac.actor_critic.pi.seed = 1234
    for opt in (sac.pi_optimizer, sac.q_optimizer):
        opt.param_groups[0]["eps"] = ADAM_EPS
    g = torch.Generator().manual_seed(seed + 1)
    for t in range(5):
        done = (torch.rand(envs, generator=g) < 0.3).to(torch.uint8)
        sac.storage.add_transitions(*(x.to(dev) for x in (torch.randn(envs, W, generator=g), torch.randn(envs, W, generator=g), torch.rand(envs, A, generator=g) * 2 - 1,
                                                         torch.randn(envs, generator=g), torch.randn(envs, W, generator=g), done)))
    if dtype == torch.float64:
        sac.actor_critic.double()
        sac.actor_critic_targ.double()
        for k in ("observations", "states", "actions", "rewards", "next_observations"):
            setattr(sac.storage, k, getattr(sac.storage, k).double())
    return sac


def _one_update(sac, record=None, replay=None):
    """update() from fixed seeds.  record: a list that receives the standard normals of every pi call; replay: such a list to use."""
    pi = sac.actor_critic.pi
    handle = None
    if record is not None:
        L, idx, stream = _lib.for_device(next(pi.parameters()).device)

        def hook(module, args):
            o = args[0]
            N, A = o[..., 0].numel(), module.mu_layer.out_features
            dev = o.device
            if torch.is_grad_enabled() or dev.type == "cuda":                     # the counter stream (module.py)
                z = sc.draws(L, idx, stream, module.seed, module.counters(N, dev), module.row_offset, N, A)
            else:                                                                 # torch_forward's randn_like, without moving the generator
                state = torch.get_rng_state()
                z = torch.randn(N, A)
                torch.set_rng_state(state)
            record.append(z.view(*o.shape[:-1], A).clone())
        handle = pi.register_forward_pre_hook(hook)
    if replay is not None:
        todo = list(replay)
        sac.eps_source = lambda shape: todo.pop(0).to(next(pi.parameters()).dtype)
    random.seed(3)
    torch.manual_seed(4)
    means = sac.update()
    if handle is not None:
        handle.remove()
    if replay is not None:
        assert not todo
    return means


def route_errors(dev, freeze=False):
    """One update() of the fused route and of the default route from the same start, and a float64 replay of the same update on the
    draws both used.  Asserts: both routes drew the same noise; the default route's own error stays below 1e-3 per tensor; per
    tensor the fused route's error against float64 is at most 2 x the default route's."""
    plain, fused = _route_learner(dev, False, freeze=freeze), _route_learner(dev, True, freeze=freeze)
    assert type(fused.q_optimizer).__name__ == "FusedAdam" and type(plain.q_optimizer).__name__ == "Adam"
    for (k, a), (_, b) in zip(plain.actor_critic.state_dict().items(), fused.actor_critic.state_dict().items()):
        assert torch.equal(a, b), k
    z_plain, z_fused = [], []
    m_plain = _one_update(plain, record=z_plain)
    m_fused = _one_update(fused, record=z_fused)
    assert len(z_plain) == len(z_fused) == 8 and all(torch.equal(a, b) for a, b in zip(z_plain, z_fused))
    ref = _route_learner(dev, False, torch.float64, freeze=freeze)
    m_ref = _one_update(ref, replay=[z.double() for z in z_plain])
    out = {}
    for i, name in enumerate(("mean_value_loss", "mean_surrogate_loss")):
        assert np.isfinite(m_fused[i]) and abs(m_fused[i] - m_ref[i]) <= 1e-4 * (1 + abs(m_ref[i])), (name, m_fused, m_plain, m_ref)
    tensors = lambda s: list(s.actor_critic.state_dict().items()) + [("targ." + k, v) for k, v in s.actor_critic_targ.state_dict().items()]
    for (k, f), (_, p), (_, r) in zip(tensors(fused), tensors(plain), tensors(ref)):
        e_f, e_p = _err(f, r), _err(p, r)
        out[k] = (e_f, e_p)
    worst = max(out.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print("%s freeze_q %s: worst fused / default error ratio %.3f at %s (%.3e against %.3e); largest default error %.3e" %
          (dev, freeze, worst[1][0] / worst[1][1], worst[0], worst[1][0], worst[1][1], max(v[1] for v in out.values())))
    for k, (e_f, e_p) in out.items():
        assert e_p < 1e-3, (k, e_p)
        assert e_f <= 2 * e_p, (k, e_f, e_p)
    return out


def check_graph_capture():
    """One minibatch of the fused route captured in a graph (a host read inside it would fail the capture) and replayed."""
    dev = torch.device("cuda:0")
    sac = _route_learner(dev, True)
    eager = _route_learner(dev, True)
    random.seed(3)
    indices = sac.storage.mini_batch_generator(2)[0]
    data, data_e = sac._gather(indices), eager._gather(indices)
    rows = data["obs"][..., 0].numel()
    for s, d in ((sac, data), (eager, data_e)):
        s.actor_critic.pi.reserve_counters(rows, dev)
        s._fused_minibatch(d)                                 # optimizer state, workspaces and partials exist before the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            lq, lp = sac._fused_minibatch(data)
    torch.cuda.current_stream().wait_stream(stream)
    graph.replay()
    torch.cuda.synchronize()
    eq, ep = eager._fused_minibatch(data_e)
    torch.cuda.synchronize()
    assert torch.isfinite(lq) and torch.isfinite(lp)
    # the replay is the second minibatch step of both learners: the same launches on the same state
    assert abs(float(lq) - float(eq)) <= 1e-5 * (1 + abs(float(eq))) and abs(float(lp) - float(ep)) <= 1e-5 * (1 + abs(float(ep)))
    for (k, a), (_, b) in zip(sac.actor_critic.state_dict().items(), eager.actor_critic.state_dict().items()):
        assert _err(a, b) <= 1e-5, k


# ---- the learner's contract ---------------------------------------------------------------------------------------------------------------

def check_contract(dev):
    fx = load_golden("sac_update")
    sac = _route_learner(dev, False)
    assert list(sac.actor_critic.state_dict().keys()) == [str(k) for k in fx["keys"]]
    for name in ("run", "update", "compute_loss_q", "compute_loss_pi", "log", "save", "load", "test"):
        assert callable(getattr(sac, name)), name
    for name in ("actor_critic", "actor_critic_targ", "storage", "q_params", "pi_optimizer", "q_optimizer", "num_learning_epochs", "num_mini_batches", "entropy_coef",
                 "gamma", "polyak", "max_grad_norm", "use_clipped_value_loss", "reward_scale", "batch_size", "warm_up", "log_dir", "print_log", "writer", "tot_timesteps",
                 "tot_time", "is_testing", "current_learning_iteration", "apply_reset", "learning_rate", "replay_size", "num_transitions_per_env", "asymmetric",
                 "device", "observation_space", "action_space", "state_space", "vec_env"):
        assert hasattr(sac, name), name
    assert sac.log_dir.endswith("_seed0") and sac.warm_up is True and sac.fused_update is False and sac.freeze_q is False and sac.layers == "fp32"
    assert list(sac.q_params) == []                                               # the exhausted chain
    assert len(_route_learner(dev, False, freeze=True).q_params) == 12
    try:
        SAC(types.SimpleNamespace(observation_space=(12,), state_space=Box(-1, 1, (12,)), action_space=Box(-1, 1, (4,))), {"learn": ROUTE_LEARN})
        raise AssertionError("a non-Space observation_space was accepted")
    except TypeError as e:
        assert "observation_space" in str(e)
    # save / load / test round trip, and the iteration in the file name
    _one_update(sac)
    path = os.path.join(tempfile.mkdtemp(), "model_37.pt")
    sac.save(path)
    other = _route_learner(dev, False, seed=99)
    other.load(path)
    assert other.current_learning_iteration == 37 and other.actor_critic.training
    for (k, a), (_, b) in zip(sac.actor_critic.state_dict().items(), other.actor_critic.state_dict().items()):
        assert torch.equal(a, b), k
    third = _route_learner(dev, False, seed=98)
    third.test(path)
    assert not third.actor_critic.training and third.current_learning_iteration == 0
    assert torch.equal(third.actor_critic.pi.mu_layer.weight, sac.actor_critic.pi.mu_layer.weight)


def check_run(device_type, fused):
    """run(2) on a small MultiIngenuity engine: warm-up ends at the reference's step, every later step updates, losses are finite,
    and next_observations' ring rows are the step kernel's own writes."""
    import dropin_check as dc
    env = dc.make_env("MultiIngenuity", 16, device_type, episode_length=4)
    dev = "cpu" if device_type == "cpu" else "cuda:0"
    learn = dict(ROUTE_LEARN, nsteps=3, replay_size=8, batch_size=4, hidden_nodes=64, fused_update=fused)
    torch.manual_seed(0)
    random.seed(0)
    sac = SAC(env, {"learn": learn}, device=dev, log_dir=os.path.join(tempfile.mkdtemp(), "run"), print_log=True)
    updates, seen, bound = [], [], []
    update, step, bind = sac.update, env.step, env.task.engine.bind_obs_out

    def counted():
        out = update()
        updates.append((sac.storage.step, out))
        return out

    def stepped(actions):
        out = step(actions)
        seen.append(out[0].clone())
        return out

    def binding(t):
        if t is not None:
            bound.append(t.data_ptr())
        return bind(t)
    sac.update, env.step, env.task.engine.bind_obs_out = counted, stepped, binding
    sac.run(2, log_interval=1)
    # batch_size 4: the fourth transition ends the warm-up (storage.step >= batch_size), and the update runs after it and after every later step
    assert [s for s, _ in updates] == [4, 5, 6] and sac.warm_up is False
    assert all(np.isfinite(v) for _, out in updates for v in out)
    assert len(seen) == 6 and bound == [sac.storage.next_observations[k].data_ptr() for k in range(6)]
    for k, obs in enumerate(seen):
        assert torch.equal(sac.storage.next_observations[k], obs.view(sac.storage.next_observations[k].shape)), k
    for name in ("model_0.pt", "model_1.pt", "model_2.pt"):
        assert os.path.exists(os.path.join(sac.log_dir, name)) == (name != "model_0.pt"), name      # iteration 0 ends inside the warm-up
    assert env.task.engine._bound is None                     # the binding is released

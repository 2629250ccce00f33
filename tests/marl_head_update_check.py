"""Checks of heads.update_heads and of the MAPPO / HAPPO trainers' `fused_head_update` route (algorithms/marl/heads.py, trainer.py), shared
by tests/test_marl_head_update.py (torch device "cpu": the CPU build) and tests/test_marl_head_update_gpu.py (the HIP build).

update_heads against the modules: tests/marl_modules.py's stand-ins, G = 3 agents (A = 3, 1, 16 -- every action tile of the kernels),
hidden 36 and 128, 37 rows.  The gate is tests/marl_heads_grad_check.py's: the relative Frobenius error against a float64 evaluation of
the same modules on the same fp32 values is at most twice that of the modules' own forward + autograd in fp32 on the same device, or
u = 2^-24 where that is smaller -- per output, per feature gradient and per parameter gradient, DRAWS = 4 draws pooled as
tests/marl_block_update_check.py pools them.

The trainers: marl_block_update_check's cases (both trainers on the feed-forward, the RNNLayer and the fused_rnn_update route), its
samples, its float64 replay and its UPDATE_DRAWS = 24 pooled draws (its docstring says why 24), with `fused_head_update` on against the
default route.  The lockstep route is marl_grouped_update_check.routes with the key on: both routes end in equal bits."""
import copy

import torch

import marl_block_update_check as bu
import marl_grouped_update_check as gu
import marl_loss_check as mlc
import marl_modules as mm
import marl_rnn_check as rc
import marl_rnn_update_check as uc
from massive_marl_benchmark_amd import _lib
from massive_marl_benchmark_amd.algorithms.marl import heads
from massive_marl_benchmark_amd.algorithms.marl import trainer as tr

DRAWS = 4
ENTRIES = ("mms_marl_heads_fwd_group", "mms_marl_heads_grad_group")


def _nets(device, hidden, acts, seed, dtype=torch.float32):
    """(actors, critics): one pair per entry of acts, randomised"""
    torch.manual_seed(seed)                                                 # (the modules' own initialisation draws from the global generator)
    g = torch.Generator().manual_seed(seed)
    actors, critics = [], []
    for a in acts:
        actor, critic = mm.Actor(5, a, hidden, 0), mm.Critic(7, hidden, 0)
        mm.randomize(actor, g)
        mm.randomize(critic, g)
        actors.append(actor.to(device, dtype))
        critics.append(critic.to(device, dtype))
    return actors, critics


def modules_forward(fa, fc, actors, critics):
    """what update_heads replaces: the modules, per network"""
    hs = [a.act.action_out for a in actors]
    return ([h.fc_mean(f) for h, f in zip(hs, fa)], [torch.sigmoid(h.log_std / h.std_x_coef) * h.std_y_coef for h in hs],
            [c.v_out(f) for c, f in zip(critics, fc)])


def _head_grads(actors, critics):
    out = {}
    for i, (a, c) in enumerate(zip(actors, critics)):
        h = a.act.action_out
        for name, p in (("fc_mean.weight", h.fc_mean.weight), ("fc_mean.bias", h.fc_mean.bias), ("log_std", h.log_std), ("v_out.weight", c.v_out.weight),
                        ("v_out.bias", c.v_out.bias)):
            out["%d.%s" % (i, name)] = None if p.grad is None else p.grad.detach().clone()
    return out


def _evaluate(fn, device, dtype, hidden, acts, seed, M):
    """outputs, feature gradients and parameter gradients of a random linear functional of fn's outputs"""
    actors, critics = _nets(device, hidden, acts, seed, dtype)
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g).to(device, dtype)
    fa = [rn(M, hidden).requires_grad_(True) for _ in acts]
    fc = [rn(M, hidden).requires_grad_(True) for _ in acts]
    mus, stds, values = fn(fa, fc, actors, critics)
    outs = {}
    loss = 0.0
    for i, a in enumerate(acts):
        assert tuple(mus[i].shape) == (M, a) and tuple(stds[i].shape) == (a,) and tuple(values[i].shape) == (M, 1)
        for name, t in (("mu", mus[i]), ("std", stds[i]), ("value", values[i])):
            outs["%d.%s" % (i, name)] = t.detach()
            loss = loss + (t * rn(*t.shape)).sum()
    loss.backward()
    for i in range(len(acts)):
        outs["%d.dfa" % i], outs["%d.dfc" % i] = fa[i].grad, fc[i].grad
    outs.update(_head_grads(actors, critics))
    return outs


# ---- 1. update_heads against the modules ---------------------------------------------------------------------------------------------------
def check_update_heads(device, hidden, acts=(3, 1, 16), M=37):
    pool = bu._Pool()
    for draw in range(DRAWS):
        seed = 100 * hidden + 10 * draw
        truth = _evaluate(modules_forward, "cpu", torch.float64, hidden, acts, seed, M)
        yard = _evaluate(modules_forward, device, torch.float32, hidden, acts, seed, M)
        got = _evaluate(heads.update_heads, device, torch.float32, hidden, acts, seed, M)
        assert truth.keys() == got.keys()
        for name, t in truth.items():
            assert got[name] is not None, name
            assert float((yard[name].detach().cpu().double() - t.cpu()).norm()) <= 1e-4 * float(t.norm()), (name, "the evaluations are not of one problem")
            pool.add(name, got[name], yard[name], t)
    pool.gate("%s/marl_head_update_heads_H%d" % (rc._where(device), hidden))


def _counted(device, fn):
    """fn() with the two entries' calls counted: (fn's result, {entry: calls})"""
    L, _, _ = _lib.for_device(device)
    calls = {k: [] for k in ENTRIES}
    restore = [gu.count(L, k, v) for k, v in calls.items()]
    try:
        res = fn()
    finally:
        for r in restore:
            r()
    return res, {k: len(v) for k, v in calls.items()}


def check_chunks(device, hidden=8, M=5):
    """33 agents (66 networks): three forward calls and, with the size queries, six backward calls; every network has the bits of a call on
    its own agent alone"""
    acts = tuple([3, 1, 5] * 11)

    def run(sel):
        actors, critics = _nets(device, hidden, acts, 3)
        actors, critics = [actors[i] for i in sel], [critics[i] for i in sel]
        g = torch.Generator().manual_seed(4)
        feats = [torch.randn(M, hidden, generator=g).to(device).requires_grad_(True) for _ in range(2 * len(acts))]
        fa, fc = [feats[2 * i] for i in sel], [feats[2 * i + 1] for i in sel]
        mus, stds, values = heads.update_heads(fa, fc, actors, critics)
        k = len(acts)                                                       # (one weight per output, the same in every selection)
        sum((m * (i + 1.5)).sum() + (s * (k + i + 1.5)).sum() + (v * (2 * k + i + 1.5)).sum() for i, m, s, v in zip(sel, mus, stds, values)).backward()
        return mus, stds, values, fa, fc, actors, critics

    everyone = list(range(len(acts)))
    (mus, stds, values, fa, fc, actors, critics), calls = _counted(device, lambda: run(everyone))
    assert calls == {ENTRIES[0]: 3, ENTRIES[1]: 6}, calls                  # 66 networks: chunks of 32, 32 and 2; a size query per backward call
    grads = _head_grads(actors, critics)
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values()) and all(f.grad is not None for f in fa + fc)
    for i in (0, 30, 31, 32):                                               # (actor i is network i of the call, critic i network 33 + i: both sides of both chunk ends)
        m1, s1, v1, fa1, fc1, a1, c1 = run([i])
        assert torch.equal(m1[0], mus[i]) and torch.equal(s1[0], stds[i]) and torch.equal(v1[0], values[i]), i
        assert torch.equal(fa1[0].grad, fa[i].grad) and torch.equal(fc1[0].grad, fc[i].grad), i
        alone = _head_grads(a1, c1)
        for name, v in alone.items():
            assert torch.equal(v, grads["%d.%s" % (i, name.split(".", 1)[1])]), (i, name)


def check_no_grad_networks(device, hidden=36, M=9):
    """A network whose inputs need no gradient is left out of the backward call: its gradients are None, the others keep their bits;
    update_actor=False does that to every actor; under no_grad nothing is recorded"""
    acts = (3, 2)
    full = _evaluate(heads.update_heads, device, torch.float32, hidden, acts, 9, M)

    def frozen(fa, fc, actors, critics):
        for p in actors[0].parameters():
            p.requires_grad_(False)
        fa[0].requires_grad_(False)
        return heads.update_heads(fa, fc, actors, critics)

    part = _evaluate(frozen, device, torch.float32, hidden, acts, 9, M)
    off = _evaluate(lambda fa, fc, a, c: heads.update_heads(fa, fc, a, c, update_actor=False), device, torch.float32, hidden, acts, 9, M)
    actor_keys = ("dfa", "fc_mean.weight", "fc_mean.bias", "log_std")
    for name, v in full.items():
        i, key = name.split(".", 1)
        if key in actor_keys and i == "0":
            assert part[name] is None, name
        else:
            assert torch.equal(part[name], v), name
        if key in actor_keys:
            assert off[name] is None, name
        else:
            assert torch.equal(off[name], v), name
    actors, critics = _nets(device, hidden, acts, 9)
    g = torch.Generator().manual_seed(10)
    feats = [torch.randn(M, hidden, generator=g).to(device) for _ in range(4)]
    with torch.no_grad():
        mus, stds, values = heads.update_heads(feats[:2], feats[2:], actors, critics)
    assert torch.equal(mus[0], full["0.mu"]) and not any(t.requires_grad for t in mus + stds + values)


def check_refusals(device):
    """check_heads refuses what the entries do not take, and with the key on so do both trainers' constructors; without the key the same
    policies are taken"""
    import pytest
    nn = torch.nn

    def policy(hidden=32, change=None):
        p = bu.Policy(device, seed=71, hidden=hidden)
        if change is not None:
            change(p)
        return p

    head = lambda p: p.actor.act.action_out
    cases = {
        "17 actions": lambda p: (setattr(head(p), "fc_mean", nn.Linear(32, 17).to(device)), setattr(head(p), "log_std", nn.Parameter(torch.ones(17, device=device)))),
        "fc_mean without bias": lambda p: setattr(head(p), "fc_mean", nn.Linear(32, bu.ACT, bias=False).to(device)),
        "v_out without bias": lambda p: setattr(p.critic, "v_out", nn.Linear(32, 1, bias=False).to(device)),
        "float64 fc_mean": lambda p: head(p).fc_mean.double(),
        "float64 log_std": lambda p: setattr(head(p), "log_std", nn.Parameter(torch.ones(bu.ACT, dtype=torch.float64, device=device))),
        "float64 v_out": lambda p: p.critic.v_out.double(),
        "v_out with two outputs": lambda p: setattr(p.critic, "v_out", nn.Linear(32, 2).to(device)),
        "v_out of another width": lambda p: setattr(p.critic, "v_out", nn.Linear(36, 1).to(device)),
        "std_x_coef 0": lambda p: setattr(head(p), "std_x_coef", 0.0),
    }
    for algo in ("MAPPO", "HAPPO"):
        cls = getattr(tr, algo)
        assert cls(mlc.trainer_config(fused_head_update=True), policy(), device)._fused_head_update
        assert not cls(mlc.trainer_config(), policy(), device)._fused_head_update
        for name, change in cases.items():
            with pytest.raises(NotImplementedError):
                cls(mlc.trainer_config(fused_head_update=True), policy(change=change), device)
            cls(mlc.trainer_config(), policy(change=change), device)                                 # without the key: as before
        for hidden in (6, 1028):
            with pytest.raises(NotImplementedError):
                cls(mlc.trainer_config(fused_head_update=True), policy(hidden), device)
            cls(mlc.trainer_config(fused_head_update=False), policy(hidden), device)
    p = policy(36)
    assert heads.check_heads([p.actor], [p.critic]) == (36, 1.0, 0.5)
    with pytest.raises(NotImplementedError):
        heads.check_heads([p.actor, policy(32).actor], [p.critic])


# ---- 2. the trainers' routes ------------------------------------------------------------------------------------------------------------------
def check_update(device, algo, route, hidden):
    """ppo_update with fused_head_update on against off on one route: every parameter gradient inside the gate, the six returned values
    equal to the fp32 level, and the entries were called (with the key off: never)"""
    pool = bu._Pool()
    for draw in range(bu.UPDATE_DRAWS):
        config, policy, sample = bu.make_sample(device, algo, route, hidden, seed=10 * draw)
        truth = bu._float64_grads(algo, config, policy, sample, device)
        (off, g_off), calls_off = _counted(device, lambda: uc._run(algo, config, policy, device, sample))
        (on, g_on), calls_on = _counted(device, lambda: uc._run(algo, dict(config, fused_head_update=True), policy, device, sample))
        assert calls_off == {ENTRIES[0]: 0, ENTRIES[1]: 0} and calls_on == {ENTRIES[0]: 1, ENTRIES[1]: 2}, (calls_off, calls_on)
        for nm, a, b in zip(uc.NAMES, on, off):
            assert torch.allclose(torch.as_tensor(a, dtype=torch.float32).cpu(), torch.as_tensor(b, dtype=torch.float32).cpu(), atol=1e-5, rtol=1e-5), (nm, a, b)
        for name, t in truth.items():
            assert t is not None and g_on[name] is not None, name
            pool.add(name, g_on[name], g_off[name], t)
    pool.gate("%s/marl_head_update_%s_%s_H%d" % (rc._where(device), algo, route, hidden))


def check_actor_frozen(device, route, algo="MAPPO", hidden=36):
    """update_actor=False with the key on, under real Adam optimizers: the actor's parameters are the same bits afterwards and none of
    them has a gradient; the critic's have gradients and have moved"""
    config, policy, sample = bu.make_sample(device, algo, route, hidden)
    p = copy.copy(policy)
    p.actor, p.critic = copy.deepcopy(policy.actor), copy.deepcopy(policy.critic)
    p.actor_optimizer = torch.optim.Adam(p.actor.parameters(), lr=5e-4, eps=1e-5)
    p.critic_optimizer = torch.optim.Adam(p.critic.parameters(), lr=5e-4, eps=1e-5)
    out = getattr(tr, algo)(dict(config, fused_head_update=True), p, device).ppo_update(sample, update_actor=False)
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in out)
    for (n, a), b in zip(p.actor.named_parameters(), policy.actor.parameters()):
        assert torch.equal(a, b) and (a.grad is None or float(a.grad.abs().max()) == 0.0), ("actor", n)
    for (n, a), b in zip(p.critic.named_parameters(), policy.critic.parameters()):
        assert a.grad is not None and float(a.grad.abs().max()) > 0.0 and not torch.equal(a, b), ("critic", n)


# ---- 3. the lockstep route --------------------------------------------------------------------------------------------------------------------
def check_group_routes(device, G, hidden, update_actor=True):
    """MAPPO.train_group against the agent loop with the key on: equal bits (marl_grouped_update_check.routes asserts them)"""
    kw = dict(hidden=hidden, fused_head_update=True)
    if hidden < 128:
        kw.update(T=4, N=8)
    return gu.routes(device, G, gu.config(**kw), update_actor=update_actor)


def check_call_counts(device):
    """The heads entries' calls per train_group do not grow from 2 to 6 agents (one forward, one size query and one backward per step);
    with the key off they are never called"""
    from massive_marl_benchmark_amd.algorithms.marl.trainer import MAPPO
    seen = {}
    for key in (True, False):
        for G in (2, 6):
            cfg = gu.config(hidden=8, T=4, N=8, fused_head_update=key)
            trainers, buffers = gu.make(device, G, cfg)
            torch.manual_seed(5)
            _, seen[key, G] = _counted(device, lambda: MAPPO.train_group(trainers, buffers))
    steps = 2 * 2                                                           # gu.config: ppo_epoch 2, num_mini_batch 2
    assert seen[True, 2] == seen[True, 6] == {ENTRIES[0]: steps, ENTRIES[1]: 2 * steps}, seen
    assert seen[False, 2] == seen[False, 6] == {ENTRIES[0]: 0, ENTRIES[1]: 0}, seen

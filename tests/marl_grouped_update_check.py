"""Checks of the lockstep MAPPO update (trainer.MAPPO.train_group) and of Runner's `grouped_update`, shared by the CPU-build tests
(test_marl_grouped_update.py) and the GPU tests (test_marl_grouped_update_gpu.py).

The yardstick is the loop the grouped route replaces: two copies of trainers, buffers and optimizers built from the same seeds, one
runs `trainer.train(buffer)` agent by agent in a given order, the other MAPPO.train_group in that order.  Every network goes through
the same functions on the same values in both and nothing in them depends on the order across agents, so everything is compared with
torch.equal: every parameter, Adam's moments and step counts, the normalisers, the train_info values (under float()) and torch's
generator state.  No tolerance lives here.

Networks: observation width 11, shared observation width 23, A = 3, two blocks; hidden 128 with T = 8, N = 32, ppo_epoch 2,
num_mini_batch 2 (128-row minibatches, the smallest M the f16x2 products take); hidden 8 with M = 16 for 17 agents (34 networks: across
mlp_base's chunk of 32) and hidden 4 with M = 8 for 33 agents (across the loss entry's chunk)."""
import tempfile

import torch

import marl_loss_check as mc
import marl_modules as mm
import marl_runner_check as mr
from massive_marl_benchmark_amd import _lib
from massive_marl_benchmark_amd.optim import FusedAdam

OBS, SOBS, ACT = 11, 23, 3
KEYS = ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio")


def config(hidden=128, T=8, N=32, **over):
    c = mr.config("mappo", run_dir=None, hidden_size=hidden, layer_N=1, episode_length=T, n_rollout_threads=N, ppo_epoch=2, num_mini_batch=2, clip_param=mc.CLIP,
                  value_loss_coef=0.7, entropy_coef=0.01, max_grad_norm=0.5, huber_delta=mc.DELTA, use_valuenorm=False, use_popart=True,
                  fused_block_update=True)
    c.update(over)
    return c


def make(device, G, cfg, fused_adam=True, obs=OBS, seed=0):
    """(trainers, buffers) of G MAPPO agents with randomised parameters and filled buffers"""
    from massive_marl_benchmark_amd.algorithms.marl.policy import MAPPO_Policy
    from massive_marl_benchmark_amd.algorithms.marl.trainer import MAPPO
    o, s, a = mr.spaces(obs, SOBS, ACT)
    trainers, buffers = [], []
    for g in range(G):
        torch.manual_seed(seed + g)
        policy = MAPPO_Policy(cfg, o, s, a, device=torch.device(device))
        gen = torch.Generator().manual_seed(seed + 100 + g)
        mm.randomize(policy.actor, gen)
        mm.randomize(policy.critic, gen)
        if fused_adam:
            policy.actor_optimizer, policy.critic_optimizer = FusedAdam.from_torch(policy.actor_optimizer), FusedAdam.from_torch(policy.critic_optimizer)
        trainers.append(MAPPO(cfg, policy, device=torch.device(device)))
        buf = mc.make_buffer("separated", cfg, obs, SOBS, ACT, device)
        if not cfg.get("use_recurrent_policy"):
            mc.fill_buffer(buf, policy, seed + 200 + g, device)
        buffers.append(buf)
    return trainers, buffers


def state(trainers, buffers=()):
    """Everything an update may change, by name, as clones"""
    out = {}
    for g, t in enumerate(trainers):
        for tag, net, opt in (("actor", t.policy.actor, t.policy.actor_optimizer), ("critic", t.policy.critic, t.policy.critic_optimizer)):
            for n, p in net.named_parameters():
                out["%d.%s.%s" % (g, tag, n)] = p.detach().clone()
                for k, v in opt.state.get(p, {}).items():
                    out["%d.%s.%s.%s" % (g, tag, n, k)] = torch.as_tensor(v).detach().clone()
        if t.value_normalizer is not None:
            for k, v in t.value_normalizer.state_dict().items():
                out["%d.norm.%s" % (g, k)] = v.detach().clone()
    for g, b in enumerate(buffers):
        for k, v in vars(b).items():
            if torch.is_tensor(v):
                out["%d.buffer.%s" % (g, k)] = v.detach().clone()
    out["rng"] = torch.get_rng_state()
    return out


def assert_equal_states(a, b):
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    differ = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not differ, ("not the sequential loop's bits", len(differ), differ[:8])


def count(L, name, calls):
    real = getattr(L, name)
    setattr(L, name, lambda *a: (calls.append(1), real(*a))[1])
    return lambda: setattr(L, name, real)


def routes(device, G, cfg, order=None, fused_adam=True, update_actor=True, counts=None):
    """Both routes from equal states in `order` (default: a non-identity one); asserts the equality of the module docstring and returns
    (sequential infos, grouped infos).  counts: receives the three entries' call counts of the grouped route."""
    from massive_marl_benchmark_amd.algorithms.marl.trainer import MAPPO
    order = list(order) if order is not None else [g for g in range(1, G)] + [0]
    trainers, buffers = make(device, G, cfg, fused_adam)
    other_t, other_b = make(device, G, cfg, fused_adam)                # (the same seeds: a second copy of everything, optimizers included)
    start = state(trainers)
    assert_equal_states(state(trainers, buffers), state(other_t, other_b))
    torch.manual_seed(5)
    seq = []
    for g in order:
        trainers[g].prep_training()
        seq.append(trainers[g].train(buffers[g], update_actor))
    after_seq = state(trainers, buffers)
    moved = [k for k in start if k != "rng" and not torch.equal(start[k], after_seq[k])]
    assert len(moved) >= G, "the updates did not move the networks"
    torch.manual_seed(5)
    for t in other_t:
        t.prep_training()
    L, _, _ = _lib.for_device(device)
    calls = {"mms_marl_ppo_loss": [], "mms_marl_ppo_loss_group": [], "mms_elu_ln_group": []}
    restore = [count(L, k, v) for k, v in calls.items()]
    try:
        grp = MAPPO.train_group([other_t[g] for g in order], [other_b[g] for g in order], update_actor)
    finally:
        for r in restore:
            r()
    assert_equal_states(after_seq, state(other_t, other_b))
    assert len(grp) == len(seq)
    for a, b in zip(seq, grp):
        assert tuple(a) == KEYS == tuple(b)
        for k in KEYS:
            assert float(a[k]) == float(b[k]) and isinstance(b[k], float), (k, float(a[k]), b[k])
    steps = cfg["ppo_epoch"] * cfg["num_mini_batch"]
    assert not calls["mms_marl_ppo_loss"] and len(calls["mms_marl_ppo_loss_group"]) == 2 * steps * ((G + 31) // 32), {k: len(v) for k, v in calls.items()}
    if counts is not None:
        counts.update({k: len(v) for k, v in calls.items()})
    return seq, grp


def check_elu_ln_count_does_not_grow(device):
    """mms_elu_ln_group calls per train_group: the same for 2, 3 and 16 agents (32 networks: one chunk)"""
    seen = []
    for G in (2, 3, 16):
        counts = {}
        routes(device, G, config(hidden=8, T=4, N=8), counts=counts)
        seen.append(counts["mms_elu_ln_group"])
    assert seen[0] > 0 and len(set(seen)) == 1, seen


def check_refusals(device):
    """What train_group does not take raises NotImplementedError and leaves parameters, optimizer states, normalisers, buffers and the
    generator as they were"""
    from massive_marl_benchmark_amd.algorithms.marl.trainer import MAPPO
    cfg = config(hidden=8, T=4, N=8)
    cases = {}
    t, b = make(device, 2, cfg)
    t2, b2 = make(device, 1, cfg, obs=OBS + 1)
    cases["unequal width"] = (t + t2, b + b2)
    t2, b2 = make(device, 1, dict(cfg, clip_param=0.3))
    cases["unequal clip_param"] = (t + t2, b + b2)
    t2, b2 = make(device, 1, dict(cfg, use_recurrent_policy=True, fused_block_update=True))
    cases["a recurrent trainer"] = (t2 + t, b2 + b)
    t2, b2 = make(device, 1, dict(cfg, fused_block_update=False))
    cases["without fused_block_update"] = (t + t2, b + b2)
    for label, (trainers, buffers) in cases.items():
        torch.manual_seed(3)
        before = state(trainers, buffers)
        try:
            MAPPO.train_group(trainers, buffers)
        except NotImplementedError as e:
            assert str(e), label
        else:
            raise AssertionError("train_group took " + label)
        assert_equal_states(before, state(trainers, buffers))


# ---- Runner ------------------------------------------------------------------------------------------------------------------------------
def _copy_tensors(dst, src):
    for k, v in vars(src).items():
        if torch.is_tensor(v):
            getattr(dst, k).copy_(v)


def check_runner(device_type, shared, fused_factor):
    """Runner.train() with grouped_update on and off from equal states (one rollout on TenAnt at 64 envs, copied into the second runner):
    the policies, every buffer's factor, last_factor and train_infos in their order; happo with the key on raises at construction"""
    from massive_marl_benchmark_amd.algorithms.marl.runner import Runner
    import pytest
    env = mr.make_env(device_type)
    over = dict(shared_buffers=shared, fused_factor=fused_factor, fused_block_update=True, ppo_epoch=2, num_mini_batch=2)
    runners = []
    for grouped in (False, True):
        torch.manual_seed(0)
        r = Runner(env, mr.config("mappo", run_dir=tempfile.mkdtemp(), grouped_update=grouped, **over))
        if not runners:
            r.warmup()
            for step in range(r.episode_length):
                values, actions, logp, rs, rsc = r.collect(step)
                if r.shared is not None:
                    rewards, dones = r.shared.env_step(actions)
                    obs = share_obs = infos = None
                else:
                    obs, share_obs, rewards, dones, infos, _ = r.envs.step(actions)
                r.insert((obs, share_obs, rewards, dones, infos, values, actions, logp, rs, rsc))
            r.compute()
        else:
            first = runners[0]
            for a in range(r.num_agents):
                r.policy[a].actor.load_state_dict(first.policy[a].actor.state_dict())
                r.policy[a].critic.load_state_dict(first.policy[a].critic.state_dict())
                if r.trainer[a].value_normalizer is not None:
                    r.trainer[a].value_normalizer.load_state_dict(first.trainer[a].value_normalizer.state_dict())
                _copy_tensors(r.buffer[a], first.buffer[a])
            if r.shared is not None:
                _copy_tensors(r.shared, first.shared)
        runners.append(r)
    assert not runners[0].grouped_update and runners[1].grouped_update
    results = []
    for r in runners:
        torch.manual_seed(11)
        infos = r.train()
        results.append((infos, state(r.trainer), [b.factor.clone() for b in r.buffer], r.last_factor.clone()))
    (ia, sa, fa, la), (ib, sb, fb, lb) = results
    assert_equal_states(sa, sb)
    assert all(torch.equal(x, y) for x, y in zip(fa, fb)) and torch.equal(la, lb) and float((la - 1).abs().max()) > 0
    assert len(ia) == len(ib) == runners[0].num_agents
    for x, y in zip(ia, ib):
        assert all(float(x[k]) == float(y[k]) for k in KEYS), (x, y)
    for algo in ("happo", "hatrpo"):
        with pytest.raises(NotImplementedError, match="one after another"):
            Runner(env, mr.config(algo, run_dir=tempfile.mkdtemp(), grouped_update=True, fused_block_update=True))
    with pytest.raises(NotImplementedError, match="fused_block_update"):
        Runner(env, mr.config("mappo", run_dir=tempfile.mkdtemp(), grouped_update=True))
    with pytest.raises(NotImplementedError, match="feed-forward"):
        Runner(env, mr.config("mappo", run_dir=tempfile.mkdtemp(), grouped_update=True, fused_block_update=True, use_recurrent_policy=True))

"""TRPO's ActorCritic on the GPU: the actor's backward (mms_mlp_grad) and R-op (mms_mlp_grad_rop) at the shipped shape against float64
torch autograd, with torch fp32 autograd's own error as the bound; HIP against the CPU build; determinism; the rollout after an
update."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from trpo_check import CFG_SHIPPED, hvp_parts, make_actor, rms, within_torch  # noqa: E402


def _paths(ac, obs, act, old_mu, v):
    """(mu, flat J^T g of the surrogate, KL gradient, HVP) for the fused module, torch fp32 and float64."""
    ref = copy.deepcopy(ac).double()
    ref.fused_grad = False
    t32 = copy.deepcopy(ac)
    t32.fused_grad = False
    out = {}
    for name, m, dt in (("fused", ac, torch.float32), ("torch32", t32, torch.float32), ("f64", ref, torch.float64)):
        out[name] = [t.double() for t in hvp_parts(m, obs.to(dt), act.to(dt), old_mu.to(dt), v.to(dt))]
    return out


@pytest.mark.parametrize("moved", [False, True])
def test_shipped_shape_against_float64(moved):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    ac, obs, act, old_mu, v = make_actor((388,), 80, CFG_SHIPPED, 8192, dev, moved)
    r = _paths(ac, obs, act, old_mu, v)
    errs = [(rms(r["fused"][i] - r["f64"][i]), rms(r["torch32"][i] - r["f64"][i]), rms(r["f64"][i])) for i in range(4)]
    for what, (ef, et, scale) in zip(("mu", "surrogate gradient", "KL gradient", "HVP"), errs):
        print("%s (moved=%s): fused %.3e, torch fp32 %.3e, scale %.3e" % (what, moved, ef, et, scale))
    assert within_torch(errs) == []


def test_hip_against_cpu_build_small():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg = {"pi_hid_sizes": [32, 24, 16], "vf_hid_sizes": [32, 24, 16], "activation": "elu"}
    ac, obs, act, old_mu, v = make_actor((20,), 6, cfg, 40, torch.device("cpu"), True)
    cpu = [t.double() for t in hvp_parts(ac, obs, act, old_mu, v)]
    g = copy.deepcopy(ac).cuda()
    gpu = [t.double().cpu() for t in hvp_parts(g, obs.cuda(), act.cuda(), old_mu.cuda(), v.cuda())]
    for a, b in zip(gpu, cpu):
        assert rms(a - b) <= 1e-5 * max(rms(b), 1e-30), (rms(a - b), rms(b))


def test_hvp_deterministic():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    ac, obs, act, old_mu, v = make_actor((388,), 80, {"pi_hid_sizes": [256, 256], "vf_hid_sizes": [256, 256], "activation": "elu"}, 2048, dev, True)
    a = hvp_parts(ac, obs, act, old_mu, v)
    b = hvp_parts(ac, obs, act, old_mu, v)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_act_after_data_copy():
    """set_pi_flat_params writes .data in place: the next rollout's act() must see the new weights."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    cfg = {"pi_hid_sizes": [256, 256, 128], "vf_hid_sizes": [256, 256, 128], "activation": "elu"}
    ac, obs, act, old_mu, v = make_actor((388,), 80, cfg, 1024, dev, False)
    hvp_parts(ac, obs, act, old_mu, v)
    flat = torch.cat([p.data.view(-1) for p in ac.actor.parameters()])
    flat = flat + 0.01 * torch.randn_like(flat)
    i = 0
    for p in ac.actor.parameters():
        p.data.copy_(flat[i:i + p.numel()].view(p.size()))
        i += p.numel()
    with torch.no_grad():
        _, _, _, mu, _ = ac.act(obs, obs)
        ref = ac.actor(obs)
    assert rms((mu - ref).double()) <= 1e-5 * rms(ref.double())


def test_minibatch_sequence_against_float64():
    """grad, CG (3 steps), sAs, line search and the .data writes, fused against the float64 sequence, with torch fp32 autograd's own
    deviation from float64 as the yardstick (the fused path may be at most 2x it: CG's three HVPs and dot products amplify rounding
    differences by an input-dependent factor), at the shipped widths and 2048 rows."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trpo_check import minibatch_sequence
    dev = torch.device("cuda:0")
    ac, obs, act, old_mu, v = make_actor((388,), 80, CFG_SHIPPED, 2048, dev, True)
    gen = torch.Generator().manual_seed(11)
    adv = torch.randn(2048, 1, generator=gen).to(dev)
    with torch.no_grad():
        old_logp = ac.evaluate(obs, None, act)[0].unsqueeze(-1) + 0.05 * torch.randn(2048, 1, generator=gen).to(dev)
    old_sigma = ac.log_std.detach().repeat(2048, 1)
    hyper = (0.1, 3, 0.1, 10, 0.01, 0.1)                  # cfg/trpo: damping, cg_nsteps, max_kl, max_num_backtrack, accept_ratio, step_fraction
    runs = {}
    for name, dt, fused in (("fused", torch.float32, True), ("torch32", torch.float32, False), ("f64", torch.float64, False)):
        m = copy.deepcopy(ac).to(dt)
        m.fused_grad = fused
        c = lambda t: t.to(dt)                            # noqa: E731
        runs[name] = minibatch_sequence(m, c(obs), c(act), c(adv), c(old_logp), c(old_mu), c(old_sigma), c(v), *hyper)
    ref = runs["f64"]
    assert runs["fused"]["success"] == runs["torch32"]["success"] == ref["success"]
    assert runs["fused"]["tries"] == ref["tries"]
    for k in ("step_dir", "full_step", "params_after"):
        ef, et = rms(runs["fused"][k].double() - ref[k]), rms(runs["torch32"][k].double() - ref[k])
        print("%s: fused %.3e, torch fp32 %.3e, scale %.3e" % (k, ef, et, rms(ref[k])))
        assert ef <= max(2.0 * et, 2.0 ** -24 * rms(ref[k])), (k, ef, et)

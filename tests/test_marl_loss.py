"""The MAPPO / HAPPO update's loss head (mms_marl_ppo_loss; algorithms/marl/loss.py: marl_ppo_loss; algorithms/marl/trainer.py: MAPPO,
HAPPO; utils/valuenorm.py) without a GPU: the symbol in both libraries, the yardstick and the CPU build pinned to the reference's
trainers (tests/golden/marl_ppo_loss.npz: every flag combination), the CPU build of the entry against float64 next to torch fp32
(marl_loss_check.py) at every shape and flag set, its exact properties -- run to run and workspace content, indices = arange against
NULL, a repeating index vector against the gathered rows, terms only, row_logp, masked rows -- pitched storage, the error paths, the
autograd function against the torch expression, the torch fallbacks, the value normaliser against the reference's state, and the
trainers: train() against a loop of ppo_update, one ppo_update against the reference's sequence in torch, the ValueNorm quirk."""
import os
import subprocess

import numpy as np
import pytest
import torch

import marl_loss_check as mc
from conftest import ROOT, load_golden
from massive_marl_benchmark_amd import _lib

SHAPES = [(1, 1), (7, 8), (257, 1), (1000, 80), (4099, 8), (333, mc.MAX_A), (1000, 6)]


def _cpu():
    return _lib.lib_cpu(), -1, None


def test_symbol_declared_and_exported():
    from massive_marl_benchmark_amd.algorithms.marl import loss as loss_mod
    assert "mms_marl_ppo_loss" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "int mms_marl_ppo_loss(" in hdr and "#define MMS_MARL_LOSS_MAX_A %d" % mc.MAX_A in hdr and "#define MMS_ABI_VERSION 4" in hdr
    assert loss_mod.MAX_A == mc.MAX_A == 128
    for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc")])
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert " T mms_marl_ppo_loss\n" in out, path


# ---- the reference's fixture ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("marl_ppo_loss")


def _fixture_problem(g, flags):
    """The fixture's minibatch as a problem, with the flag combination of one of its cases; PopArt's statistics are those of a fresh
    normaliser that took the returns in twice (cal_value_loss calls PopArt's forward once per error), ValueNorm leaves the targets raw."""
    from massive_marl_benchmark_amd.algorithms.marl.utils.valuenorm import ValueNorm
    happo, norm, huber, clipped, pm, vm = (int(x) for x in flags)
    t = lambda k: torch.from_numpy(g[k])
    M, A = g["mu"].shape
    clip, delta, value_coef, entropy_coef = (float(x) for x in g["constants"])
    pr = dict(M=M, A=A, mu=t("mu"), std=t("std"), value=t("value").view(-1), actions=t("actions"), old_logp=t("old_logp"),
              **{k: t(k).view(-1) for k in mc.NARROW}, norm_mean=torch.zeros(1), norm_var=torch.ones(1))
    n = ValueNorm(1)
    if norm == 1:
        n(t("returns"))
        n(t("returns"))
        pr["norm_mean"], pr["norm_var"] = n.running_mean_var()
    c = mc.cfg(huber=huber, clipped=clipped, pm=pm, vm=vm, norm=int(norm == 1), factor=happo, value_coef=value_coef, entropy_coef=entropy_coef, clip=clip, delta=delta)
    return pr, c, n


def test_yardstick_and_cpu_build_are_the_reference(golden):
    """Every case of the fixture: the checker's float64 expression and the CPU build's outputs against what the reference's ppo_update
    returned and autograd left in the leaves (fp32 values: 2e-5 of the tensor's largest magnitude); rows with e < -d: exactly 0."""
    g = golden
    L, dev, stream = _cpu()
    names = [str(x) for x in g["case_names"]]
    assert len(names) == 56 and len(set(names)) == 56
    dstd_dlog = torch.from_numpy(g["std"]).double() * (1.0 - 2.0 * torch.from_numpy(g["std"]).double())       # std = 0.5 sigmoid(log_std)
    zero_rows = 0
    for i, name in enumerate(names):
        pr, c, n = _fixture_problem(g, g["case_flags"][i])
        if "c%d_norm_state" % i in g:
            state = torch.tensor([float(n.running_mean), float(n.running_mean_sq), float(n.debiasing_term)])
            assert torch.equal(state, torch.from_numpy(g["c%d_norm_state" % i])), name
        want = {"policy_loss": g["c%d_scalars" % i][0], "value_loss": g["c%d_scalars" % i][1], "dist_entropy": g["c%d_scalars" % i][2],
                "ratio": g["c%d_scalars" % i][3], "dmu": g["c%d_dmu" % i], "dlog_std": g["c%d_dlog_std" % i], "dvalue": g["c%d_dvalue" % i].reshape(-1)}
        y = mc.expression(pr, torch.float64, c)
        out = mc.run(L, dev, stream, pr, c)
        assert out["guards"] and out["ws_outside"]
        for label, got in (("yardstick", y), ("cpu build", out["out"])):
            got = dict(got, dlog_std=got["dstd"].double() * dstd_dlog)
            for k, w in want.items():
                w = torch.as_tensor(w).double()
                err, top = float((got[k].double() - w).abs().max()), float(w.abs().max())
                assert err <= 2e-5 * max(top, 1e-3), (name, label, k, err, top)
        # the reference's own branch e < -d: loss and gradient exactly 0
        if c["huber"] and not c["norm"]:
            eo = pr["returns"] - pr["value"]
            ec = pr["returns"] - (pr["value_preds"] + (pr["value"] - pr["value_preds"]).clamp(-c["clip"], c["clip"]))
            dead = (eo < -c["delta"] - 1e-3) & ((ec < -c["delta"] - 1e-3) | (c["clipped"] == 0))
            assert int(dead.sum()) >= 5
            zero_rows += int(dead.sum())
            assert bool((torch.from_numpy(want["dvalue"])[dead] == 0).all()) and bool((out["out"]["dvalue"][dead] == 0).all())
            assert bool((y["dvalue"][dead] == 0).all())
    assert zero_rows > 0


def test_value_normaliser_is_the_reference_s(golden):
    """The state after three cal_value_loss calls of the reference's MAPPO: PopArt took every batch in twice, ValueNorm once."""
    from massive_marl_benchmark_amd.algorithms.marl.utils.valuenorm import PopArt, ValueNorm
    batches = torch.from_numpy(golden["norm_batches"])
    for name, per_call in (("popart", 2), ("valuenorm", 1)):
        n = (PopArt if name == "popart" else ValueNorm)(1)
        for b in batches:
            if name == "popart":
                first, second = n(b), n(b)                              # forward: update, then normalise
                assert first.shape == b.shape and float(second.mean().abs()) < 10.0
            else:
                n.update(b)
        mean, var = n.running_mean_var()
        got = torch.stack([n.running_mean[0], n.running_mean_sq[0], n.debiasing_term, mean[0], var[0]])
        assert torch.equal(got, torch.from_numpy(golden[name + "_state3"])), (name, got, golden[name + "_state3"])
        assert torch.allclose(n.denormalize(n.normalize(batches[0])), batches[0], atol=1e-5) and not n.normalize(batches[0]).requires_grad
    assert n.running_mean.device.type == "cpu" and n.running_mean.dtype == torch.float32


# ---- the CPU build against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["shipped", "all"])
@pytest.mark.parametrize("M,A", SHAPES)
def test_cpu_build_against_float64(M, A, flags):
    import parity
    L, dev, stream = _cpu()
    pr = mc.problem(M, A, seed=1)
    print("M %d A %d %s: %d rows drawn again" % (M, A, flags, pr["redraws"]))
    stats = {}
    mc.check(L, dev, stream, pr, dict(mc.FLAG_SETS)[flags], stats=stats)
    parity.record("cpu/marl_loss/M%d_A%d_%s" % (M, A, flags), **{k + "_e_over_et": v["e_over_et"] for k, v in stats.items()})


@pytest.mark.parametrize("flags", [name for name, _ in mc.FLAG_SETS])
def test_each_flag_and_the_shipped_combinations(flags):
    L, dev, stream = _cpu()
    pr = mc.problem(1000, 8, seed=2)
    assert bool((pr["active_masks"] == 0).any())
    mc.check(L, dev, stream, pr, dict(mc.FLAG_SETS)[flags])


def test_regimes_are_populated():
    """The draw reaches every regime at a size the suite uses: r on both sides of the range, the three Huber branches, the clipped branch
    selected, and at M = 7 the forced rows alone provide them."""
    for M in (7, 4099):
        pr = mc.problem(M, 8, seed=1)
        r = torch.exp((mc.logp64(pr["mu"], pr["std"], pr["actions"]) - pr["old_logp"].double()).sum(-1))
        eo = (pr["returns"] - pr["value"]).double()
        d = (pr["value"] - pr["value_preds"]).double()
        assert bool((r > 1 + mc.CLIP).any()) and bool((r < 1 - mc.CLIP).any()) and bool(((r - 1).abs() < mc.CLIP).any())
        assert bool((d.abs() > mc.CLIP).any())
        if M > 7:
            assert bool((eo > mc.DELTA).any()) and bool((eo < -mc.DELTA).any()) and bool((eo.abs() < mc.DELTA).any())
            y = mc.expression(pr, torch.float64, mc.cfg(huber=1, clipped=1))
            frac = float(((y["dvalue"] == 0) & (d.abs() > mc.CLIP) & (eo > -mc.DELTA)).double().mean())
            assert 0.02 < frac < 0.5, frac


def test_rows_in_the_bands_are_left_out_and_counted():
    """A problem as drawn (rows in the bands kept): dmu and dvalue outside the bands, selection sets equal, the cap holds."""
    L, dev, stream = _cpu()
    c = mc.cfg(huber=1, clipped=1, norm=1)
    pr = mc.problem(4099, 8, seed=1, clean=False)
    in_r, in_v = mc.bands(pr)
    assert 0 < int(in_r.sum()) + int(in_v.sum()) <= mc.BAND_CAP * 4099
    res = mc.run(L, dev, stream, pr, c)
    assert not mc.gates(pr, res["out"], c, sums=False)
    assert mc.gates(pr, res["out"], c, sums=True)                        # the sums are not compared on such a problem
    zero = (res["out"]["dmu"] == 0).all(-1) & ~in_r                      # the harness sees a selection flip
    bad = dict(res["out"], dmu=res["out"]["dmu"].clone())
    bad["dmu"][int(zero.nonzero()[0])] = 1e-9
    assert any(f[1] == "selection flips" for f in mc.gates(pr, bad, c, sums=False))


def test_exact_properties():
    L, dev, stream = _cpu()
    mc.exact_properties(L, dev, stream, 1000, 80)
    mc.exact_properties(L, dev, stream, 600, 6, c=mc.cfg(**mc.SHIPPED))


def test_pitched_storage_of_a_shared_block():
    L, dev, stream = _cpu()
    mc.pitched_storage(L, dev, stream)
    mc.pitched_storage(L, dev, stream, A=6, c=mc.cfg(**mc.SHIPPED))


def test_abi_errors():
    L, dev, stream = _cpu()
    mc.check_error_paths(L, dev, stream, other_device=0)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["shipped_happo", "all"])
def test_autograd_function_against_torch(flags):
    mc.autograd_function("cpu", dict(mc.FLAG_SETS)[flags])


def test_inputs_the_entry_does_not_take_fall_back_to_torch():
    mc.fallbacks("cpu")


def test_field_rows_of_buffer_tensors_and_views():
    from massive_marl_benchmark_amd.algorithms.marl.loss import field_rows
    T, N, G, A = 4, 5, 10, 8
    wide, tall = torch.zeros(T, N, G, A), torch.zeros(T + 1, N, G)
    assert field_rows(wide[:, :, 3], A) == (G * A, T * N) and field_rows(torch.zeros(T, N, A), A) == (A, T * N)
    assert field_rows(tall[:, :, 3:4], 1) == (G, (T + 1) * N) and field_rows(torch.zeros(T + 1, N, 1), 1) == (1, (T + 1) * N)
    assert field_rows(torch.zeros(T + 1, N, G, 1)[:, :, 3], 1) == (G, (T + 1) * N) and field_rows(torch.zeros(7), 1) == (1, 7)
    assert field_rows(torch.zeros(T, N, 2 * A)[:, :, ::2], A) is None and field_rows(torch.zeros(T, N + 1, A)[:, :N], A) is None
    assert field_rows(torch.zeros(T, N, A + 1), A) is None and field_rows(torch.zeros(1).expand(7), 1) is None


# ---- the trainers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,kind,over", [("MAPPO", "separated", {}), ("MAPPO", "shared", dict(use_popart=False, use_valuenorm=True)),
                                            ("HAPPO", "shared", {}), ("HAPPO", "separated", dict(use_policy_active_masks=True, use_value_active_masks=True,
                                                                                                 use_popart=False, use_max_grad_norm=False))])
def test_train_equals_a_loop_of_ppo_update(algo, kind, over):
    trainer, info = mc.train_equals_update_loop("cpu", algo, kind, **over)
    assert (trainer.value_normalizer is None) == (not (over.get("use_popart", True) or (algo == "MAPPO" and over.get("use_valuenorm", False))))


@pytest.mark.parametrize("algo,over", [("MAPPO", {}), ("HAPPO", {}), ("MAPPO", dict(use_popart=False, use_valuenorm=True)),
                                       ("MAPPO", dict(use_popart=False, use_huber_loss=False, use_clipped_value_loss=False, use_policy_active_masks=True,
                                                      use_value_active_masks=True))])
def test_ppo_update_against_the_reference_s_sequence(algo, over):
    mc.trainer_update_against_reference("cpu", algo, **over)


def test_valuenorm_quirk_and_happo_factor_are_pinned():
    """MAPPO with ValueNorm: the normaliser is updated, the targets are raw -- the update equals the one without a normaliser bit for
    bit; HAPPO with ValueNorm in its config has no normaliser at all; HAPPO's factor changes the policy loss, MAPPO ignores it."""
    from massive_marl_benchmark_amd.algorithms.marl import trainer as tr
    tv, gv = mc.trainer_update_against_reference("cpu", "MAPPO", use_popart=False, use_valuenorm=True)
    tn, gn = mc.trainer_update_against_reference("cpu", "MAPPO", use_popart=False)
    assert tv.value_normalizer is not None and float(tv.value_normalizer.debiasing_term) > 0 and tn.value_normalizer is None
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(gv, gn))
    th, gh = mc.trainer_update_against_reference("cpu", "HAPPO", use_popart=False, use_valuenorm=True)
    assert th.value_normalizer is None
    assert not torch.equal(gh[2], gn[2]) and torch.equal(gh[0], gn[0])                      # the factor: the policy loss only
    policy = mc.Policy(14, 22, 6, "cpu", seed=1)
    for bad in (dict(use_recurrent_policy=True), dict(use_naive_recurrent_policy=True)):
        with pytest.raises(NotImplementedError):
            tr.MAPPO(mc.trainer_config(**bad), policy, "cpu")
    policy.actor.act.action_out = torch.nn.Linear(4, 4)                                     # not a DiagGaussian: a discrete head
    with pytest.raises(NotImplementedError):
        tr.HAPPO(mc.trainer_config(), policy, "cpu")

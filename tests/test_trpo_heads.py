"""The head of TRPO's policy step (mms_trpo_heads) without a GPU: the symbol in both libraries, the yardstick pinned to the reference's
`evaluate` fixture, the CPU build of the entry against float64 next to torch fp32 (trpo_heads_check.py) at every shape, index mode and
old_logp mode with every output subset's bits, the exact properties, the error paths, the bits it shares with mms_ppo_loss, and three
corruptions of the lane arithmetic that the gates must miss by a stated factor."""
import os
import subprocess

import pytest
import torch

import ppo_loss_check as pc
import trpo_heads_check as tc
from conftest import ROOT, load_golden
from massive_marl_benchmark_amd import _lib


def _cpu():
    return _lib.lib_cpu(), -1, None


def test_symbol_declared_and_exported():
    assert "mms_trpo_heads" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "int mms_trpo_heads(" in hdr and "trpo.py:287-298, 417-435, 464-478" in hdr and "#define MMS_ABI_VERSION 4" in hdr     # an addition
    lane = open(os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc", "trpo_loss_lane.h")).read()
    assert "gkl and gn have the SAME BITS" in lane
    for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc")])
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert " T mms_trpo_heads\n" in out, path


def test_yardstick_is_the_reference_evaluate():
    """logp of the checker's expression, and of the CPU build, against what the reference's ActorCritic.evaluate returned (ppo_act.npz);
    with act's own log-probabilities as old_logp every ratio is 1: a_loss = -mean(adv), and kl = 0 at mu = old_mu, sigma = old_sigma."""
    g = load_golden("ppo_act")
    t = lambda k: torch.from_numpy(g[k])
    M, A = g["mu"].shape
    ref = t("eval_log_prob").double()
    pr = dict(M=M, A=A, mu=t("mu"), log_std=t("log_std"), rmu=t("mu"), actions=t("actions"), adv=torch.ones(M), old_mu=t("mu"), old_sigma=t("sigma"),
              old_logp=t("log_prob").view(-1).contiguous())
    want = tc.expression(pr, torch.float64)
    assert float((want["logp"] - ref).abs().max()) <= 1e-5 * float(ref.abs().max())           # the fixture holds torch's fp32 values
    L, dev, stream = _cpu()
    out = tc.run(L, dev, stream, pr)["out"]
    assert float((out["logp"].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert abs(float(out["a_loss"]) + 1.0) <= 1e-4 and abs(float(out["kl"])) <= 1e-6 and float(out["gkl"].abs().max()) == 0.0


@pytest.mark.parametrize("dense_old_logp", [False, True])
@pytest.mark.parametrize("index_mode", [None, "perm", "repeat"])
@pytest.mark.parametrize("M,A", tc.SHAPES)
def test_cpu_build_against_float64(M, A, index_mode, dense_old_logp):
    L, dev, stream = _cpu()
    tc.check(L, dev, stream, M, A, index_mode, dense_old_logp)


def test_exact_properties():
    L, dev, stream = _cpu()
    tc.exact_properties(L, dev, stream, 1000, 80)
    tc.exact_properties(L, dev, stream, 600, 6)


def test_logp_has_the_bits_of_mms_ppo_loss():
    """The CPU build compiles both entries alike: a_loss, kl and gsur are mms_ppo_loss's unclipped surrogate, kl and dmu bit for bit."""
    L, dev, stream = _cpu()
    for name, (mine, theirs, _) in tc.logp_equals_ppo_loss(L, dev, stream).items():
        assert torch.equal(mine, theirs), name


def test_abi_errors():
    L, dev, stream = _cpu()
    tc.check_error_paths(L, dev, stream, other_device=0)


# ---- the harness proves itself: the lane arithmetic corrupted in the truth must miss the gates by the stated factor -------------------
@pytest.mark.parametrize("mutation,hit,clean,factor", [("inv_m", ("gsur", "gkl", "gn"), ("a_loss", "kl", "logp"), 1e5),
                                                       ("einv", ("logp", "a_loss", "gsur"), ("kl", "gkl", "gn"), 1e3),
                                                       ("old_sigma_den", ("kl", "gkl", "gn"), ("a_loss", "logp", "gsur"), 1e3)])
def test_a_corrupted_lane_statement_misses_the_gate(mutation, hit, clean, factor):
    """1 / M dropped (M = 1000: a factor 1000 on three outputs whose gate is about 1e-6 of their scale); exp(-l) for exp(-2 l) (l about
    -0.3: z changes by a third); old_sigma for l in the KL's denominator (they differ by 0.05 rms: a tenth of the quotient)."""
    L, dev, stream = _cpu()
    pr = tc.problem(1000, 80, 1)
    got = tc.run(L, dev, stream, pr)["out"]
    fails, ratios = tc.gates(pr, got, mutation=mutation)
    assert {f[0] for f in fails} == set(hit), fails
    assert all(ratios[k] >= factor for k in hit) and all(ratios[k] <= 1.0 for k in clean), ratios

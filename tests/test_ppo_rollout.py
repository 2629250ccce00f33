"""The PPO rollout's tail entry by entry (tests/ppo_rollout_check.py) on the CPU build of the C ABI: the output heads, the sampling, the
GAE scans and the MARL views at the small shapes, the refusals, and the proof of the harness: every mutation of a truth must miss its
gate by 100 x the bound.  tests/test_ppo_rollout_gpu.py runs the same list on the HIP build."""
import pytest

import ppo_rollout_check as pc
from massive_marl_benchmark_amd import _lib


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


def test_heads_every_shape():
    worst = {}
    for N, H, A in pc.heads_shapes():
        pc._merge(worst, pc.check_heads(_cpu(), N, H, A))
    pc.report("cpu", "heads", **worst)


@pytest.mark.parametrize("VH", [4, 64, 252, 256, 260, 512, 1024, 1028])
def test_value_head(VH):
    pc.report("cpu", "value_head_VH%d" % VH, **pc.check_value_head(_cpu(), VH))


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_sampling_exact_parts(entry):
    pc.check_sampling_exact(_cpu(), entry)


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_sampling_is_keyed(entry):
    pc.check_keying(_cpu(), entry)


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_draw_and_logp_identity(entry):
    pc.check_draw(_cpu(), entry)


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_sample_moments(entry):
    pc.check_moments(_cpu(), entry)


def test_act_slots_through_ppo_loss():
    pc.check_cross_entry(_cpu())


@pytest.mark.parametrize("regime", pc.GAE_REGIMES)
def test_gae_ppo(regime):
    worst = {}
    for T, N in pc.GAE_SHAPES_SMALL:
        pc._merge(worst, pc.check_gae_ppo(_cpu(), T, N, regime))
    pc.report("cpu", "gae_ppo_%s" % regime, **worst)


@pytest.mark.parametrize("T,N", pc.GAE_SHAPES_CAP)
def test_gae_ppo_past_the_grid_cap(T, N):
    for regime in ("random", "shifted"):
        pc.check_gae_ppo(_cpu(), T, N, regime)


@pytest.mark.parametrize("T,N,A", [(1, 1, 1), (8, 33, 3), (13, 1000, 10), (5, 77, 10), (1, 52430, 10)])
def test_gae_marl(T, N, A):
    pc.report("cpu", "gae_marl_T%d_N%d_A%d" % (T, N, A), **pc.check_gae_marl(_cpu(), T, N, A))


def test_marl_views():
    pc.check_marl_views(_cpu())


def test_refusals():
    assert pc.check_refusals(_cpu()) >= 40


# ---- the harness proves itself: a corrupted truth must miss its gate by 100 x the bound ----------------------------------------------
def test_mutation_actor_product_drops_four_k():
    assert pc.check_heads(_cpu(), 37, 512, 80, mutation="drop_k")["mu"] >= 100


def test_mutation_logp_scale_not_squared():
    assert pc.check_draw(_cpu(), "act", mutation="exp_l")["logp"] >= 100


def test_mutation_counter_off_by_one():
    assert pc.check_draw(_cpu(), "act", mutation="counter")["draw"] >= 100


def test_mutation_value_head_reads_value():
    assert pc.check_heads(_cpu(), 37, 512, 80, mutation="value_from_value")["value"] >= 100


def test_mutation_done_ignored():
    r = pc.check_gae_ppo(_cpu(), 13, 1000, "random", mutation="ignore_done")
    assert r["returns"] >= 100 and r["adv"] >= 100


def test_mutation_biased_std():
    r = pc.check_gae_ppo(_cpu(), 1, 257, "random", mutation="biased")
    assert r["norm_two"] >= 100 and r["norm_normalized"] >= 100


def test_mutation_next_agents_normaliser():
    assert pc.check_gae_marl(_cpu(), 8, 33, 3, mutation="shift_norm")["norm1"] >= 100

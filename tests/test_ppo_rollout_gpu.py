"""The PPO rollout's tail entry by entry (tests/ppo_rollout_check.py) on the MI355X: ppo_head_act_kernel at every column-tile count and
wave count, the 64 KB LDS fallback and (in a fresh child process, MMS_HEAD_RT=2) the 32-rows-per-block form; the value head's dot
product; the sampling of both entries against the restated noise stream; the GAE scans and the views past the launch's 2048-block cap;
the refusals.  Truth is float64 per output element; tests/test_ppo_rollout.py runs the same list on the CPU build."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ppo_rollout_check as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu():
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _lib.for_device("cuda:0")
    return L, dev, stream, "cuda"


@pytest.mark.parametrize("N,H,A", pc.heads_shapes())
def test_heads(torch_cuda, N, H, A):
    pc.report("cuda:0", "heads_N%d_H%d_A%d" % (N, H, A), **pc.check_heads(_gpu(), N, H, A))


@pytest.mark.parametrize("VH", [4, 64, 252, 256, 260, 512, 1024, 1028])
def test_value_head(torch_cuda, VH):
    pc.report("cuda:0", "value_head_VH%d" % VH, **pc.check_value_head(_gpu(), VH))


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_sampling_exact_parts(torch_cuda, entry):
    pc.check_sampling_exact(_gpu(), entry)


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_sampling_is_keyed(torch_cuda, entry):
    pc.check_keying(_gpu(), entry)


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_draw_and_logp_identity(torch_cuda, entry):
    pc.check_draw(_gpu(), entry)


@pytest.mark.parametrize("entry", ["act", "heads"])
def test_sample_moments(torch_cuda, entry):
    pc.check_moments(_gpu(), entry)


def test_act_slots_through_ppo_loss(torch_cuda):
    pc.check_cross_entry(_gpu())


def test_heads_32_rows_per_block(torch_cuda, tmp_path):
    """MMS_HEAD_RT is read once per process: a fresh child with MMS_HEAD_RT=2 dumps every output of the five heads calls
    (ppo_rollout_check.DUMP_CALLS), this process computes them at the default."""
    path = str(tmp_path / "heads_rt2.npz")
    done = subprocess.run([sys.executable, pc.__file__, "--dump", path], timeout=120, env=dict(os.environ, MMS_HEAD_RT="2"))
    assert done.returncode == 0, done.returncode
    child = dict(np.load(path))
    pc.report("cuda:0", "heads_32_rows", **pc.check_dump(child, pc.dump_calls(_gpu())))


@pytest.mark.parametrize("regime", pc.GAE_REGIMES)
def test_gae_ppo(torch_cuda, regime):
    worst = {}
    for T, N in pc.GAE_SHAPES_SMALL:
        pc._merge(worst, pc.check_gae_ppo(_gpu(), T, N, regime))
    pc.report("cuda:0", "gae_ppo_%s" % regime, **worst)


@pytest.mark.parametrize("T,N", pc.GAE_SHAPES_CAP)
def test_gae_ppo_past_the_grid_cap(torch_cuda, T, N):
    """more than 2048 x 256 columns: the scan's grid-stride loop takes its second trip and the normalisation sums all 2048 partials"""
    worst = {}
    for regime in ("random", "shifted"):
        pc._merge(worst, pc.check_gae_ppo(_gpu(), T, N, regime))
    pc.report("cuda:0", "gae_ppo_T%d_N%d" % (T, N), **worst)


@pytest.mark.parametrize("T,N,A", [(1, 1, 1), (8, 33, 3), (13, 1000, 10), (5, 77, 10), (1, 52430, 10)])
def test_gae_marl(torch_cuda, T, N, A):
    pc.report("cuda:0", "gae_marl_T%d_N%d_A%d" % (T, N, A), **pc.check_gae_marl(_gpu(), T, N, A))


def test_marl_views(torch_cuda):
    pc.check_marl_views(_gpu())


def test_refusals(torch_cuda):
    assert pc.check_refusals(_gpu()) >= 40

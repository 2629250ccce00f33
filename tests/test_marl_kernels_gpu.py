"""The grouped MAPPO / HAPPO inference kernels entry by entry (tests/marl_kernels_check.py) on the MI355X: row statistics
(policy_kernels.hip: row_stats_kernel, row_stats_chan_kernel), layernorm_rows_kernel at both register widths, marl_heads_kernel at both
row counts, marl_heads_finish_kernel, and the LayerNorm-fold epilogues of linear_act_fast_kernel (six instantiations) and of the two
split layer kernels (MT = 2 / 4 x out_mode 1 / 2 each), against float64 per output and against the CPU build.  Shapes alone select the
kernels; the split layers' tiling follows the device's CU count, which the tests read to choose (M, N) and to print what they expect."""
import pytest

import marl_kernels_check as mk

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


def _cpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.lib_cpu(), -1, None, "cpu"


@pytest.mark.parametrize("chan", [True, False], ids=["chan", "plain"])
def test_row_stats(torch_cuda, chan):
    mk.check_row_stats(*_gpu(), chan)


def test_row_stats_chan_large_mean(torch_cuda):
    mk.check_chan_large_mean(*_gpu())


@pytest.mark.parametrize("K", [1, 46, 63, 64, 65, 388, 1024, 1025, 3808, 4096])
def test_layernorm(torch_cuda, K):
    mk.check_layernorm(*_gpu(), K)


@pytest.mark.parametrize("H", [1, 46, 64, 100, 512, 1024])
def test_heads(torch_cuda, H):
    """(M = 1, 7, 33 with four networks: two rows per wave; H = 1024 with A = 16 fills the 64 KB of LDS)"""
    for M in (1, 7, 33):
        mk.check_heads(*_gpu(), H, M)


def test_heads_many_groups_ragged_rows(torch_cuda):
    """32 networks x 485 rows: ceil(485 / 32) x 32 = 512 blocks, launch_marl_heads' threshold for eight rows per wave; the last block
    of every network holds 5 rows"""
    mk.check_heads(*_gpu(), 100, 485, A=[(1, 3, 8, 16)[g % 4] for g in range(32)])


def test_heads_sampling_is_keyed(torch_cuda):
    mk.check_heads_sampling_exact(*_gpu())


def test_heads_sample_moments(torch_cuda):
    mk.check_heads_moments(*_gpu())


def test_heads_contract(torch_cuda):
    mk.check_heads_contract(*_gpu())


def _fold_shape(torch, which):
    """(M, N) for 32 networks by the rule of launch_linear_split16 and the CU count, and the tiling it must select"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n1 = 128 * ((cus + 63) // 64)
    M, N, want = {"mt2_m128": (128, 128, 2), "mt2_m384": (384, 384, 2), "mt4_one_wave": (512, n1, 4), "mt4_ragged_waves": (512, n1 + 128, 4)}[which]
    MT, tiles, blocks = mk.expected_tiling(cus, 32, M, N)
    print("%s: %d CUs, M %d N %d: expecting MT = %d, %d tiles on %d persistent blocks (%s)" % (
        which, cus, M, N, MT, tiles, blocks, "one tile each" if tiles <= blocks else "%d blocks take %d tiles, the others %d" % (
            tiles % blocks or blocks, -(-tiles // blocks), tiles // blocks)))
    assert MT == want, (which, cus, MT)
    if which == "mt4_ragged_waves":
        assert tiles > cus and tiles % cus != 0, (cus, tiles)
    return M, N


@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("which", ["mt2_m128", "mt2_m384", "mt4_one_wave", "mt4_ragged_waves"])
@pytest.mark.parametrize("fmt", ["f16x2", "bf16x3"])
def test_folded_layer(torch_cuda, fmt, which, K):
    M, N = _fold_shape(torch_cuda, which)
    mk.check_folded_layer(*_gpu(), fmt, 32, M, N, K, label="%s_K%d" % (which, K))


@pytest.mark.parametrize("fmt", ["f16x2", "bf16x3"])
def test_folded_layer_more_than_sixteen_slots(torch_cuda, fmt):
    """N = 1152: 18 slots, the loop branch of chan_combine through the real path (out_mode 2 -> mms_marl_heads_finish)"""
    mk.check_folded_layer(*_gpu(), fmt, 2, 128, 1152, 64, head_dims=[5, 16])


@pytest.mark.parametrize("K", [64, 388])
@pytest.mark.parametrize("ln_in,ln_out", [(0, 1), (1, 0), (1, 1)], ids=["part_out", "stat_in", "both"])
def test_linear_fold32(torch_cuda, ln_in, ln_out, K):
    mk.check_linear_fold32(*_gpu(), ln_in, ln_out, K)


def test_kernels_against_cpu_build(torch_cuda):
    """Three shapes of each section on both builds: the statistics kernels of section 1 within section 1's bounds (not bit for bit:
    marl_kernels_check.row_stats_builds_agree says why), sections 2-4 at 1e-5 of the per-output scale."""
    import parity
    worst = {}
    for chan in (True, False):
        kw = dict(Ms=(257,), slot_counts=(8, 17, 33))
        worst["row_stats_%s" % ("chan" if chan else "plain")] = mk.row_stats_builds_agree(mk.check_row_stats(*_gpu(), chan, **kw), mk.check_row_stats(*_cpu(), chan, **kw), chan)
    for K in (46, 1025, 4096):
        worst["layernorm_K%d" % K] = mk.layernorm_builds_agree(mk.check_layernorm(*_gpu(), K, Ms=(130,)), mk.check_layernorm(*_cpu(), K, Ms=(130,)), K, (130,))
    for H, M in ((46, 33), (512, 7), (1024, 33)):
        worst["heads_H%d_M%d" % (H, M)] = mk.heads_builds_agree(mk.check_heads(*_gpu(), H, M), mk.check_heads(*_cpu(), H, M), H, M)
    for fmt, M, N, K in (("f16x2", 128, 128, 64), ("f16x2", 384, 384, 100), ("bf16x3", 128, 128, 100)):
        worst["fold_%s_M%d_K%d" % (fmt, M, K)] = mk.fold_builds_agree(mk.check_folded_layer(*_gpu(), fmt, 32, M, N, K), mk.check_folded_layer(*_cpu(), fmt, 32, M, N, K))
    print("gpu against cpu build, worst difference / bound:", worst)
    parity.record("gpu/marl_kernels_against_cpu_build", **worst)

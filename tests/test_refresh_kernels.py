"""The weight-refresh entries (mms_fold_planes16_group, mms_fold_scales16_group, mms_weight_planes16_group, mms_chain_refresh16) and the
grouped mms_split_planes_group per output (tests/refresh_kernels_check.py) on the CPU build of the C ABI.  The CPU build has one loop
where the HIP build has an aligned and an unaligned instantiation: the launch compositions that select them there check the host side
of the entries here (per-group shapes, NULL arrays and entries, shifted buffers), with the CPU build's own gates (D = K: one chain over
the row).  tests/test_refresh_kernels_gpu.py runs the same list on the HIP build.  The gates' self-checks (a float64 reference that lost
an element, or the tail of the last piece, must miss the s, c and rb gates at least twice over) run here and on the device."""
import pytest

import refresh_kernels_check as rk
from massive_marl_benchmark_amd import _lib


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


def test_fold_planes_aligned_set_three_arrangements():
    rk.check_fold_aligned_paths(*_cpu())


def test_fold_planes_unaligned_widths():
    rk.check_fold_unaligned(*_cpu())


def test_fold_planes_heads_shaped():
    rk.check_fold_heads_shaped(*_cpu())


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("which", sorted(rk.FOLD_OPTIONAL))
def test_fold_planes_optional_arguments(which, aligned):
    rk.check_fold_optional(*_cpu(), which, aligned)


def test_fold_planes_boundary_rows():
    rk.check_fold_boundary_rows(*_cpu())


@pytest.mark.parametrize("K", [100, 388])
@pytest.mark.parametrize("mutation", ["element", "tail"])
def test_fold_gates_see_a_dropped_element_or_tail(mutation, K):
    rk.check_fold_gates_see_mutations(*_cpu(), mutation, K)


def test_fold_scales():
    rk.check_fold_scales(*_cpu())


def test_zero_network_layer():
    rk.check_zero_network_layer(*_cpu())


def test_weight_planes_per_group():
    rk.check_weight_planes(*_cpu())


def test_chain_refresh():
    rk.check_chain_refresh(*_cpu())


def test_split_planes_group_three_groups():
    rk.check_split_planes_group(*_cpu())

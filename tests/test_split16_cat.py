"""mms_split_planes16_cat without a GPU: the CPU build of the entry against the CPU build's mms_split_planes16_group on the
materialised concatenation, byte for byte (tests/split16_cat_check.py), its guards and its error paths."""
import ctypes

import pytest

import split16_cat_check as sc
from massive_marl_benchmark_amd import _lib


def test_symbol_is_exported_by_both_libraries():
    assert "mms_split_planes16_cat" in _lib.SYMBOLS
    assert hasattr(_lib.lib_cpu(), "mms_split_planes16_cat")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mms_split_planes16_cat")


@pytest.mark.parametrize("rows,K0,K1", sc.CASES)
def test_cpu_build_equals_split_of_the_concatenation(rows, K0, K1):
    sc.check_case(_lib.lib_cpu(), -1, None, "cpu", rows, K0, K1)


def test_rows_zero_cpu_build():
    sc.check_rows_zero(_lib.lib_cpu(), -1, None, "cpu")


def test_abi_errors_cpu_build():
    L = _lib.lib_cpu()
    sc.error_paths(L, -1, None, "cpu")
    assert L.mms_split_planes16_cat(0, 0, 1, 0, None, 1, 0, None, None, None, None, 0, 0, None, None, None, None) != 0      # a device ordinal
    assert "device must be -1" in _lib.last_error(None, L)

"""The GRU gate backward (mms_gru_gates_grad_group, include/mms.h) entry by entry (tests/gru_grad_check.py) on the CPU build of the C
ABI.  tests/test_gru_grad_gpu.py runs the same list on the HIP build."""
import os
import subprocess

import pytest

import gru_grad_check as gc
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


def test_abi_declares_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "int mms_gru_gates_grad_group(" in hdr
    assert "#define MMS_ABI_VERSION 4" in hdr and _lib.lib_cpu().mms_abi_version() == 4            # an addition: the version stays
    assert "mms_gru_gates_grad_group" in _lib.SYMBOLS
    for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T mms_gru_gates_grad_group\n" in out, path


@pytest.mark.parametrize("H,M", gc.SHAPES)
def test_against_float64(H, M):
    gc.check_against_f64(*_cpu(), H, M, layout=gc.LAYOUTS[(H // 4 + M) % 3])


def test_against_float64_past_the_chunk_cap():
    gc.check_against_f64(*_cpu(), *gc.BIG, G=1)


def test_against_float64_32_networks():
    gc.check_against_f64(*_cpu(), 36, 7, G=32, layout="agents")


def test_no_rows():
    gc.check_empty(*_cpu())


def test_masks_and_null_operands():
    gc.check_masks(*_cpu())


def test_rows_independent_and_deterministic():
    gc.check_rows_independent(*_cpu())


def test_layouts_and_writes():
    gc.check_layouts(*_cpu())


def test_contract():
    gc.check_contract(*_cpu())

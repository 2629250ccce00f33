"""The update's output-head entries (mms_marl_heads_fwd_group, mms_marl_heads_grad_group, include/mms.h) entry by entry
(tests/marl_heads_grad_check.py) on the CPU build of the C ABI.  tests/test_marl_heads_grad_gpu.py runs the same list on the HIP build."""
import os
import subprocess

import pytest

import marl_heads_grad_check as hc
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


def test_abi_declares_and_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "#define MMS_ABI_VERSION 4" in hdr and _lib.lib_cpu().mms_abi_version() == 4            # an addition: the version stays
    for name in (hc.FWD, hc.BWD):
        assert "int %s(" % name in hdr
        assert name in _lib.SYMBOLS
        for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
            out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            assert " T %s\n" % name in out, (name, path)


@pytest.mark.parametrize("H,M,spec", hc.SHAPES)
def test_against_float64(H, M, spec):
    hc.check_against_f64(*_cpu(), H, M, spec)


def test_against_float64_32_networks():
    hc.check_against_f64(*_cpu(), *hc.WIDE)


@pytest.mark.parametrize("H,M,spec", hc.SHAPES[1:6] + (hc.WIDE,))
def test_every_group_equals_the_single_group_call(H, M, spec):
    hc.check_groups_equal_single(*_cpu(), H, M, spec)


@pytest.mark.parametrize("H", [36, 512])
def test_groups_and_rows_independent(H):
    hc.check_groups_independent(*_cpu(), H)


def test_null_outputs():
    hc.check_null_outputs(*_cpu())


def test_no_rows():
    hc.check_empty(*_cpu())


def test_contract():
    hc.check_contract(*_cpu())

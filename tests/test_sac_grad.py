"""The backward of SAC's fused head (mms_sac_heads_grad, include/mms.h) and the actor's `fused_grad=True` path (algorithms/rl/sac/
module.py) without a GPU: the CPU build of the entry against float64 per element, its bias sums, structure and error paths, and the
module on torch's "cpu" device against float64 autograd.  The checks are sac_grad_check.py's, shared with test_sac_grad_gpu.py."""
import os
import subprocess

import pytest

import sac_grad_check as gc
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cpu():
    return gc.build("cpu")


def test_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "int mms_sac_heads_grad(" in hdr and "#define MMS_ABI_VERSION 4" in hdr
    assert "measure-zero" in hdr.split("int mms_sac_heads_grad(")[0].split("int mms_sac_heads_act(")[1]      # the clamp tie is stated
    assert "mms_sac_heads_grad" in _lib.SYMBOLS
    for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc")])
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert " T mms_sac_heads_grad\n" in out, path


@pytest.mark.parametrize("N,H,A,limit,det", gc.ENTRY_SHAPES)
def test_cpu_build_against_float64(cpu, N, H, A, limit, det):
    gc.check_entry(cpu, N, H, A, limit, det)


def test_structure_cpu_build(cpu):
    gc.check_structure(cpu)


def test_abi_errors_cpu_build(cpu):
    gc.check_abi_errors(cpu)
    assert gc.ws_bytes(cpu, 1000, 24) == 0                         # the CPU build needs no workspace


def test_module_gradients_against_float64(cpu):
    gc.module_gradient_ratios(cpu)


def test_module_semantics(cpu):
    gc.check_module_semantics(cpu)


def test_fallback_is_the_torch_path():
    gc.check_fallback("cpu")


def test_policy_loss_leaves_frozen_critics_alone():
    gc.check_policy_loss("cpu")

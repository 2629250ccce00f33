"""mms_det_heads_act / mms_det_heads_grad (include/mms.h) and the `fused_grad=True` path of DDPG's / TD3's modules without a GPU: the CPU
build of both entries per case and path, their error paths, and the modules on torch's "cpu" device against float64 autograd.  The
checks are det_head_check.py's, shared with test_det_head_gpu.py."""
import os
import subprocess

import pytest

import det_head_check as dc
import sac_learner_check as sl
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cpu():
    return dc.build("cpu")


def test_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    for name in ("mms_det_heads_act", "mms_det_heads_grad"):
        assert "int %s(" % name in hdr and name in _lib.SYMBOLS
        for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
            if not os.path.exists(path):
                subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc")])
            out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
            assert " T %s\n" % name in out, (path, name)


def test_forward_cpu_build(cpu):
    ratios = dc.forward_ratios(cpu)
    dc.record_ratios("cpu", {"forward": ratios})
    sl.assert_head_rule(ratios, "forward")


def test_backward_cpu_build(cpu):
    dc.record_ratios("cpu", {"backward": dc.backward_ratios(cpu)})
    assert dc.ws_bytes(cpu, 1000, 24) == 0                          # the CPU build needs no workspace


def test_abi_errors_cpu_build(cpu):
    dc.check_abi_errors(cpu)


def test_module_gradients_against_float64(cpu):
    ratios = {H: dc.module_gradient_ratios(cpu, H) for H in (64, 128)}
    dc.record_ratios("cpu", {"module": ratios})
    sl.assert_head_rule(ratios, "pi_loss")


def test_module_semantics(cpu):
    dc.check_module_semantics(cpu)


def test_fallback_is_the_torch_path():
    dc.check_fallback("cpu")

"""mms_param_step (clip + Adam + polyak, include/mms.h) on the CPU build, FusedAdam (optim.py) on torch's "cpu" device and the opt-in
wiring of MADDPG / MAPPO.  The checks are param_step_check.py's, shared with test_param_step_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import param_step_check as pc
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu():
    return _lib.lib_cpu(), -1, None


def test_symbol_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "int mms_param_step(" in hdr and "#define MMS_PARAM_MAX_TENSORS %d" % pc.MAX_TENSORS in hdr and "#define MMS_PARAM_CHUNK %d" % pc.CHUNK in hdr
    assert "#define MMS_ABI_VERSION 4" in hdr and "NOT rewritten in place" in hdr
    from massive_marl_benchmark_amd import optim
    assert optim.MAX_TENSORS == pc.MAX_TENSORS
    for name in ("mms_param_step", "mms_param_step_partials"):
        assert name in _lib.SYMBOLS
        for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
            if not os.path.exists(path):
                subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc")])
            out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
            assert " T %s\n" % name in out, path


def test_kernel_unit_is_built_without_fast_math():
    """The parameter step's translation unit has its own rule: no KERNEL_FLAGS, -ffp-contract=off, IEEE division and square root."""
    mk = open(os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc", "Makefile")).read()
    rule = re.search(r"\.\./lib/obj/param_step_kernels\.o:.*\n\t.*\n\t(.*)\n", mk).group(1)
    assert "$(PARAM_FLAGS)" in rule and "KERNEL_FLAGS" not in rule
    flags = re.search(r"^PARAM_FLAGS \?= (.*)$", mk, re.M).group(1)
    assert "-ffp-contract=off" in flags and "filter-out -fno-hip-fp32-correctly-rounded-divide-sqrt" in flags
    assert "param_step_lane.h" in re.search(r"^\$\(CPU_OUT\):(.*)$", mk, re.M).group(1)


@pytest.mark.parametrize("hp", range(len(pc.HP)))
@pytest.mark.parametrize("tensors", range(len(pc.TENSOR_SETS)), ids=[s[0] for s in pc.TENSOR_SETS])
def test_against_float64(tensors, hp):
    pc.check_against_float64(*_cpu(), "cpu", tensors, hp)


def test_polyak_is_bit_identical_to_the_reference_statements():
    pc.check_polyak_bits(*_cpu(), "cpu")


def test_two_product_expression_matches_torch_bit_for_bit():
    """fl(fl(t polyak) + fl(c p)), c = (float)(1.0 - polyak), every operation rounded to fp32 on its own: torch's two statements."""
    g = torch.Generator().manual_seed(1)
    t, p = torch.randn(10000, generator=g), torch.randn(10000, generator=g)
    want = pc.statements(t, p).numpy()
    tn, pn = t.numpy(), p.numpy()
    got = (tn * np.float32(pc.POLYAK)).astype(np.float32) + (np.float32(1.0 - pc.POLYAK) * pn).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.float32(1.0 - pc.POLYAK) != np.float32(1.0) - np.float32(pc.POLYAK)      # why the entry takes polyak as a double


def test_norm_semantics():
    pc.check_norm_semantics(*_cpu(), "cpu")


def test_determinism_and_independence():
    pc.check_determinism(*_cpu(), "cpu")


def test_nonfinite_gradient():
    pc.check_nonfinite(*_cpu(), "cpu")


def test_error_paths():
    pc.check_error_paths(*_cpu(), "cpu", other_device=0)


def test_partials_size():
    L = _lib.lib_cpu()
    size = lambda ns: L.mms_param_step_partials(len(ns), (ctypes.c_int64 * max(1, len(ns)))(*ns))
    assert size([]) == 1 and size([0]) == 1 and size([1]) == 1 and size([4096]) == 1 and size([4097, 1, 0]) == 3
    assert size([-1]) == 0 and size([1] * (pc.MAX_TENSORS + 1)) == 0


def test_fused_adam():
    pc.check_fused_adam(torch.device("cpu"))


def test_fused_adam_without_the_cpu_library_runs_the_torch_ops(monkeypatch):
    """CPU tensors without the CPU library selected: the wrapper's documented torch-ops path, not a call of the entry."""
    from massive_marl_benchmark_amd import optim
    monkeypatch.setattr(_lib, "LIB_CPU_PATH", os.path.join(ROOT, "no", "such", "libmms_cpu.so"))
    monkeypatch.setattr(_lib, "for_device", lambda dev: pytest.fail("the entry must not be reached"))
    w, twin = torch.nn.Parameter(torch.full((70,), 0.5)), torch.nn.Parameter(torch.full((70,), 0.5))
    w.grad, twin.grad = torch.full((70,), 3.0), torch.full((70,), 3.0)
    got = optim.FusedAdam([w], lr=1e-2).clip_and_step(1.0)
    want = torch.nn.utils.clip_grad_norm_([twin], 1.0)
    torch.optim.Adam([twin], lr=1e-2).step()
    assert abs(float(got) - float(want)) <= 1e-6 * float(want) and torch.allclose(w, twin, rtol=1e-6, atol=0) and torch.equal(w.grad, torch.full((70,), 3.0))


def test_maddpg_wiring():
    pc.check_maddpg_wiring("cpu")


@pytest.mark.parametrize("algo", ["MAPPO", "HAPPO"])
def test_mappo_wiring(algo):
    pc.check_mappo_wiring("cpu", algo)

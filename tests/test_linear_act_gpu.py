"""The exact-fp32 layer kernels (csrc/policy_kernels.hip: linear_act_fast_kernel<TAIL, ELU_ONLY, MI>, linear_act_kernel<2>, <1> and
<1, BLOCKED>) case by case (tests/linear_act_check.py) on the MI355X, through mms_linear_group_act and mms_linear2_act: per element
against float64 with guarded operands and destinations, and against the CPU build.  The shapes alone select the kernels
(lk.expected_kernel restates launch_linear_act), so the launcher's overrides must not be in the environment."""
import os

import pytest

import linear_act_check as lk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


@pytest.fixture(autouse=True)
def no_dispatch_override():
    found = [v for v in lk.ENV_OVERRIDES if v in os.environ]
    if found:
        pytest.fail("%s set in the environment: launch_linear_act would not select the kernels the case table names; unset to run these tests" % ", ".join(found))


def _gpu():
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _lib.for_device("cuda:0")
    return L, dev, stream, "cuda"


def _cpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.lib_cpu(), -1, None, "cpu"


def _id(case):
    return "-".join(str(v) if not isinstance(v, tuple) else "act" + "_".join(map(str, v)) for v in case)


def test_case_table_reaches_every_kernel(torch_cuda):
    """All eleven kernels and both tile maps at either tile height, by the launcher's rule, with its overrides absent (the fixture)"""
    names, maps, one, two = lk.coverage()
    print("mms_linear_group_act cases reach:", sorted(names))
    print("tile maps reached: MI=1", sorted(maps[1]), "MI=2", sorted(maps[2]))
    print("mms_linear2_act cases reach: one problem", sorted(one), "two problems", sorted(two))
    assert names == lk.ALL_KERNELS and len(names) == 11
    assert maps[1] == {"xcd", "linear"} and maps[2] == {"xcd", "linear"}
    assert one == two == lk.ALL_KERNELS - {"generic<1,blocked>"}


@pytest.mark.parametrize("case", lk.CASES, ids=_id)
def test_case(torch_cuda, case):
    lk.check_case(*_gpu(), *case)


@pytest.mark.parametrize("case", lk.LINEAR2_CASES, ids=_id)
def test_linear2_entry(torch_cuda, case):
    lk.check_linear2(*_gpu(), *case)


def test_linear2_entry_has_no_blocked_form(torch_cuda):
    lk.check_linear2_has_no_blocked(*_gpu())


def test_blocked_flag_ignored_on_fast_path(torch_cuda):
    lk.check_blocked_flag_ignored_on_fast_path(*_gpu())


def test_no_rows(torch_cuda):
    lk.check_empty(*_gpu())


def test_tanh(torch_cuda):
    lk.check_tanh(*_gpu())


@pytest.mark.parametrize("case", lk.BUILDS_AGREE_CASES, ids=_id)
def test_against_cpu_build(torch_cuda, case):
    """One fast MI = 1, one fast MI = 2 and one generic case on both builds: the difference is at most the sum of the two per-element bounds"""
    import parity
    worst = lk.builds_agree(lk.check_case(*_gpu(), *case), lk.check_case(*_cpu(), *case))
    print("gpu against cpu build, worst difference / (sum of the bounds): %.3g" % worst)
    parity.record("gpu/linear_act_against_cpu_build_" + _id(case), worst_over_bound_sum=worst)

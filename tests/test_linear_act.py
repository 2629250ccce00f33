"""The exact-fp32 layer entries (mms_linear2_act, mms_linear_group_act; include/mms.h) case by case (tests/linear_act_check.py) on the
CPU build of the C ABI: a correct implementation stays inside every bound of the list.  tests/test_linear_act_gpu.py runs the same
list on the HIP build, where the shapes select the eleven kernels of csrc/policy_kernels.hip."""
import pytest

import linear_act_check as lk
from massive_marl_benchmark_amd import _lib


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


def _id(case):
    return "-".join(str(v) if not isinstance(v, tuple) else "act" + "_".join(map(str, v)) for v in case)


def test_case_table_reaches_every_kernel():
    """By the launcher's rule (lk.expected_kernel) the table selects all eleven unfolded kernels, both branches of the fast kernel's
    tile map at either tile height, and every kernel mms_linear2_act can reach with one and with two problems."""
    names, maps, one, two = lk.coverage()
    print("mms_linear_group_act cases reach:", sorted(names))
    print("tile maps reached: MI=1", sorted(maps[1]), "MI=2", sorted(maps[2]))
    print("mms_linear2_act cases reach: one problem", sorted(one), "two problems", sorted(two))
    assert names == lk.ALL_KERNELS and len(names) == 11
    assert maps[1] == {"xcd", "linear"} and maps[2] == {"xcd", "linear"}
    assert one == two == lk.ALL_KERNELS - {"generic<1,blocked>"}
    assert {lk.expected_kernel(*c[:4], a) for c in lk.CASES for a in c[4] if (*c[:4], a) in lk.TWICE} == lk.ALL_KERNELS
    # the rule itself at its edges: 255 / 256 blocks, M = 64 / 65, K = 4 / 8, the blocked flag where a fast kernel runs
    assert lk.expected_kernel(1, 65, 128, 8, 1) == "generic<1>" and lk.expected_kernel(1, 64, 128, 8, 1) == "generic<2>"
    assert lk.expected_kernel(1, 128, 128, 8, 1) == "fast<tail,elu,MI=1>" and lk.expected_kernel(1, 128, 128, 4, 1) == "generic<1>"
    assert lk.expected_kernel(17, 384, 640, 32, 2) == "fast<full,act,MI=1>" and lk.expected_kernel(32, 256, 512, 32, 2) == "fast<full,act,MI=2>"
    assert lk.expected_kernel(32, 320, 512, 32, 1) == "generic<2>" and lk.expected_kernel(2, 192, 256, 100, 17) == "fast<tail,elu,MI=1>"
    assert lk.expected_kernel(3, 130, 100, 68, 17) == "generic<1,blocked>"


@pytest.mark.parametrize("case", lk.CASES, ids=_id)
def test_case(case):
    lk.check_case(*_cpu(), *case)


@pytest.mark.parametrize("case", lk.LINEAR2_CASES, ids=_id)
def test_linear2_entry(case):
    lk.check_linear2(*_cpu(), *case)


def test_linear2_entry_has_no_blocked_form():
    lk.check_linear2_has_no_blocked(*_cpu())


def test_blocked_flag_ignored_on_fast_path():
    lk.check_blocked_flag_ignored_on_fast_path(*_cpu())


def test_no_rows():
    lk.check_empty(*_cpu())


def test_tanh():
    lk.check_tanh(*_cpu())

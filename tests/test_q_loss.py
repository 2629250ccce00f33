"""The critics' loss heads with a gradient (mms_q_heads_loss, include/mms.h) without a GPU: the CPU build of the entry against
mms_q_heads_backup's q and against float64 from its own q_out, ties, row independence, NULL outputs and the contract.  The checks
are q_loss_check.py's, shared with test_q_loss_gpu.py."""
import os
import subprocess

import pytest
import torch

import q_loss_check as lc
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cpu():
    return _lib.lib_cpu(), -1, None, torch.device("cpu")


def test_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "int mms_q_heads_loss(" in hdr and "#define MMS_ABI_VERSION 4" in hdr
    doc = hdr.split("int mms_q_heads_loss(")[0].split("int mms_q_heads_backup(")[1]
    assert "sac.py:367-389" in doc and "sac.py:392-403" in doc                 # the call sites it replaces
    assert "mms_q_heads_loss" in _lib.SYMBOLS
    for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "massive_marl_benchmark_amd", "csrc")])
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert " T mms_q_heads_loss\n" in out, path


@pytest.mark.parametrize("M,H,G", lc.SHAPES + [lc.MULTI])
def test_cpu_build_against_float64(cpu, M, H, G):
    L, device, stream, dev = cpu
    lc.check_shape(L, device, stream, dev, M, H, G, "cpu")


def test_shape_table_reaches_every_kernel():
    """launch_main's five NJ for either G, each with all chunks live and (NJ >= 4) with chunks guarded out."""
    assert lc.coverage() == lc.REACHABLE and len(lc.REACHABLE) == 16 and len({k[:2] for k in lc.REACHABLE}) == 10
    assert lc.coverage(lc.SHAPES) == {(1, 1, "full"), (2, 1, "full"), (2, 4, "guarded"), (2, 16, "full"), (2, 2, "full")}
    assert [lc.expected_kernel(1, H)[1:] for H in (64, 128, 192, 256, 320, 512, 576, 1024)] == [(1, 1), (2, 2), (4, 3), (4, 4), (8, 5), (8, 8), (16, 9), (16, 16)]


@pytest.mark.parametrize("M,H,G", lc.NEW_SHAPES)
def test_kernel_table(cpu, M, H, G):
    L, device, stream, dev = cpu
    lc.check_shape(L, device, stream, dev, M, H, G, "cpu")


@pytest.mark.parametrize("mutation", ["chunk", "last"])
def test_gates_see_a_dropped_chunk_or_element(cpu, mutation):
    """The float64 statement without the last 64 k of h and w, or without the last k, at nj = 16: the gates of dh and dw are missed at
    least ten times over, for either network."""
    L, device, stream, dev = cpu
    worst = lc.check_shape(L, device, stream, dev, 33, 1024, 2, "cpu", mutation=mutation)
    assert sorted(worst) == ["dh0", "dh1", "dw0", "dw1"] and min(worst.values()) >= 10, worst


def test_null_outputs_one_network(cpu):
    lc.check_null_outputs(*cpu, M=17, H=320, G=1)


def test_ties_and_strict_rows(cpu):
    lc.check_ties_and_strict(*cpu)


def test_rows_do_not_depend_on_their_place(cpu):
    lc.check_row_independence(*cpu)


def test_null_outputs(cpu):
    lc.check_null_outputs(*cpu)


def test_contract(cpu):
    L, device, stream, dev = cpu
    lc.check_contract(L, device, stream, 0)
    assert lc.workspace(L, device, stream, 1000, 256, 2, dev)[2].value == 0       # the CPU build needs no workspace

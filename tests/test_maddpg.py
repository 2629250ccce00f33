"""MADDPG on the CPU build (lib/libmms_cpu.so): the two entries mms_det_heads_act_group and mms_q_heads_backup_group per case, and
the modules of algorithms/marl/maddpg against the reference's recorded update (tests/golden/maddpg_update.npz).  The checks are
maddpg_check.py's, shared with test_maddpg_gpu.py."""
import pytest
import torch

import maddpg_check as mc
from massive_marl_benchmark_amd import _lib


def _cpu():
    return _lib.lib_cpu(), -1, None


@pytest.mark.parametrize("case", mc.HEAD_CASES, ids=lambda c: "M%d-H%d-A%d-G%d-a%d" % c)
def test_head_against_float64(case):
    mc.check_head_case(*_cpu(), case, "cpu")


def test_head_exactness():
    mc.check_head_exactness(*_cpu(), "cpu")


@pytest.mark.parametrize("case", [(7, 64, 3, 2, 0), (17, 512, 8, 10, 0), (333, 512, 16, 3, 2), (1000, 512, 8, 10, 5)], ids=lambda c: "M%d-H%d-A%d-G%d-a%d" % c)
def test_head_noise(case):
    mc.check_head_noise(*_cpu(), case, "cpu")


def test_head_noise_statistics():
    mc.check_head_statistics(*_cpu(), "cpu")


def test_head_error_paths():
    mc.check_head_error_paths(*_cpu(), other_device=0)


@pytest.mark.parametrize("case", mc.Q_CASES, ids=lambda c: "M%d-H%d-G%d" % c)
def test_q_group_equals_ungrouped(case):
    mc.check_q_case(*_cpu(), case, "cpu")


def test_q_group_error_paths():
    mc.check_q_error_paths(*_cpu(), other_device=0)


# ---- every det_heads_act_kernel<NCT, WAVES> and every part of the grouped Q kernel's k-loop (maddpg_check's docstring) ----

def test_head_table_reaches_every_kernel():
    """The launcher's `switch` (NCT 1..8) times its four WAVES: an instantiation added there without a case fails here."""
    assert len(mc.REACHABLE) == 32 and mc.head_coverage() == mc.REACHABLE
    assert mc.head_coverage(mc.NEW_HEAD_CASES) == mc.REACHABLE and len(mc.head_coverage(mc.HEAD_CASES)) == 5
    assert mc.expected_kernel(512, 128) == (8, 8) and mc.expected_kernel(192, 1) == (1, 1) and mc.expected_kernel(384, 17) == (2, 2)
    assert mc.expected_kernel(768, 113) == (8, 4)
    for t in range(1, 9):            # each NCT with a full last column tile and with one live column in it
        assert {A for _, _, A, _, _ in mc.NEW_HEAD_CASES if (A + 15) // 16 == t} >= {16 * t, 16 * (t - 1) + 1}
    assert all(mc.noise_case(c)[1:3] == c[1:3] and sum(mc.noise_case(c)[3:]) * c[2] <= 128 for c in mc.NEW_HEAD_CASES)


def test_q_group_table_reaches_every_path():
    assert mc.q_coverage() == mc.Q_REACHABLE and mc.q_coverage(mc.NEW_Q_CASES) == mc.Q_REACHABLE
    assert mc.q_coverage(mc.Q_CASES) == {("grouped", "remainder"), ("grouped", "unrolled")}


@pytest.mark.parametrize("case", mc.NEW_HEAD_CASES, ids=lambda c: "M%d-H%d-A%d-G%d-a%d" % c)
def test_head_kernel_table(case):
    mc.check_head_case(*_cpu(), case, "cpu")
    mc.check_head_noise(*_cpu(), mc.noise_case(case), "cpu")


@pytest.mark.parametrize("mutation", ["tile", "last"])
def test_head_gate_sees_a_dropped_tile_or_column(mutation):
    """The float64 side without the last column tile's weights, or without the last column's, at NCT = 8 with one live column in the
    last tile: the gate is missed at least ten times over."""
    assert mc.check_head_case(*_cpu(), (33, 768, 113, 3, 0), "cpu", mutation=mutation) >= 10
    assert mc.check_head_case(*_cpu(), (1, 512, 128, 3, 2), "cpu", mutation=mutation) >= 10


@pytest.mark.parametrize("case", mc.NEW_Q_CASES, ids=lambda c: "M%d-H%d-G%d" % c)
def test_q_group_path_table(case):
    mc.check_q_case(*_cpu(), case, "cpu")


# ---- the modules against the reference's recorded update ----

def test_storage_against_reference_ring():
    mc.check_storage("cpu")


def test_losses_at_initial_parameters(monkeypatch):
    mc.check_losses("cpu", _lib.lib_cpu(), monkeypatch)


def test_ddpg_update_and_ordering(monkeypatch):
    mc.check_update("cpu", _lib.lib_cpu(), monkeypatch)


def test_train_dicts():
    mc.check_train("cpu")


def test_use_target_critic(monkeypatch):
    mc.check_target_critic("cpu", _lib.lib_cpu(), monkeypatch)


def test_act_all_33_agents_padded_rows(monkeypatch):
    mc.check_act_all("cpu", _lib.lib_cpu(), monkeypatch)


def test_runner_ten_ant(monkeypatch, tmp_path):
    mc.check_runner("cpu", _lib.lib_cpu(), monkeypatch, tmp_path)


def test_runner_imports_without_tensorboard():
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch.utils.tensorboard'] = None\n"
            "from massive_marl_benchmark_amd.algorithms.marl.maddpg import runner\n"
            "w = runner.SummaryWriter('x'); w.add_scalars('a', {'a': 1.0}, 0); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=mc.os.path.dirname(mc.os.path.dirname(mc.os.path.abspath(__file__))))
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr

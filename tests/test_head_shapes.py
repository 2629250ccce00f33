"""The fused policy head at every critic width VH / head width H of tests/head_shapes_check.py on the CPU build of the C ABI: the host
logic of mms_bind_policy_head and mms_step, the tiled-copy path of csrc/cpu/mms_cpu.cpp, and the proof of the check itself: every
mutation of a truth must miss its gate by 100 x the bound.  tests/test_head_shapes_gpu.py runs the same cases on the HIP build."""
import pytest

import head_shapes_check as hs
from massive_marl_benchmark_amd import _lib

_PAIRS = {}


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    yield
    for pair in _PAIRS.values():
        pair.close()
    _PAIRS.clear()


def _run(name, monkeypatch, mutation=None):
    return hs.run_case(hs.pair_for(_PAIRS, _cpu(), hs.CASES[name]["N"], monkeypatch), name, monkeypatch, mutation=mutation)


@pytest.mark.parametrize("name", list(hs.CASES))
def test_fused_head(monkeypatch, name):
    _run(name, monkeypatch)


def test_weight_tiles_layout():
    """the test's own tiled copy against the element formula of include/mms.h, outputs >= A zero"""
    import numpy as np
    w = np.arange(19 * 8, dtype=np.float32).reshape(19, 8) + 1
    t = hs.weight_tiles(w)
    assert t.size == 2 * 2 * 16 * 4
    for j in range(32):
        for k in range(8):
            assert t[(((j // 16) * 2 + k // 4) * 16 + j % 16) * 4 + k % 4] == (w[j, k] if j < 19 else 0.0)


# ---- the check proves itself: a corrupted truth must miss its gate by 100 x the bound, on the fused step's outputs ----------------------
def test_mutation_actor_product_drops_four_k(monkeypatch):
    assert _run("N48_H512_VH512_tiles", monkeypatch, mutation="drop_k")["mu"] >= 100
    assert _run("N16_H1024_VH260_rows", monkeypatch, mutation="drop_k")["mu"] >= 100


def test_mutation_value_head_reads_value(monkeypatch):
    assert _run("N48_H512_VH1284_rows", monkeypatch, mutation="value_from_value")["value"] >= 100


def test_mutation_counter_off_by_one(monkeypatch):
    assert _run("N48_H1024_VH1024_tiles", monkeypatch, mutation="counter")["draw"] >= 100


@pytest.mark.parametrize("VH", [260, 772])
def test_mutation_value_drops_the_last_four(monkeypatch, VH):
    """the four floats that are exactly lane 0's second trip of the staged loop"""
    assert _run("N48_H512_VH%d_tiles" % VH, monkeypatch, mutation="value_drop_tail")["value"] >= 100

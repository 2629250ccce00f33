"""The staged schedule of the fused policy head (csrc/head_block.h: ppo_head_block with SWAVES > 0 and ppo_head_stage_values, the
prologue of the <768, 16> TenAnt step kernel) on the MI355X at the critic widths and head widths of tests/head_shapes_check.py: VH at
every edge of the staging waves' two-trips-per-pass loop, H = 512 and 1024, the tiled and the row-major weight read, NULL destinations.
One step per case on engines of 16 or 48 envs; truth is float64 per output element, and the stand-alone heads kernel and a second
engine stepped by it are compared bit for bit.  tests/test_head_shapes.py runs the same cases on the CPU build, with the mutations."""
import pytest

import head_shapes_check as hs

pytestmark = pytest.mark.gpu

_PAIRS = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    yield torch
    for pair in _PAIRS.values():
        pair.close()
    _PAIRS.clear()


def _gpu():
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _lib.for_device("cuda:0")
    return L, dev, stream, "cuda"


def _run(name, monkeypatch, mutation=None):
    return hs.run_case(hs.pair_for(_PAIRS, _gpu(), hs.CASES[name]["N"], monkeypatch), name, monkeypatch, mutation=mutation)


@pytest.mark.parametrize("name", list(hs.CASES))
def test_fused_head(torch_cuda, monkeypatch, name):
    _run(name, monkeypatch)


@pytest.mark.parametrize("VH", [260, 772])
def test_mutation_value_drops_the_last_four(torch_cuda, monkeypatch, VH):
    """the check can fail on the device's outputs: a truth without the four floats of lane 0's second trip misses the value gate by 100 x"""
    assert _run("N48_H512_VH%d_rows" % VH, monkeypatch, mutation="value_drop_tail")["value"] >= 100

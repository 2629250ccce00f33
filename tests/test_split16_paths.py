"""tests/split16_paths_check.py on the CPU build of the C ABI: the launcher's rule restated (expected_path) against hand-worked values, the
path list's coverage of all 16 plain linear_split16_kernel instantiations and every path row on 256 and on 304 CUs, the float64 truth,
the decoding and the slicing helpers at small cases before they meet the GPU (tests/test_split16_paths_gpu.py), and the proof of the
harness: every mutation misses its gate by 100 x."""
import pytest

import split16_paths_check as sp
from massive_marl_benchmark_amd import _lib


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


@pytest.mark.parametrize("cus,forced,shape,want", [
    # 32 networks of 512 rows: 64 tiles of 256 rows per 128 columns
    (256, 0, (32, 512, 640, 96, 1, 0), (4, True, False, 320, 256, True)),
    (256, 2, (32, 512, 640, 96, 1, 0), (2, True, False, 640, 256, True)),
    (256, 4, (32, 512, 640, 96, 1, 0), (4, True, False, 320, 256, True)),
    (304, 0, (32, 512, 640, 96, 1, 0), (4, True, False, 320, 304, True)),
    (256, 0, (31, 512, 640, 64, 2, 1), (4, False, False, 310, 256, False)),      # 310 tiles: not a multiple of 8
    (256, 0, (32, 512, 512, 64, 1, 0), (4, True, True, 256, 256, True)),         # exactly one tile of 256 rows per CU: the tail
    (304, 0, (32, 512, 512, 64, 1, 0), (2, True, False, 512, 304, True)),        # 256 < 304: 128-row tiles, persistent
    (304, 4, (32, 512, 512, 64, 1, 0), (4, True, True, 256, 256, True)),
    (256, 0, (32, 384, 384, 32, 0, 0), (2, False, False, 288, 256, True)),       # M = 384 has no 256-row tiling
    (256, 4, (32, 384, 384, 32, 0, 0), (2, False, False, 288, 256, True)),       # ... forced or not
    (256, 0, (31, 384, 384, 160, 3, 1), (2, False, False, 279, 256, False)),
    (256, 0, (3, 256, 128, 32, 1, 0), (2, True, False, 6, 6, False)),            # one k-slice: no tail
    (256, 0, (3, 256, 128, 64, 1, 0), (2, True, True, 6, 6, False)),
    (256, 4, (3, 256, 128, 64, 0, 1), (4, False, True, 3, 3, False)),
    (304, 2, (32, 128, 128, 100, 3, 1), (2, False, True, 32, 32, True)),
])
def test_expected_path_hand_worked(cus, forced, shape, want):
    assert sp.expected_path(cus, forced, *shape) == want


def test_expected_path_three_planes():
    """linear_split_kernel has one instantiation per (MT, OUT): no ELU, no TAIL"""
    assert sp.expected_path(256, 0, 32, 512, 640, 64, 1, 0, "bf16x3") == (4, False, False, 320, 256, True)
    assert sp.expected_path(256, 0, 3, 256, 128, 64, 1, 1, "bf16x3") == (2, False, False, 6, 6, False)


def test_path_rows():
    assert sp.path_rows((4, True, False, 320, 256, True), 32) == {"several_ragged", "several_groups"}
    assert sp.path_rows((4, True, False, 512, 256, True), 32) == {"several_even", "several_groups"}
    assert sp.path_rows((4, True, False, 310, 256, False), 2) == {"several_ragged_noxcd"}
    assert sp.path_rows((2, True, False, 6, 6, False), 3) == {"one_plain"}
    assert sp.path_rows((2, True, True, 6, 6, False), 3) == {"one_tail"}


def test_shapes_on_256_cus():
    assert [c[:4] for c in sp.cases(256, 0)] == [("one", 3, 256, 128), ("mt4_ragged", 32, 512, 640), ("mt4_even", 32, 512, 1024), ("mt4_noxcd", 31, 512, 640),
                                                 ("mt2_ragged", 32, 384, 384), ("mt2_even", 32, 128, 2048), ("mt2_noxcd", 31, 384, 384)]
    assert max(G * M * N for _, G, M, N, _ in sp.cases(256, 0)) <= 32 * 512 * 1024


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("fmt", ["f16x2", "bf16x3"])
def test_list_covers_every_instantiation_and_row(cus, fmt):
    reports = [{"paths": sp.planned_paths(cus, forced)} for forced in (0, 2, 4)]
    seen, missing = sp.coverage(reports, fmt)
    assert missing == set(), sorted(missing)
    if fmt == "f16x2":
        assert len({c[:4] for c in seen}) == 16 and len(sp.required(fmt)) == 8 * 5 + 8
        # the persistent loop's first wait differs for KC = 1, 2 and > 2: every several-tiles shape runs at all of them
        assert {(k + 31) // 32 for k in sp.KS} == {1, 2, 3, 4, 5} and 100 in sp.KS
    else:
        assert len({c[:4] for c in seen}) == 4


def test_two_plane_layer_against_float64_and_slices():
    """sections 2 and 3 of the check list on the CPU build: every activation and output mode, the slices compared unconditionally"""
    figs = sp.run_case(_cpu(), 256, 0, "f16x2", "cpu", 3, 256, 256, 100, ratios=False, slices="always")
    assert len(figs) == 8 and all(f["slice_bytes_differ"] == 0 and f["elem"] < 1.0 for f in figs.values())
    figs = sp.run_case(_cpu(), 256, 0, "f16x2", "cpu", 1, 128, 384, 32, ratios=False, slices="always")
    assert len(figs) == 8 and all(f["slice_bytes_differ"] == 0 for f in figs.values())


def test_three_plane_layer_against_float64_and_slices():
    figs = sp.run_case(_cpu(), 256, 0, "bf16x3", "cpu", 2, 128, 256, 64, ratios=False, slices="always")
    assert len(figs) == 8 and all(f["slice_bytes_differ"] == 0 and f["elem"] < 1.0 for f in figs.values())


def test_failures_are_reported_not_swallowed():
    """with a report given, a miss lands in it (the GPU children read nothing else)"""
    rep = sp.new_report(256, 0)
    sp.run_case(_cpu(), 256, 0, "f16x2", "cpu", 2, 256, 128, 64, acts=(2,), ratios=False, mutation="drop_k", report=rep)
    assert len(rep["f64"]) == 4 and "per-element bound missed" in rep["f64"][0]      # (the yardstick misses a corrupted truth too)
    rep = sp.new_report(256, 0)
    sp.run_case(_cpu(), 256, 0, "f16x2", "cpu", 2, 256, 128, 64, acts=(2,), ratios=False, mutation="swap_tiles", report=rep)
    assert len(rep["bits"]) == 2 and "bytes differ from the full launch, first at network 0 row " in rep["bits"][0]


def test_repeat_check_runs():
    rep = dict(sp.new_report(256, 0))
    sp.check_repeat(_cpu(), 256, 0, "f16x2", "cpu", 2, 128, 128, 64, rep, launches=2)
    assert rep["repeat"] == [] and len(rep["repeated"]) == 4


# ---- the harness proves itself: a corrupted truth (or compared copy) must miss its gate by 100 x ------------------------------------------
def _mutated(mutation, K, act):
    figs = sp.run_case(_cpu(), 256, 0, "f16x2", "cpu", 2, 256, 128, K, acts=(act,), ratios=False, mutation=mutation)
    assert len(figs) == 2                                               # fp32 out and planes out
    return figs.values()


def test_mutation_one_k_slice_dropped_from_one_tile():
    assert all(f["elem"] >= 100 and f["yardstick"] >= 100 for f in _mutated("drop_k", 96, 1))


def test_mutation_relu_taken_for_identity():
    assert all(f["elem"] >= 100 for f in _mutated("relu_as_identity", 64, 2))


def test_mutation_lo_cross_terms_dropped():
    assert all(f["elem"] >= 100 and f["yardstick"] >= 100 for f in _mutated("hi_only", 32, 0))


def test_mutation_two_tiles_swapped():
    for f in _mutated("swap_tiles", 64, 1):
        assert f["elem"] >= 100 and f["yardstick"] < 1.0 and f["slice_bytes_differ"] > 0

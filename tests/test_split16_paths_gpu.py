"""tests/split16_paths_check.py on the MI355X: every plain instantiation of linear_split16_kernel (MT 2 / 4 x OUT 0 / 1 x ELU x TAIL) and of
linear_split_kernel (MT x OUT) on every pipeline path -- one tile per block (plain sequence, tail) and several (two each, ragged, ragged
on a tile count that is no multiple of 8, more than two networks), at KC = 1, 2, 3, 5 and a ragged last chunk, with ELU, ReLU, tanh and
no activation -- against float64 per element, against the same layer as launches of one 128-column slice (at most one tile per block)
bit for bit, and launch after launch.

The tile height is chosen by split_tiles_256, which reads MMS_SPLIT_MT once per process: the check list runs in three fresh child
processes (this file as a script; MMS_SPLIT_MT unset, = 2 and = 4, started together), each reports as JSON, the tests read the reports."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SETTINGS = (0, 2, 4)                                                    # MMS_SPLIT_MT; 0: unset


def _child(path):
    for d in (ROOT, HERE):
        if d not in sys.path:
            sys.path.insert(0, d)
    import torch
    import split16_paths_check as sp
    from massive_marl_benchmark_amd import _lib
    L, di, stream = _lib.for_device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    report = sp.new_report(cus, int(os.environ.get("MMS_SPLIT_MT", "0")))
    sp.run_list((L, di, stream, "cuda"), cus, report["forced_mt"], report)
    with open(path, "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    out = tmp_path_factory.mktemp("split16_paths")
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    procs = {}
    for mt in SETTINGS:                                                 # fresh processes (never a replaced image), all three at once
        path = str(out / ("mt%d.json" % mt))
        env = {k: v for k, v in os.environ.items() if k != "MMS_SPLIT_MT"}
        if mt:
            env["MMS_SPLIT_MT"] = str(mt)
        procs[mt] = (path, subprocess.Popen(py + [os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    res = {}
    for mt, (path, proc) in procs.items():
        try:
            log = proc.communicate(timeout=300)[0].decode()
        except subprocess.TimeoutExpired:
            proc.kill()
            log = "timed out\n" + proc.communicate()[0].decode()
        assert proc.returncode == 0, "child with MMS_SPLIT_MT=%d: exit %s\n%s" % (mt, proc.returncode, log[-3000:])
        with open(path) as f:
            res[mt] = json.load(f)
        assert res[mt]["forced_mt"] == mt
    return res


@pytest.mark.parametrize("fmt", ["f16x2", "bf16x3"])
def test_path_list_is_covered(reports, fmt):
    """Every instantiation and every row of the path list was launched by at least one of the three processes; the table is printed."""
    import split16_paths_check as sp
    seen, missing = sp.coverage(reports.values(), fmt)
    count = {}
    for mt, r in reports.items():
        for label, f, MT, out, elu, tail, tiles, blocks, xcd, rows in r["paths"]:
            if f == fmt:
                for row in rows:
                    count[(MT, out, bool(elu), bool(tail), row)] = count.get((MT, out, bool(elu), bool(tail), row), 0) + 1
    print("%s on %d CUs: launches per <MT, OUT, ELU, TAIL> and path row" % (fmt, reports[0]["cus"]))
    for key in sorted(count):
        print("  <%d, %d, 0, %s, %s> %-22s %4d" % (key[0], key[1], str(key[2]).lower(), str(key[3]).lower(), key[4], count[key]))
    assert missing == set(), sorted(missing)
    assert len({k[:4] for k in seen}) == (16 if fmt == "f16x2" else 4)
    assert len({r["cus"] for r in reports.values()}) == 1


@pytest.mark.parametrize("mt", SETTINGS)
def test_paths_against_float64(reports, mt):
    """Per-element bound, yardstick, rms / worst-ratio and mean rules of test_split16_layers_error / test_split_layers_error
    (split16_paths_check.run_case); the worst figures per format and K are recorded."""
    import parity
    figs = reports[mt]["figures"]
    worst = {}
    for label, f in figs.items():
        key = "%s_K%d" % (f["fmt"], f["K"])
        w = worst.setdefault(key, {"elem": 0.0, "yardstick": 0.0, "rms_ratio": 0.0, "max_ratio": 0.0, "mean_over_rms": 0.0, "cases": 0})
        for k in ("elem", "yardstick", "rms_ratio", "max_ratio"):
            w[k] = max(w[k], f[k])
        w["mean_over_rms"] = max(w["mean_over_rms"], abs(f["mean_over_rms"]))
        w["cases"] += 1
    for key in sorted(worst):
        print("MMS_SPLIT_MT=%d %s: %s" % (mt, key, worst[key]))
    parity.record("gpu/split16_paths/mt%d" % mt, **worst)
    assert len(figs) == 7 * 5 * 4 * 2 + 3 * 2 * 2 * 2
    assert reports[mt]["f64"] == []


@pytest.mark.parametrize("mt", SETTINGS)
def test_paths_agree_bit_for_bit(reports, mt):
    """A launch of several tiles per block stores the bits of the same layer run as 128-column slices of at most one tile per block:
    the persistent loop (first and later tiles), the tail and the plain sequence are the same arithmetic (_compare_slices)."""
    sliced = [f for f in reports[mt]["figures"].values() if "slice_bytes_differ" in f]
    assert len(sliced) >= 6 * 5 * 4 * 2
    assert reports[mt]["bits"] == []


@pytest.mark.parametrize("mt", SETTINGS)
def test_paths_repeatable(reports, mt):
    """20 launches reproduce the first bit for bit, one case per several-tiles path x OUT x {ELU, ReLU} (check_repeat)."""
    import split16_paths_check as sp
    assert reports[mt]["repeat"] == []
    done = {(f, MT, out, bool(elu), row) for f, MT, out, elu, rows in reports[mt]["repeated"] for row in rows}
    heights = (2,) if mt == 2 else (2, 4)
    assert {("f16x2", MT, out, elu, row) for MT in heights for out in sp.OUTS for elu in (True, False) for row in sp.SEVERAL} <= done


def test_processes_agree(reports):
    """128-row and 256-row tiles give every accumulator its products in the same order: equal cases (same seed in every child), equal
    bits, whatever MMS_SPLIT_MT selected."""
    a = reports[0]["digest"]
    assert len(a) == 7 * 5 * 4 * 2 + 3 * 2 * 2 * 2
    for mt in (2, 4):
        b = reports[mt]["digest"]
        assert a.keys() == b.keys()
        assert [k for k in a if a[k] != b[k]] == []


if __name__ == "__main__":
    _child(sys.argv[1])

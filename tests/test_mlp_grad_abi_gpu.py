"""mms_mlp_grad / mms_mlp_grad_rop of the HIP build (csrc/trpo_kernels.hip) through the C ABI, per output tensor, with the harness and the
gates of mlp_grad_check.py (proved on the CPU build by test_mlp_grad_abi.py).  Truth (float64) and yardstick (torch fp32) are computed
on the device.  The cases are the smallest shapes that reach each edge:

  min      12, 40, 5 at M = 1            L = 2 (l == L directly above l == 1, one product per weight gradient in the R-op), one real
                                         row in a 128-row pad
  ones     1, 1, 1 at M = 33             every width 1
  ragged   33, 65, 31, 7 at M = 129      widths across the 32-k chunk and the 64-column block of the transposing split; M one past a
                                         128 boundary
  wide     36, 130, 257, 20, 6 at 300    widths just past 128 and 256; 12 row chunks, so S = 4 with 3 chunks per part
  L8       8, 24, 40, 24, 40, 24, 40, 24, 4 at M = 77    kMlpMaxLayers; all eight Ra buffers; the f0 / f1 alternation
  mixedS   20, 1024, 1024, 8 at M = 1000 by mlp_plan S = 16, 4, 16: the ta / tb / part layout changes from layer to layer
  regimes  as wide                       first 4 rows of x and b_1 zero (h_1 == 0 exactly); b_2 += 8 (h_2 > 0 everywhere); b_3 -= 1.5
                                         (about 3 % of h_3 == -1 exactly, a saturated unit: f' = f'' = 0)
  dead     as wide                       b_2 -= 40: h_2 == -1 everywhere, so d_2, e_1, d_1, dw_1, db_1, dw_2 and db_2 are exactly 0 and
                                         must come out exactly 0
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import mlp_grad_check as mc  # noqa: E402
from massive_marl_benchmark_amd import _lib  # noqa: E402


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.for_device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(mc.CASES))
def test_hip_build_per_tensor(name):
    lib, dev, stream = _gpu()
    inp = mc.case_inputs(name, device="cuda:0")
    L = len(inp["dims"]) - 1
    truth, yard, scale = mc.reference(inp)
    r = mc.run_abi(lib, dev, stream, inp, fill=0x00)
    stats = {}
    fails = mc.gates(r["out"], truth, yard, scale, L, stats)
    print(name, "workspace bytes", r["bytes"], stats)
    mc.record(name, stats, workspace_grad=r["bytes"][0], workspace_rop=r["bytes"][1])
    assert fails == []
    assert r["guards"], "a write outside an output"
    assert r["ws_outside"], "a write outside the workspace that the size query asked for"
    assert r["bytes"][0] > 0 and r["bytes"][1] >= r["bytes"][0]
    # no kernel reads workspace that it did not write: the same bits on a workspace of 0xFF bytes (NaN in every format involved)
    ff = mc.run_abi(lib, dev, stream, inp, fill=0xFF)
    assert ff["guards"] and ff["ws_outside"]
    for k, t in r["out"].items():
        assert _same_bits(ff["out"][k], t), ("workspace contents reach", k)
    # run to run
    again = mc.run_abi(lib, dev, stream, inp, fill=0x00)
    for k, t in r["out"].items():
        assert _same_bits(again["out"][k], t), ("not deterministic", k)
    # d_out = e_out = NULL: the same gradients, nothing else written
    bare = mc.run_abi(lib, dev, stream, inp, fill=0xFF, save=False)
    assert bare["guards"] and bare["untouched"] and bare["ws_outside"]
    assert sorted(bare["out"]) == sorted(k for k in r["out"] if k.startswith(("dw_", "db_")))
    for k, t in bare["out"].items():
        assert _same_bits(t, r["out"][k]), ("d_out / e_out change", k)


def test_workspace_and_shape_refusals():
    """Refused before any launch: nothing is written, and the message says why."""
    lib, dev, stream = _gpu()
    for name, (dims, M, _) in mc.CASES.items():
        (rc_g, n_g), (rc_r, n_r) = (mc.query(lib, dev, stream, w, dims, M) for w in ("grad", "rop"))
        assert rc_g == 0 and rc_r == 0 and n_r >= n_g > 0 and n_g % 256 == 0 and n_r % 256 == 0, (name, n_g, n_r)
    inp = mc.case_inputs("ragged", device="cuda:0")
    dims, M = inp["dims"], inp["M"]
    need = {w: mc.query(lib, dev, stream, w, dims, M)[1] for w in ("grad", "rop")}
    o = mc.outputs(dims, M, "cuda:0")
    ws = mc.Workspace(need["rop"], 0x00, "cuda:0")
    for which, call in (("grad", mc.call_grad), ("rop", mc.call_rop)):
        n = need[which]
        for what, kw, nbytes, contains in (("one byte short", {}, n - 1, "workspace too small"),
                                           ("offset by 64 bytes", {"shift": 64}, n, "256-byte aligned"),
                                           ("M = 2097025", {"M": 2097025}, n, "bad arguments"),
                                           ("layers = 9", {"L": 9}, n, "bad arguments")):
            rc = call(lib, dev, stream, inp, o, ws, nbytes, **kw)
            msg = _lib.last_error(None, lib)
            torch.cuda.synchronize()
            assert rc != 0 and contains in msg and ("mms_mlp_grad_rop" if which == "rop" else "mms_mlp_grad:") in msg, (which, what, rc, msg)
            assert all(t.all_nan() for t in o.values()), (which, what)
            assert bool((ws.buf == 0).all()), (which, what)

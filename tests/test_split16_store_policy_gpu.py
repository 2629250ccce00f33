"""The output stores of linear_split16_kernel's tail (csrc/split16_kernels.hip, TAIL instantiations) carry a cache policy per row tile
(kTailStoreCovered for row tiles 0 .. MT - 2, kTailStoreLast for row tile MT - 1).  A cache policy cannot be observed from outside;
what it could break is visibility (a consumer in stream order, a host copy behind a synchronisation) and stray or missing bytes, so
that is what is pinned here, through mms_linear_group_act_split16 as tests/test_split16_tail_gpu.py goes (its _Layer / _operands, the
helpers of test_gpu_parity.py), at the smallest shapes that put row tiles of both kinds into one tile at either height:
M = 256 / 384, N = 128 / 256, one and two networks, planes and fp32 out, K = 64 (KC 2: the tail alone), 96, 160 and the ragged 388.

* Outputs and guards: every output lies between two 4-KB guard regions, all prefilled with 0xFF.  Behind the launch and a device
  synchronisation the host copy shows both guards untouched and no prefilled ELEMENT inside the output.  (Element, not byte: a single
  0xFF byte is an ordinary mantissa byte of one output in 256; a whole fp32 0xFFFFFFFF or fp16 0xFFFF is a NaN, which no finite layer
  output is, and every store the kernel issues covers whole elements -- so one surviving element is one missed store.)
* The float64 gates of test_gpu_parity.py::test_split16_layers_error, unchanged, on every case.
* Consumer in stream order: a planes-out layer (K = 160 -> 256) feeds an fp32-out layer (256 -> 128), both tail launches, two networks,
  384 rows; the final output's digest is the same with the two launches back to back on one stream, with a device synchronisation
  between them, and as one captured graph replayed three times (intermediate and output refilled with 0xFF before every run).
* The two tile heights agree bit for bit on every case, the chain included.

The tile height is chosen by split_tiles_256, which reads MMS_SPLIT_MT once per process: the body runs in a fresh child process per
setting (this file as a script, MMS_SPLIT_MT=2 and =4, started together) and reports as JSON; the tests read the reports.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEIGHTS = (2, 4)
MS, NS, GS, KS = (256, 384), (128, 256), (1, 2), (64, 96, 160, 388)
GUARD = 4096


# ---- the child --------------------------------------------------------------------------------------------------------------------
def _guarded(torch, nbytes):
    """[guard | output | guard], all 0xFF; returns (whole buffer, the output's view)."""
    buf = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _check_cases(torch, L, report):
    import numpy as np
    from test_gpu_parity import _h32_bytes, _h32_to_f64
    from test_split16_tail_gpu import _Layer, _operands
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pad4 = lambda t, K: torch.nn.functional.pad(t, (0, (-K) % 4))
    elu = torch.nn.functional.elu
    torch.manual_seed(5)
    for M in MS:
        for N in NS:
            for K in KS:
                for planes_out in (1, 0):
                    for G in GS:
                        case = "%dx%dx%dx%d_%s" % (G, M, N, K, "planes" if planes_out else "f32")
                        x, w, b = _operands(torch, G, M, N, K, True)
                        lay = _Layer(torch, L, x, w, b, planes_out)
                        nbytes = _h32_bytes(M, N) if planes_out else M * N * 4
                        bufs = [_guarded(torch, nbytes) for _ in range(G)]
                        lay.ys = [o for _, o in bufs]
                        lay.run()
                        torch.cuda.synchronize()
                        # -- outputs and guards, on the host copy
                        for g, (buf, _) in enumerate(bufs):
                            host = buf.cpu().numpy()
                            front, body, back = host[:GUARD], host[GUARD:GUARD + nbytes], host[GUARD + nbytes:]
                            touched = int((front != 0xFF).sum()) + int((back != 0xFF).sum())
                            stale = int((body.view(np.uint16) == 0xFFFF).sum()) if planes_out else int((body.view(np.uint32) == 0xFFFFFFFF).sum())
                            if touched:
                                report["guards"].append("%s network %d: %d guard bytes written" % (case, g, touched))
                            if stale:
                                report["guards"].append("%s network %d: %d output elements still hold the prefill" % (case, g, stale))
                        report["digest"][case] = lay.digest()
                        # -- test_split16_layers_error's gates
                        y32 = [torch.empty(M, N, device="cuda") for _ in range(G)]
                        x4, w4 = [pad4(t, K) for t in x], [pad4(t, K) for t in w]     # (kept alive until the launches have run)
                        for g in range(G):
                            assert L.mms_linear2_act(0, M, N, (K + 3) // 4 * 4, p(x4[g]), p(w4[g]), p(b[g]), p(y32[g]), None, None, None, None, 1, lay.stream) == 0
                        torch.cuda.synchronize()
                        e_split, e_f32, e_torch = [], [], []
                        for g in range(G):
                            if planes_out:
                                out, v = _h32_to_f64(torch, lay.ys[g], M, N, lay.ci[g][0, 0])
                                if not float(v[:, :, 0].abs().max()) <= 2.0 ** 14:
                                    report["f64"].append("%s: a hidden activation left the bound" % case)
                            else:
                                out = lay.ys[g].view(torch.float32).view(M, N).double()
                            ref = elu(torch.nn.functional.linear(x[g].double(), w[g].double(), b[g].double()))
                            scale = x[g].abs().double() @ w[g].abs().double().t() + b[g].abs().double()
                            worst = float(((out - ref).abs() - 5e-7 * scale).max())
                            worst32 = float(((y32[g].double() - ref).abs() - 5e-7 * scale).max())
                            if not worst < 1.2e-7:
                                report["f64"].append("%s network %d: per-element bound missed by %.3e" % (case, g, worst))
                            if not worst32 < 1.2e-7:
                                report["f64"].append("%s network %d: the yardstick itself misses the per-element bound by %.3e" % (case, g, worst32))
                            keep = torch.ones(M, dtype=torch.bool, device="cuda")
                            keep[1] = keep[2] = False                   # (the two rescaled rows would dominate / vanish in an rms over all rows)
                            e_split.append((out - ref)[keep])
                            e_f32.append((y32[g].double() - ref)[keep])
                            e_torch.append((elu(torch.nn.functional.linear(x[g], w[g], b[g])).double() - ref)[keep])
                        es, ef, et = torch.cat(e_split), torch.cat(e_f32), torch.cat(e_torch)
                        rms = float(es.pow(2).mean().sqrt())
                        rms_ratio, max_ratio = rms / float(ef.pow(2).mean().sqrt()), float(es.abs().max() / ef.abs().max())
                        rms_vs_torch, max_vs_torch = rms / float(et.pow(2).mean().sqrt()), float(es.abs().max() / et.abs().max())
                        report["figures"][case] = {"rms_ratio": rms_ratio, "max_ratio": max_ratio, "mean_over_rms": float(es.mean()) / rms,
                                                   "rms_ratio_vs_torch_fp32": rms_vs_torch, "max_ratio_vs_torch_fp32": max_vs_torch}
                        if K >= 256 and not (rms_vs_torch <= 1.0 and max_vs_torch <= 1.0):
                            report["f64"].append("%s: against torch's fp32 linear rms ratio %.3f, worst ratio %.3f (<= 1.0)" % (case, rms_vs_torch, max_vs_torch))
                        if K >= 100:
                            lim = (0.6, 0.8) if K >= 256 else (0.9, 1.0)
                            if not (rms_ratio <= lim[0] and max_ratio <= lim[1]):
                                report["f64"].append("%s: rms ratio %.3f (<= %.1f), worst ratio %.3f (<= %.1f)" % (case, rms_ratio, lim[0], max_ratio, lim[1]))
                            if not abs(float(es.mean())) <= max(2.0 * abs(float(ef.mean())), (0.02 if K >= 256 else 0.05) * rms):
                                report["f64"].append("%s: biased, mean %.3e at rms %.3e" % (case, float(es.mean()), rms))
                        elif not rms_ratio <= 1.5:
                            report["f64"].append("%s: rms ratio %.3f (<= 1.5)" % (case, rms_ratio))


def _check_consumer(torch, L, report):
    """Layer A (K = 160 -> 256, planes out) -> layer B (256 -> 128, fp32 out), two networks, 384 rows: the consumer reads what the
    producer stored, whatever lies between the two launches."""
    from test_gpu_parity import _h32_bytes
    from test_split16_tail_gpu import _Layer, _operands
    torch.manual_seed(13)
    G, M, K, H, N = 2, 384, 160, 256, 128
    x, w, b = _operands(torch, G, M, H, K, False)
    a = _Layer(torch, L, x, w, b, 1)
    hbufs = [_guarded(torch, _h32_bytes(M, H)) for _ in range(G)]
    a.ys = [o for _, o in hbufs]
    # layer B: its X operand is layer A's planes under the bound chain's inverse scale; only its weights are split
    _, w2, b2 = _operands(torch, G, M, N, H, False)
    bl = _Layer(torch, L, [torch.zeros(M, H, device="cuda") for _ in range(G)], w2, b2, 0)
    bl.xp, bl.xi = a.ys, [c[0, 0] for c in a.ci]
    ybufs = [_guarded(torch, M * N * 4) for _ in range(G)]
    bl.ys = [o for _, o in ybufs]

    def refill():
        for buf, _ in hbufs + ybufs:
            buf.fill_(0xFF)

    def launch(sync_between):
        a.run()
        if sync_between:
            torch.cuda.synchronize()
        bl.run()

    def result(mode):
        torch.cuda.synchronize()
        for g, (buf, _) in enumerate(hbufs + ybufs):
            host = buf.cpu()
            if int((host[:GUARD] != 0xFF).sum()) + int((host[-GUARD:] != 0xFF).sum()):
                report["consumer"].append("%s: guard bytes of buffer %d written" % (mode, g))
        if not all(bool(torch.isfinite(y.view(torch.float32)).all()) for y in bl.ys):
            report["consumer"].append("%s: the consumer's output is not finite (it read the prefill)" % mode)
        return hashlib.sha1(b"".join(t.cpu().numpy().tobytes() for t in bl.ys)).hexdigest()

    digests = {}
    refill()
    launch(True)
    digests["synchronized"] = result("synchronized")
    refill()
    launch(False)
    digests["back_to_back"] = result("back_to_back")
    graph = torch.cuda.CUDAGraph()
    refill()
    torch.cuda.synchronize()
    keep = a.stream, bl.stream
    with torch.cuda.graph(graph):
        a.stream = bl.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        launch(False)
    a.stream, bl.stream = keep
    for i in range(3):
        refill()
        graph.replay()
        digests["graph_replay_%d" % i] = result("graph_replay_%d" % i)
    report["chain"] = digests


def _child(path):
    for d in (ROOT, HERE):
        if d not in sys.path:
            sys.path.insert(0, d)
    import torch
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    report = {"height": os.environ.get("MMS_SPLIT_MT"), "guards": [], "f64": [], "consumer": [], "digest": {}, "figures": {}, "chain": {}}
    _check_cases(torch, L, report)
    _check_consumer(torch, L, report)
    with open(path, "w") as f:
        json.dump(report, f)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    out = tmp_path_factory.mktemp("split16_store_policy")
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    procs = {}
    for mt in HEIGHTS:                                                  # fresh processes (never a replaced image), both at once
        path = str(out / ("mt%d.json" % mt))
        procs[mt] = (path, subprocess.Popen(py + [os.path.abspath(__file__), path], env=dict(os.environ, MMS_SPLIT_MT=str(mt)),
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    res = {}
    for mt, (path, proc) in procs.items():
        try:
            log = proc.communicate(timeout=180)[0].decode()
        except subprocess.TimeoutExpired:
            proc.kill()
            log = "timed out\n" + proc.communicate()[0].decode()
        assert proc.returncode == 0, "child with MMS_SPLIT_MT=%d: exit %s\n%s" % (mt, proc.returncode, log[-3000:])
        with open(path) as f:
            res[mt] = json.load(f)
        assert res[mt]["height"] == str(mt)
    return res


N_CASES = len(MS) * len(NS) * len(KS) * 2 * len(GS)


@pytest.mark.parametrize("mt", HEIGHTS)
def test_outputs_complete_and_guards_untouched(reports, mt):
    """No prefilled element inside any output, no written byte in the 4 KB in front of and behind it (_check_cases)."""
    assert len(reports[mt]["digest"]) == N_CASES
    assert reports[mt]["guards"] == []


@pytest.mark.parametrize("mt", HEIGHTS)
def test_store_policy_against_float64(reports, mt):
    """Per-element bound, rms / worst ratio and bias gates of test_split16_layers_error on every case (_check_cases)."""
    figs = reports[mt]["figures"]
    print("MMS_SPLIT_MT=%d: rms ratio %.2f-%.2f, worst ratio %.2f-%.2f over %d cases" % (
        mt, min(f["rms_ratio"] for f in figs.values()), max(f["rms_ratio"] for f in figs.values()),
        min(f["max_ratio"] for f in figs.values()), max(f["max_ratio"] for f in figs.values()), len(figs)))
    assert len(figs) == N_CASES
    assert reports[mt]["f64"] == []


@pytest.mark.parametrize("mt", HEIGHTS)
def test_consumer_in_stream_order(reports, mt):
    """Planes-out layer -> fp32-out layer: one digest whether the launches run back to back, with a synchronisation between them, or
    as a captured graph replayed three times (_check_consumer)."""
    chain = reports[mt]["chain"]
    assert sorted(chain) == ["back_to_back", "graph_replay_0", "graph_replay_1", "graph_replay_2", "synchronized"]
    assert reports[mt]["consumer"] == []
    assert len(set(chain.values())) == 1, chain


def test_tile_heights_agree(reports):
    """128-row and 256-row tiles store the same bits on every case, the chain included."""
    a, b = reports[2]["digest"], reports[4]["digest"]
    assert a.keys() == b.keys() and len(a) == N_CASES
    assert [k for k in a if a[k] != b[k]] == []
    assert reports[2]["chain"] == reports[4]["chain"]


if __name__ == "__main__":
    _child(sys.argv[1])

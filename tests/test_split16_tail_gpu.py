"""The tail of linear_split16_kernel (csrc/split16_kernels.hip, TAIL instantiations): launches of at most one tile per block take their
last two k-slices row-tile-major behind one barrier, with each row tile's epilogue between the MFMAs of the next.  Through
mms_linear_group_act_split16 exactly as test_gpu_parity.py::test_split16_layers_error goes (same helpers for planes, scales and H32
decoding), at the smallest shapes that reach every path of it: M = 256 / 384, N = 128 / 256, one and two networks, planes and fp32 out,
K = 32 ... 192 and the ragged 388 = KC 1 (the plain sequence: a single slice has no tail), 2 (the tail alone), 3 and 4 (the rolling
loop's first and last short ends), 5, 6, 13.

The tile height is chosen by split_tiles_256, which reads MMS_SPLIT_MT once per process: the body below runs in a fresh child
process per setting (this file as a script, MMS_SPLIT_MT=2 and =4, started together) and reports as JSON; the tests read the reports.
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
KS = (32, 64, 96, 128, 160, 192, 388)


# ---- the child --------------------------------------------------------------------------------------------------------------------
class _Layer:
    """One mms_linear_group_act_split16 problem: fp32 operands -> planes and scales (mms_split_planes16_group) -> the layer."""

    def __init__(self, torch, L, x, w, b, planes_out, act=1):
        from test_gpu_parity import _h32_bytes
        self.torch, self.L, self.x, self.w, self.b, self.planes_out, self.act = torch, L, x, w, b, planes_out, act
        G, (M, K), N = len(x), x[0].shape, w[0].shape[0]
        self.G, self.M, self.N, self.K = G, M, N, K
        arr = self.arr
        f32 = lambda *sh: torch.empty(*sh, device="cuda")
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        from massive_marl_benchmark_amd import _lib
        self.xp = [torch.empty(_h32_bytes(M, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        self.wp = [torch.empty(_h32_bytes(N, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        xs, self.xi, ws, self.wi = [[f32(n) for _ in range(G)] for n in (M, M, N, N)]
        # the hidden activations' scale from the bound chain of THIS layer's fp32 operands (zero padding in K changes neither)
        chain = [torch.stack([w[g].abs().sum(1).max(), b[g].abs().max()]).view(1, 1, 2).contiguous() for g in range(G)]
        self.cs, self.ci = [f32(1, 1, M) for _ in range(G)], [f32(1, 1, M) for _ in range(G)]
        _lib.check(L.mms_split_planes16_group(0, G, M, K, 0, arr(x), arr(self.xp), arr(xs), arr(self.xi), 1, 1, arr(chain), arr(self.cs), arr(self.ci), None, 0.0, self.stream),
                   None, "split16 x")
        _lib.check(L.mms_split_planes16_group(0, G, N, K, 0, arr(w), arr(self.wp), arr(ws), arr(self.wi), 0, 0, None, None, None, None, 0.0, self.stream), None, "split16 w")
        self.ys = [torch.full((_h32_bytes(M, N) if planes_out else M * N * 4,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(G)]

    @staticmethod
    def arr(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def run(self):
        from massive_marl_benchmark_amd import _lib
        arr = self.arr
        rc = self.L.mms_linear_group_act_split16(0, self.G, self.M, self.N, self.K, arr(self.xp), arr(self.wp), arr(self.b), arr(self.ys), arr(self.xi), arr(self.wi),
                                                 arr([c[0, 0] for c in self.cs]) if self.planes_out else None, self.act, self.planes_out,
                                                 None, None, None, None, None, 0, self.stream)
        assert rc == 0, _lib.last_error(None)

    def digest(self):
        self.torch.cuda.synchronize()
        return hashlib.sha1(b"".join(t.cpu().numpy().tobytes() for t in self.ys)).hexdigest()


def _operands(torch, G, M, N, K, rescaled_rows):
    x = [torch.randn(M, K, device="cuda") for _ in range(G)]
    x = [torch.where(t > 0, t, torch.expm1(t)).contiguous() for t in x]                      # ELU-shaped activations
    if rescaled_rows:
        for t in x:
            t[1] *= 1e6
            t[2] *= 1e-6
    w = [torch.randn(N, K, device="cuda") / K ** 0.5 for _ in range(G)]
    b = [torch.randn(N, device="cuda") * 0.1 for _ in range(G)]
    return x, w, b


def _check_f64(torch, L, report):
    """test_split16_layers_error's gates, unchanged, at the tail's shapes: every element within the fp32 kernel's own per-element bound
    (5e-7 of sum |x||w| + |b|, + 1.2e-7 for ELU's expf(v) - 1), the yardstick held to the same; K >= 256: rms error <= 0.6 x and worst
    error <= 0.8 x the exact-fp32 kernel's, 100 <= K < 256: 0.9 x / 1.0 x, below: rms <= 1.5 x; no mean error of its own."""
    from test_gpu_parity import _h32_to_f64
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pad4 = lambda t, K: torch.nn.functional.pad(t, (0, (-K) % 4))
    elu = torch.nn.functional.elu
    torch.manual_seed(5)
    for M in (256, 384):
        for N in (128, 256):
            for K in KS:
                for planes_out in (1, 0):
                    for G in (1, 2):
                        case = "%dx%dx%dx%d_%s" % (G, M, N, K, "planes" if planes_out else "f32")
                        x, w, b = _operands(torch, G, M, N, K, True)
                        lay = _Layer(torch, L, x, w, b, planes_out)
                        lay.run()
                        y32 = [torch.empty(M, N, device="cuda") for _ in range(G)]
                        x4, w4 = [pad4(t, K) for t in x], [pad4(t, K) for t in w]     # (kept alive until the launches have run)
                        for g in range(G):
                            assert L.mms_linear2_act(0, M, N, (K + 3) // 4 * 4, p(x4[g]), p(w4[g]), p(b[g]), p(y32[g]), None, None, None, None, 1, lay.stream) == 0
                        report["digest"][case] = lay.digest()
                        e_split, e_f32 = [], []
                        for g in range(G):
                            if planes_out:
                                out, v = _h32_to_f64(torch, lay.ys[g], M, N, lay.ci[g][0, 0])
                                if float(v[:, :, 0].abs().max()) > 2.0 ** 14:
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
                        es, ef = torch.cat(e_split), torch.cat(e_f32)
                        rms = float(es.pow(2).mean().sqrt())
                        rms_ratio, max_ratio = rms / float(ef.pow(2).mean().sqrt()), float(es.abs().max() / ef.abs().max())
                        report["figures"][case] = {"rms_ratio": rms_ratio, "max_ratio": max_ratio, "mean_over_rms": float(es.mean()) / rms}
                        if K >= 100:
                            lim = (0.6, 0.8) if K >= 256 else (0.9, 1.0)
                            if not (rms_ratio <= lim[0] and max_ratio <= lim[1]):
                                report["f64"].append("%s: rms ratio %.3f (<= %.1f), worst ratio %.3f (<= %.1f)" % (case, rms_ratio, lim[0], max_ratio, lim[1]))
                            if not abs(float(es.mean())) <= max(2.0 * abs(float(ef.mean())), (0.02 if K >= 256 else 0.05) * rms):
                                report["f64"].append("%s: biased, mean %.3e at rms %.3e" % (case, float(es.mean()), rms))
                        elif not rms_ratio <= 1.5:
                            report["f64"].append("%s: rms ratio %.3f (<= 1.5)" % (case, rms_ratio))


def _check_padding(torch, L, report):
    """A problem with K = 32 n and the same problem zero-padded in K to 32 (n + j), j = 1, 2, 3, agree bit for bit -- behind the data
    (the data runs through the rolling loop, the zeros through the tail) and in front of it (the other way round).  Zero chunks add
    +-0 to every accumulator, which changes nothing but the sign of a sum that is itself an exact zero: random normal operands have
    no such sums (and no negative zeros to begin with), so the two launches must store the same bits."""
    torch.manual_seed(7)
    zeros = lambda rows, cols: torch.zeros(rows, cols, device="cuda")
    for (G, M, N) in ((1, 256, 128), (2, 384, 256)):
        for planes_out in (1, 0):
            for n in (1, 2, 3, 4):
                x, w, b = _operands(torch, G, M, N, 32 * n, False)
                base = _Layer(torch, L, x, w, b, planes_out)
                base.run()
                want = base.digest()
                for j in (1, 2, 3):
                    for side in ("behind", "front"):
                        cat = (lambda t: torch.cat([t, zeros(t.shape[0], 32 * j)], 1).contiguous()) if side == "behind" else \
                              (lambda t: torch.cat([zeros(t.shape[0], 32 * j), t], 1).contiguous())
                        lay = _Layer(torch, L, [cat(t) for t in x], [cat(t) for t in w], b, planes_out)
                        if planes_out and not all(torch.equal(c, d) for c, d in zip(lay.cs, base.cs)):
                            report["pad"].append("the padded problem's output scales differ (the test's own premise)")
                        lay.run()
                        if lay.digest() != want:
                            diff = sum(int((s != t).sum()) for s, t in zip(lay.ys, base.ys))
                            report["pad"].append("%dx%dx%d %s: K = 32 x %d padded %s by %d chunks differs in %d bytes" %
                                                 (G, M, N, "planes" if planes_out else "f32", n, side, j, diff))


def _check_repeat(torch, L, report):
    """The kernel has no atomics: 50 launches on the same operands reproduce the first bit for bit -- a grouped shape (six networks,
    1024 x 256, K = 96) and one tile per network (256 x 128, K = 160), planes and fp32 out."""
    torch.manual_seed(11)
    for (G, M, N, K) in ((6, 1024, 256, 96), (1, 256, 128, 160)):
        for planes_out in (1, 0):
            x, w, b = _operands(torch, G, M, N, K, False)
            lay = _Layer(torch, L, x, w, b, planes_out)
            lay.run()
            torch.cuda.synchronize()
            first = [t.clone() for t in lay.ys]
            bad = torch.zeros((), dtype=torch.int64, device="cuda")
            for _ in range(50):
                for t in lay.ys:
                    t.zero_()
                lay.run()
                for t, f in zip(lay.ys, first):
                    bad += (t != f).sum()
            if int(bad) != 0:
                report["repeat"].append("%dx%dx%dx%d %s: %d bytes differ over 50 launches" % (G, M, N, K, "planes" if planes_out else "f32", int(bad)))


def _child(path):
    for d in (ROOT, HERE):
        if d not in sys.path:
            sys.path.insert(0, d)
    import torch
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    report = {"height": os.environ.get("MMS_SPLIT_MT"), "f64": [], "pad": [], "repeat": [], "digest": {}, "figures": {}}
    _check_f64(torch, L, report)
    _check_padding(torch, L, report)
    _check_repeat(torch, L, report)
    with open(path, "w") as f:
        json.dump(report, f)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    out = tmp_path_factory.mktemp("split16_tail")
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


@pytest.mark.parametrize("mt", HEIGHTS)
def test_tail_against_float64(reports, mt):
    """Per-element bound and rms / worst ratio gates of test_split16_layers_error, the exact-fp32 kernel beside it (_check_f64)."""
    figs = reports[mt]["figures"]
    print("MMS_SPLIT_MT=%d: rms ratio %.2f-%.2f, worst ratio %.2f-%.2f over %d cases" % (
        mt, min(f["rms_ratio"] for f in figs.values()), max(f["rms_ratio"] for f in figs.values()),
        min(f["max_ratio"] for f in figs.values()), max(f["max_ratio"] for f in figs.values()), len(figs)))
    assert len(figs) == 2 * 2 * len(KS) * 2 * 2
    assert reports[mt]["f64"] == []


@pytest.mark.parametrize("mt", HEIGHTS)
def test_tail_zero_padding_is_exact(reports, mt):
    """Rolling loop and tail compute the same bits: zero chunks behind / in front of the data change nothing (_check_padding)."""
    assert reports[mt]["pad"] == []


@pytest.mark.parametrize("mt", HEIGHTS)
def test_tail_repeatable(reports, mt):
    """50 launches reproduce the first bit for bit (_check_repeat)."""
    assert reports[mt]["repeat"] == []


def test_tile_heights_agree(reports):
    """128-row and 256-row tiles give every accumulator its products in the same order: the same operands (same seed in both
    children), the same bits out."""
    a, b = reports[2]["digest"], reports[4]["digest"]
    assert a.keys() == b.keys() and len(a) > 0
    assert [k for k in a if a[k] != b[k]] == []


if __name__ == "__main__":
    _child(sys.argv[1])

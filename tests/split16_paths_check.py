"""The plain (LN == 0) instantiations of linear_split16_kernel<MT, OUT, LN, ELU, TAIL> (csrc/split16_kernels.hip) and of its three-plane
sibling linear_split_kernel<MT, OUT, 0> (csrc/split_kernels.hip), one check list for both builds of the C ABI: per instantiation AND per
pipeline path.  launch_linear_split16 selects among 16 plain instantiations (MT 2 / 4 x OUT 0 / 1 x ELU x TAIL) by shape, activation and
the device's CU count; inside the persistent (TAIL = false) ones the waits differ between a block's first tile and its later tiles,
between KC = 1, 2 and > 2, and the tile mapping between XCD-aware and plain.  A wrong vmcnt count or a missing barrier there gives a
slice consumed before it landed: wrong numbers in launches with several tiles per block, never a fault.

1. expected_path / path_rows / cases: the launcher's rule restated, and shapes derived from the CU count that reach every row of it.
2. run_case: one shape and K, all activations and both output modes, against float64 per element -- the gates of
   test_gpu_parity.py::test_split16_layers_error (f16x2) / test_split_layers_error (bf16x3) unchanged, mms_linear2_act beside it.
3. ... and, for launches of several tiles per block, against the same problem as N / 128 launches of one 128-column slice each (at most
   one tile per block: the tail or the plain sequence), bit for bit.
4. check_repeat: 20 launches reproduce the first bit for bit.
5. `mutation=`: a check corrupts its own truth (or the compared copy) and returns the ratios; tests/test_split16_paths.py holds each
   to a miss of 100 x.

run_list is what a child process of tests/test_split16_paths_gpu.py runs (MMS_SPLIT_MT unset, = 2, = 4); it fills a JSON report."""
import ctypes
import hashlib

import torch

from massive_marl_benchmark_amd import _lib

KS = (32, 64, 96, 160, 100)                     # KC = 1, 2, 3, 5 and 4 with a ragged last chunk
ACTS = (0, 1, 2, 3)                             # identity, ELU, ReLU, tanh
OUTS = (0, 1)                                   # fp32 out, planes out
ACT_F64 = {0: lambda v: v, 1: torch.nn.functional.elu, 2: torch.relu, 3: torch.tanh}
SEVERAL = ("several_even", "several_ragged", "several_ragged_noxcd", "several_groups")
REPEATS = 20


# ---- 1. the path list ----------------------------------------------------------------------------------------------------------------
def expected_path(cus, forced_mt, G, M, N, K, act, out, fmt="f16x2"):
    """split_tiles_256 (csrc/layer_common.h) and the MMS_LAUNCH_SPLIT16 macro of launch_linear_split16, restated: the instantiation and
    the launch a plain layer gets on a device of `cus` CUs with MMS_SPLIT_MT = forced_mt (0: unset).
    Returns (MT, ELU, TAIL, tiles, blocks, xcd_aware); the three-plane kernel has neither ELU nor TAIL instantiations (both False)."""
    assert M % 128 == 0 and N % 128 == 0 and out in (0, 1) and act in ACTS and forced_mt in (0, 2, 4)
    tiles256 = G * (M // 256) * (N // 128) if M % 256 == 0 else 0
    big = (forced_mt == 4 and tiles256 > 0) if forced_mt else tiles256 >= cus
    MT = 4 if big else 2
    tiles = G * (M // (64 * MT)) * (N // 128)
    blocks = min(tiles, cus)                                            # persistent: at most one block per CU
    f16 = fmt == "f16x2"
    tail = f16 and tiles <= cus and (K + 31) // 32 >= 2                 # (kTail: LN == 0 and OUT != 2)
    return MT, f16 and act == 1, tail, tiles, blocks, ((tiles | blocks) & 7) == 0


def _entry(label, fmt, out, path, G):
    return [label, fmt, path[0], out, path[1], path[2], path[3], path[4], path[5], sorted(path_rows(path, G))]


def path_rows(path, G):
    """The rows of the path list a launch belongs to."""
    MT, elu, tail, tiles, blocks, xcd = path
    if tiles <= blocks:
        return {"one_tail" if tail else "one_plain"}
    rows = {"several_groups"} if G > 2 else set()                       # (a.x[gi] / a.w[gi] for gi >= 2 are loaded in the tile setup)
    if tiles == 2 * blocks:
        rows.add("several_even")
    if tiles % blocks:
        rows.add("several_ragged" if xcd else "several_ragged_noxcd")
    return rows


def required(fmt="f16x2"):
    """Every (MT, OUT, ELU, TAIL, row) the three child processes together must have launched."""
    need = set()
    for MT in (2, 4):
        for out in OUTS:
            if fmt != "f16x2":                                          # linear_split_kernel<MT, OUT, 0>: one tile per block and several
                need |= {(MT, out, False, False, "one_plain"), (MT, out, False, False, "several_ragged")}
                continue
            for elu in (True, False):
                need |= {(MT, out, elu, False, row) for row in SEVERAL + ("one_plain",)}
                need.add((MT, out, elu, True, "one_tail"))
    return need


def _first(per, cus, ok):
    for nt in range(1, 64):
        if per * nt > cus and (per * nt) % cus != 0 and ok(per * nt):
            return 128 * nt
    raise AssertionError("no ragged shape at %d tiles per 128 columns on %d CUs" % (per, cus))


def _even(cus, MT):
    """(G, M, N) with exactly two tiles of 64 MT rows per block; at MT = 2 with an M the launcher cannot tile by 256 rows"""
    for G in range(32, 2, -1):
        for k in ((2, 1, 4) if MT == 4 else (1, 3, 5)):
            if (2 * cus) % (G * k) == 0 and (2 * cus) // (G * k) <= 32:
                return G, 64 * MT * k, 128 * ((2 * cus) // (G * k))
    raise AssertionError("no shape gives %d CUs two tiles each" % cus)


def cases(cus, forced_mt):
    """[(name, G, M, N, want)]: the same shapes for every setting of MMS_SPLIT_MT (equal cases must give equal bits in all three
    processes); want = (MT, row) where the setting selects the path the shape was made for, else None.  On 256 CUs: 32 x 512 x 640 is
    320 tiles of 256 rows, x 1024 is 512, 31 x 512 x 640 is 310 (not a multiple of 8); 32 x 384 x 384 is 288 tiles of 128 rows,
    32 x 128 x 2048 is 512, 31 x 384 x 384 is 279; three networks of 256 x 128 are one tile per block at either height."""
    assert cus % 8 == 0 and cus >= 128, "the XCD-aware tile mapping needs a grid that is a multiple of 8"
    m4 = forced_mt in (0, 4)
    out = [("one", 3, 256, 128, (4 if forced_mt == 4 else 2, "one"))]
    out.append(("mt4_ragged", 32, 512, _first(64, cus, lambda t: t % 8 == 0), (4, "several_ragged") if m4 else None))
    out.append(("mt4_even",) + _even(cus, 4) + ((4, "several_even") if m4 else None,))
    out.append(("mt4_noxcd", 31, 512, _first(62, cus, lambda t: t % 8 != 0), (4, "several_ragged_noxcd") if m4 else None))
    out.append(("mt2_ragged", 32, 384, _first(96, cus, lambda t: t % 8 == 0), (2, "several_ragged")))
    out.append(("mt2_even",) + _even(cus, 2) + ((2, "several_even"),))
    out.append(("mt2_noxcd", 31, 384, _first(93, cus, lambda t: t % 8 != 0), (2, "several_ragged_noxcd")))
    for name, G, M, N, want in out:
        for K in KS:
            path = expected_path(cus, forced_mt, G, M, N, K, 0, 0)
            rows = path_rows(path, G)
            if want is not None:
                row = want[1] if want[1] != "one" else ("one_plain" if K == 32 else "one_tail")
                assert path[0] == want[0] and row in rows and (G <= 2 or path[3] <= path[4] or "several_groups" in rows), (name, cus, forced_mt, K, path, rows)
            if path[3] > path[4]:                                       # the slices of section 3 are launches of at most one tile per block
                sl = expected_path(cus, forced_mt, G, M, 128, K, 0, 0)
                assert sl[3] <= sl[4], (name, cus, sl)
    return out


def cases3(cus, forced_mt):
    """The three-plane kernel's four plain instantiations, one tile per block and several: a subset of the same shapes."""
    return [c for c in cases(cus, forced_mt) if c[0] in ("one", "mt4_ragged", "mt2_ragged")]


# ---- operands and launches -----------------------------------------------------------------------------------------------------------
def _ptrs(ts, off=0):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() + off for t in ts])


def _sync(tdev):
    if tdev != "cpu":
        torch.cuda.synchronize()


def plane_bytes(fmt, rows, K):
    return rows * ((K + 31) // 32) * (128 if fmt == "f16x2" else 192)


def operands(tdev, fmt, G, M, N, K, seed):
    """test_split16_layers_error's recipe: ELU-shaped inputs, rows 1 and 2 scaled by 1e6 and 1e-6 (f16x2: their plane scales differ by
    2^40; the three-plane format has no scales and test_split_layers_error no such rows), weights randn / sqrt(K), biases 0.1 randn."""
    gen = torch.Generator(device=tdev)
    gen.manual_seed(seed)
    x = torch.randn(G, M, K, device=tdev, generator=gen)
    x = torch.where(x > 0, x, torch.expm1(x)).contiguous()
    if fmt == "f16x2":
        x[:, 1] *= 1e6
        x[:, 2] *= 1e-6
    w = torch.randn(G, N, K, device=tdev, generator=gen) / K ** 0.5
    b = torch.randn(G, N, device=tdev, generator=gen) * 0.1
    return x, w, b


class Layer:
    """One mms_linear_group_act_split16 / mms_linear_group_act_split problem: fp32 operands -> planes (and scales, and the bound chain's
    y_scale) -> the layer, whole or one 128-column slice of it."""

    def __init__(self, env, fmt, x, w, b):
        self.L, self.di, self.stream, self.tdev = env
        L, di, stream, tdev = env
        self.fmt, self.x, self.w, self.b = fmt, x, w, b
        (G, M, K), N = x.shape, w.shape[1]
        self.G, self.M, self.N, self.K = G, M, N, K
        u8 = lambda n: torch.zeros(G, n, dtype=torch.uint8, device=tdev)
        self.xp, self.wp = u8(plane_bytes(fmt, M, K)), u8(plane_bytes(fmt, N, K))
        if fmt == "f16x2":
            f32 = lambda n: torch.empty(G, n, device=tdev)
            xs, self.xi, ws, self.wi, self.cs, self.ci = f32(M), f32(M), f32(N), f32(N), f32(M), f32(M)
            # the hidden activations' scale from the bound chain of THIS layer's fp32 operands
            chain = torch.stack([w.abs().sum(2).max(1).values, b.abs().max(1).values], 1).contiguous()
            _lib.check(L.mms_split_planes16_group(di, G, M, K, 0, _ptrs(x), _ptrs(self.xp), _ptrs(xs), _ptrs(self.xi), 1, 1, _ptrs(chain), _ptrs(self.cs), _ptrs(self.ci),
                                                  None, 0.0, stream), None, "split16 x", L)
            _lib.check(L.mms_split_planes16_group(di, G, N, K, 0, _ptrs(w), _ptrs(self.wp), _ptrs(ws), _ptrs(self.wi), 0, 0, None, None, None, None, 0.0, stream),
                       None, "split16 w", L)
        else:
            _lib.check(L.mms_split_planes_group(di, G, M, K, 0, _ptrs(x), _ptrs(self.xp), stream), None, "split x", L)
            _lib.check(L.mms_split_planes_group(di, G, N, K, 0, _ptrs(w), _ptrs(self.wp), stream), None, "split w", L)

    def per(self, out):
        """bytes per output element: a float, two fp16 planes, or three bf16 planes"""
        return (4 if self.fmt == "f16x2" else 6) if out else 4

    def output(self, out, N=None):
        """[G, M + 1, row bytes], poisoned; the last row is the guard"""
        return torch.full((self.G, self.M + 1, self.per(out) * (N or self.N)), 0xFF, dtype=torch.uint8, device=self.tdev)

    def run(self, ys, act, out, col0=None):
        """the whole layer into ys, or (col0 given) its columns [col0, col0 + 128) as a launch of its own with N = 128"""
        L, KC = self.L, (self.K + 31) // 32
        N = self.N if col0 is None else 128
        c0 = col0 or 0
        wp = _ptrs(self.wp, c0 * KC * (128 if self.fmt == "f16x2" else 192))
        if self.fmt == "f16x2":
            rc = L.mms_linear_group_act_split16(self.di, self.G, self.M, N, self.K, _ptrs(self.xp), wp, _ptrs(self.b, 4 * c0), _ptrs(ys), _ptrs(self.xi),
                                                _ptrs(self.wi, 4 * c0), _ptrs(self.cs) if out else None, act, out, None, None, None, None, None, None, self.stream)
        else:
            rc = L.mms_linear_group_act_split(self.di, self.G, self.M, N, self.K, _ptrs(self.xp), wp, _ptrs(self.b, 4 * c0), _ptrs(ys), act, out,
                                              None, None, None, None, None, None, self.stream)
        assert rc == 0, _lib.last_error(None, L)

    def body(self, ys):
        """the M rows' bytes of an output buffer, [G, M, row bytes]"""
        return ys[:, :self.M]

    def guard_intact(self, ys):
        return bool((ys[:, self.M] == 0xFF).all())

    def decode(self, ys, out):
        """-> (float64 [G, M, N], largest |hi plane| of a planes output or None)"""
        G, M, N = self.G, self.M, self.N
        raw = self.body(ys).contiguous()
        if not out:
            return raw.view(torch.float32).view(G, M, N).double(), None
        if self.fmt == "f16x2":                                         # test_gpu_parity._h32_to_f64
            v = raw.view(torch.float16).view(G, M, N // 32, 2, 32).double()
            return (v[:, :, :, 0] + v[:, :, :, 1] / 2048.0).reshape(G, M, N) * self.ci.double()[:, :, None], float(v[:, :, :, 0].abs().max())
        v = raw.view(torch.bfloat16).view(G, M, N // 32, 3, 32).float()   # test_gpu_parity._planes_to_f32: the planes sum exactly in fp32
        return ((v[:, :, :, 0] + v[:, :, :, 1]) + v[:, :, :, 2]).reshape(G, M, N).double(), None

    def hi_only(self):
        """the operands the hi planes alone stand for (f16x2): what a kernel without the cross terms multiplies"""
        G, M, N, K = self.G, self.M, self.N, self.K
        KC = (K + 31) // 32
        xh = self.xp.view(torch.float16).view(G, M, KC, 2, 32)[:, :, :, 0].double().reshape(G, M, KC * 32)[:, :, :K] * self.xi.double()[:, :, None]
        wh = self.wp.view(torch.float16).view(G, N, KC, 2, 32)[:, :, :, 0].double().reshape(G, N, KC * 32)[:, :, :K] * self.wi.double()[:, :, None]
        return xh, wh

    def yardstick(self, act):
        """mms_linear2_act, the exact-fp32 layer kernel, on the same fp32 operands (two networks per launch)"""
        G, M, N, K = self.G, self.M, self.N, self.K
        pad = (-K) % 4
        if not hasattr(self, "_x4"):
            self._x4, self._w4 = torch.nn.functional.pad(self.x, (0, pad)).contiguous(), torch.nn.functional.pad(self.w, (0, pad)).contiguous()
        y = torch.empty(G, M, N, device=self.tdev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        for g in range(0, G, 2):
            two = g + 1 < G
            rc = self.L.mms_linear2_act(self.di, M, N, K + pad, p(self._x4[g]), p(self._w4[g]), p(self.b[g]), p(y[g]),
                                        p(self._x4[g + 1]) if two else None, p(self._w4[g + 1]) if two else None, p(self.b[g + 1]) if two else None,
                                        p(y[g + 1]) if two else None, act, self.stream)
            assert rc == 0, _lib.last_error(None, self.L)
        return y


_WEIGHTS = {}


def digest(t):
    """64 bits of a byte tensor, computed where it lives: sum of its int64 words times fixed odd position weights, modulo 2^64"""
    if t.device.type == "cpu":
        return hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()[:16]
    words = t.contiguous().view(-1).view(torch.int64)
    key = (words.numel(), t.device)
    if key not in _WEIGHTS:
        _WEIGHTS.clear()
        _WEIGHTS[key] = (torch.arange(words.numel(), dtype=torch.int64, device=t.device) * 0x632BE59BD9B4E019 + 0x2545F4914F6CDD1D) | 1
    return "%016x" % (int((words * _WEIGHTS[key]).sum()) & (2 ** 64 - 1))


# ---- 2. / 3. one shape and K: float64 per element, slices bit for bit -----------------------------------------------------------------
def gate_elem(fmt, err, scale):
    """worst |error| / per-element bound: test_split16_layers_error's `max(|e| - 5e-7 scale) < 1.2e-7` (the 1.2e-7: half an ulp of 1 in
    expf(v) - 1, visible in the tiny row), test_split_layers_error's `max(|e| / scale) < 5e-7`"""
    return float((err.abs() / (5e-7 * scale + (1.2e-7 if fmt == "f16x2" else 0.0))).max())


def run_case(env, cus, forced_mt, fmt, name, G, M, N, K, acts=ACTS, outs=OUTS, ratios=True, slices=True, mutation=None, seed=5, report=None):
    """Sections 2 and 3 for one (shape, K): every activation x output mode.  Returns {label: figures}; failures go to report["f64"] /
    report["bits"] (raised as an assertion if no report is given).  slices: True = where the launch has several tiles per block, "always".  ratios: the rms / worst-ratio / mean rules against the exact-fp32
    kernel (the HIP build; the CPU build sums the planes back and runs mms_linear2_act's own fmaf chain, so there the ratio is 1 by
    construction).  mutation: see section 5 below -- then nothing is asserted and the figures carry the ratios."""
    tdev = env[3]
    rep = report if report is not None else {"f64": [], "bits": [], "paths": [], "digest": {}, "figures": {}}
    x, w, b = operands(tdev, fmt, G, M, N, K, seed)
    lay = Layer(env, fmt, x, w, b)
    xd, wd, bd = x.double(), w.double(), b.double()
    pre = torch.baddbmm(bd[:, None, :], xd, wd.transpose(1, 2))
    scale = torch.baddbmm(bd.abs()[:, None, :], xd.abs(), wd.abs().transpose(1, 2))
    if mutation == "drop_k":                                            # one 32-column k-slice dropped from one tile of the truth
        pre[G - 1, 128:256, 0:128] -= xd[G - 1, 128:256, 32:64] @ wd[G - 1, 0:128, 32:64].t()
    if mutation == "hi_only":                                           # the truth without the lo cross terms
        xh, wh = lay.hi_only()
        pre = torch.baddbmm(bd[:, None, :], xh, wh.transpose(1, 2))
    keep = torch.ones(M, dtype=torch.bool, device=tdev)
    if fmt == "f16x2":
        keep[1] = keep[2] = False                                       # (the two rescaled rows would dominate / vanish in an rms over all rows)
    figs = {}
    for act in acts:
        ref = ACT_F64[0 if mutation == "relu_as_identity" else act](pre)
        y32 = lay.yardstick(act).double()
        e32 = y32 - ref
        for out in outs:
            label = "%s_%s_%dx%dx%dx%d_act%d_%s" % (fmt, name, G, M, N, K, act, "planes" if out else "f32")
            path = expected_path(cus, forced_mt, G, M, N, K, act, out, fmt)
            rows = sorted(path_rows(path, G))
            rep["paths"].append(_entry(label, fmt, out, path, G))
            print("%s: MT %d ELU %d TAIL %d, %d tiles on %d blocks, %s mapping: %s" % (label, path[0], path[1], path[2], path[3], path[4],
                                                                                       "XCD-aware" if path[5] else "plain", ", ".join(rows)))
            ys = lay.output(out)
            lay.run(ys, act, out)
            _sync(tdev)
            if mutation == "swap_tiles":                                # two tiles of the compared copy swapped (128 columns are 512 bytes of a row, floats or fp16 planes)
                assert fmt == "f16x2" or not out
                t = ys[0, 0:128, 0:512].clone()
                ys[0, 0:128, 0:512] = ys[0, 128:256, 0:512]
                ys[0, 128:256, 0:512] = t
            got, top = lay.decode(ys, out)
            err = got - ref
            f = {"fmt": fmt, "K": K, "elem": gate_elem(fmt, err, scale), "yardstick": gate_elem(fmt, e32, scale)}
            es, ef = err[:, keep], e32[:, keep]
            rms = float(es.pow(2).mean().sqrt())
            f["rms_ratio"], f["max_ratio"] = rms / float(ef.pow(2).mean().sqrt()), float(es.abs().max() / ef.abs().max())
            f["mean_over_rms"] = float(es.mean()) / rms
            bad = []
            if not f["elem"] < 1.0:
                bad.append("per-element bound missed, worst error / bound %.3f" % f["elem"])
            if not f["yardstick"] < 1.0:
                bad.append("the yardstick itself misses the per-element bound, %.3f" % f["yardstick"])
            if top is not None and top > 2.0 ** 14:
                bad.append("a hidden activation left the bound: hi plane up to %g" % top)
            if not lay.guard_intact(ys):
                bad.append("the guard row was written")
            if ratios and K >= 100:
                # K >= 256 would be (0.6, 0.8) and 0.02 in the two-plane test; every K of this list is below
                lim, bias = ((0.9, 1.0), 0.05) if fmt == "f16x2" else ((0.5, 0.8), 0.02)
                if not (f["rms_ratio"] <= lim[0] and f["max_ratio"] <= lim[1]):
                    bad.append("rms ratio %.3f (<= %.1f), worst ratio %.3f (<= %.1f)" % (f["rms_ratio"], lim[0], f["max_ratio"], lim[1]))
                if not abs(float(es.mean())) <= max(2.0 * abs(float(ef.mean())), bias * rms):
                    bad.append("biased, mean %.3e at rms %.3e (the yardstick's mean %.3e)" % (float(es.mean()), rms, float(ef.mean())))
            elif ratios and fmt == "f16x2" and not f["rms_ratio"] <= 1.5:
                bad.append("rms ratio %.3f (<= 1.5)" % f["rms_ratio"])
            rep["f64"] += ["%s: %s" % (label, s) for s in bad]
            rep["digest"][label] = digest(lay.body(ys))
            if slices == "always" or (slices and path[3] > path[4]) or mutation == "swap_tiles":
                f["slice_bytes_differ"] = _compare_slices(lay, cus, forced_mt, ys, act, out, label, rep)
            figs[label] = f
    rep["figures"].update(figs)
    if report is None and mutation is None:
        assert rep["f64"] == [] and rep["bits"] == [], (rep["f64"], rep["bits"])
    return figs


def _compare_slices(lay, cus, forced_mt, ys, act, out, label, rep):
    """Section 3: the rolling loop, the tail and the plain sequence give every accumulator its products in the same order and run the
    same epilogue statements, so the layer as N / 128 launches of one 128-column slice (all networks, all rows, at most one tile per
    block: offset w, b and w_inv pointers, a dense [M, 128] output) stores the bits of the full launch's columns."""
    per = lay.per(out)
    full = lay.body(ys)
    differ = 0
    for j in range(lay.N // 128):
        path = expected_path(cus, forced_mt, lay.G, lay.M, 128, lay.K, act, out, lay.fmt)
        assert path[3] <= path[4], ("a slice launch with several tiles per block", path)
        if j == 0:
            rep["paths"].append(_entry(label + "_slice", lay.fmt, out, path, lay.G))
        sl = lay.output(out, 128)
        lay.run(sl, act, out, col0=128 * j)
        _sync(lay.tdev)
        if not lay.guard_intact(sl):
            rep["bits"].append("%s slice %d: the guard row was written" % (label, j))
        ne = lay.body(sl) != full[:, :, per * 128 * j:per * 128 * (j + 1)]
        n = int(ne.sum())
        if n:
            g, m, c = [int(v) for v in ne.nonzero()[0]]
            rep["bits"].append("%s slice %d: %d bytes differ from the full launch, first at network %d row %d column %d (tiles of %d rows)" % (
                label, j, n, g, m, 128 * j + c // per, 64 * expected_path(cus, forced_mt, lay.G, lay.M, lay.N, lay.K, act, out, lay.fmt)[0]))
        differ += n
    return differ


# ---- 4. run to run ---------------------------------------------------------------------------------------------------------------------
def check_repeat(env, cus, forced_mt, fmt, name, G, M, N, K, report, acts=(1, 2), launches=REPEATS):
    """The kernels have no atomics: `launches` launches on the same operands, outputs zeroed in between, reproduce the first."""
    tdev = env[3]
    x, w, b = operands(tdev, fmt, G, M, N, K, 11)
    lay = Layer(env, fmt, x, w, b)
    for act in acts:
        for out in OUTS:
            ys = lay.output(out)
            lay.run(ys, act, out)
            _sync(tdev)
            first = ys.clone()
            bad = torch.zeros((), dtype=torch.int64, device=tdev)
            for _ in range(launches):
                ys.zero_()
                lay.run(ys, act, out)
                bad += (lay.body(ys) != lay.body(first)).sum()
            path = expected_path(cus, forced_mt, G, M, N, K, act, out, fmt)
            report["repeated"].append([fmt, path[0], out, path[1], sorted(path_rows(path, G))])
            if int(bad) != 0:
                report["repeat"].append("%s %s %dx%dx%dx%d act %d %s: %d bytes differ over %d launches" % (fmt, name, G, M, N, K, act, "planes" if out else "f32",
                                                                                                        int(bad), launches))


# ---- what one child process runs ------------------------------------------------------------------------------------------------------
def new_report(cus, forced_mt):
    return {"cus": cus, "forced_mt": forced_mt, "f64": [], "bits": [], "repeat": [], "paths": [], "repeated": [], "digest": {}, "figures": {}}


def plan(cus, forced_mt):
    """[(fmt, name, G, M, N, Ks, acts, K of the repeat check or None)]: the two-plane kernel at every shape x K x activation x output
    mode; the three-plane kernel (no tail, no compile-time activation) at one tile per block and the two ragged shapes"""
    out = [("f16x2", name, G, M, N, KS, ACTS, 96 if name != "one" else None) for name, G, M, N, want in cases(cus, forced_mt)]
    return out + [("bf16x3", name, G, M, N, (64, 100), (1, 2), 96 if name != "one" else None) for name, G, M, N, want in cases3(cus, forced_mt)]


def planned_paths(cus, forced_mt):
    """The `paths` entries run_list will report on such a device, without a launch (tests/test_split16_paths.py: the list covers every
    instantiation and row on 256 and on 304 CUs)."""
    out = []
    for fmt, name, G, M, N, Ks, acts, _ in plan(cus, forced_mt):
        for K in Ks:
            for act in acts:
                for o in OUTS:
                    path = expected_path(cus, forced_mt, G, M, N, K, act, o, fmt)
                    out.append(_entry("", fmt, o, path, G))
                    if path[3] > path[4]:
                        out.append(_entry("", fmt, o, expected_path(cus, forced_mt, G, M, 128, K, act, o, fmt), G))
    return out


def run_list(env, cus, forced_mt, report):
    for fmt, name, G, M, N, Ks, acts, k_repeat in plan(cus, forced_mt):
        for K in Ks:
            run_case(env, cus, forced_mt, fmt, name, G, M, N, K, acts=acts, report=report)
        if k_repeat:
            check_repeat(env, cus, forced_mt, fmt, name, G, M, N, k_repeat, report, acts=(1, 2) if fmt == "f16x2" else (1,))
    return report


def coverage(reports, fmt="f16x2"):
    """-> (launched, missing): the (MT, OUT, ELU, TAIL, row) combinations the reports' launches reached, and those of required() they did not"""
    seen = set()
    for r in reports:
        for label, f, MT, out, elu, tail, tiles, blocks, xcd, rows in r["paths"]:
            if f == fmt:
                seen |= {(MT, out, bool(elu), bool(tail), row) for row in rows}
    return seen, required(fmt) - seen

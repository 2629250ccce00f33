"""Checks of mms_mlp_grad / mms_mlp_grad_rop (include/mms.h, csrc/trpo_kernels.hip) through the C ABI, shared by the CPU-build tests
(test_mlp_grad_abi.py) and the GPU tests (test_mlp_grad_abi_gpu.py): seeded inputs, the closed form of both entries in torch, the call
through ctypes with guarded outputs and an exactly sized workspace, and the gates, per output tensor.

At the ABI h, g, V and c are inputs, so the float64 truth and the fp32 yardstick are the SAME formulas on the SAME inputs as the
kernels' (no forward pass of the module in between, no autograd summation order).  Gates, per tensor, err = out - truth in float64:
  (a) every element finite;
  (b) max |err| / scale <= 5e-7 x depth, scale = the same recursion in float64 on the absolute values of every operand and factor
      (so where scale is 0 the exact result is 0 term by term, and the output must be exactly 0); 5e-7 is the project's per-element
      bound for one fp32 GEMM with K <= 1028 (test_gpu_parity.py: test_linear2_act_kernel, test_split_layers_error), depth the number
      of chained products from the inputs to the tensor;
  (c) n >= 64:   rms(err) <= max(m x rms(yard - truth), 2^-24 x rms(truth)), m = 1.25 for n >= 1024 and 2.0 below;
  (d) n >= 1024: max |err| <= max(3 x max |yard - truth|, 2^-23 x max |truth|).
The margins of (c) and (d) are the spread between two equally good fp32 evaluations of these formulas (torch fp32 against torch fp32
with a permuted contraction order, over CASES with two seeds: rms ratio <= 1.09 for n >= 1024 and <= 1.73 below, max ratio <= 2.2),
not anything measured on the kernels: they are documented as no worse than fp32 and get that spread and no more.  A wrong element is
off by about rms(truth), some 10^6 rounding levels.  Tensors under 64 elements get (a) and (b) only: a yardstick error over a handful
of elements can be 0 by accident."""
import ctypes

import torch

from massive_marl_benchmark_amd import _lib

GUARD = 64               # floats of NaN on each side of every output
WS_PAD = 512             # bytes of fill around the workspace slice (the slice starts at a 256-aligned address inside)
PER_GEMM = 5e-7

WIDE = (36, 130, 257, 20, 6)
# name -> (dims, M, options of make_inputs).  What each reaches: the table in test_mlp_grad_abi_gpu.py
CASES = {
    "min": ((12, 40, 5), 1, {}),
    "ones": ((1, 1, 1), 33, {}),
    "ragged": ((33, 65, 31, 7), 129, {}),
    "wide": (WIDE, 300, {}),
    "L8": ((8, 24, 40, 24, 40, 24, 40, 24, 4), 77, {}),
    "mixedS": ((20, 1024, 1024, 8), 1000, {}),
    "regimes": (WIDE, 300, {"zero_rows": 4, "bias_shift": {2: 8.0, 3: -1.5}}),
    "dead": (WIDE, 300, {"bias_shift": {2: -40.0}}),
}


def make_inputs(dims, M, seed, zero_rows=0, bias_shift=None, round_h=True, device="cpu"):
    """x ~ N(0,1), W_l ~ N(0,1) / sqrt(fan_in), b_l ~ 0.1 N(0,1), V_l and c_l ~ N(0,1), g ~ N(0,1) / M, all fp32 values; h_l from a
    float64 forward, rounded to fp32 after each layer (round_h=False: kept in float64, unrounded -- what autograd's own float64 forward
    holds).  zero_rows: the first rows of x and all of b_1 are zero (h_1 == 0 exactly there); bias_shift {l: c}: b_l += c."""
    L = len(dims) - 1
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = rn(M, dims[0])
    W = [rn(dims[l], dims[l - 1]) / dims[l - 1] ** 0.5 for l in range(1, L + 1)]
    b = [0.1 * rn(dims[l]) for l in range(1, L + 1)]
    V = [rn(dims[l], dims[l - 1]) for l in range(1, L + 1)]
    C = [rn(dims[l]) for l in range(1, L + 1)]
    g = rn(M, dims[L]) / M
    if zero_rows:
        x[:zero_rows] = 0.0
        b[0].zero_()
    for l, c in (bias_shift or {}).items():
        b[l - 1] += c
    h, cur = [], x.double()
    for l in range(1, L):
        a = cur @ W[l - 1].double().t() + b[l - 1].double()
        hl = torch.where(a > 0, a, torch.expm1(a))
        if round_h:
            hl = hl.float()
        h.append(hl)
        cur = hl.double()
    to = lambda t: t.contiguous().to(device)
    return {"dims": tuple(dims), "M": M, "x": to(x), "W": [to(t) for t in W], "b": [to(t) for t in b], "V": [to(t) for t in V],
            "C": [to(t) for t in C], "g": to(g), "h": [to(t) for t in h]}


def case_inputs(name, seed=0, device="cpu", **kw):
    dims, M, opt = CASES[name]
    return make_inputs(dims, M, seed, device=device, **dict(opt, **kw))


def closed_form(dims, x, h, W, g, V, C, dtype, absolute=False, fpp=True):
    """Every output of mms_mlp_grad and mms_mlp_grad_rop by name (dw_l, db_l, l = 1..L; d_l, e_l, l = 1..L-1; rmu; rdw_l, rdb_l), the
    formulas of include/mms.h with torch ops in `dtype`.  f' and f'' are read from h as given: h > 0 ? 1 : h + 1 and h > 0 ? 0 : h + 1.
    absolute: the same recursion in float64 on |.| of every operand and factor -- the per-element scale.  fpp=False leaves the f''
    term of Rd out (a mutation for the harness's own test)."""
    L = len(dims) - 1
    if absolute:
        dtype = torch.float64
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    c = lambda t: ab(t.to(dtype))
    f1 = [ab(torch.where(t > 0, torch.ones_like(t), t + 1).to(dtype)) for t in h]          # f'(h_l), l = 1..L-1 at index l-1
    f2 = [ab(torch.where(t > 0, torch.zeros_like(t), t + 1).to(dtype)) for t in h]
    hin = [c(x)] + [c(t) for t in h]                                                       # h_0 .. h_{L-1}
    W, V, C, g = [c(t) for t in W], [c(t) for t in V], [c(t) for t in C], c(g)
    out = {}
    d, e = [None] * (L + 1), [None] * (L + 1)
    d[L] = g
    for l in range(L, 0, -1):
        out["dw_%d" % l] = d[l].t() @ hin[l - 1]
        out["db_%d" % l] = d[l].sum(0)
        if l > 1:
            e[l - 1] = d[l] @ W[l - 1]
            d[l - 1] = e[l - 1] * f1[l - 2]
            out["e_%d" % (l - 1)], out["d_%d" % (l - 1)] = e[l - 1], d[l - 1]
    ra, rh = [None] * (L + 1), [None] * (L + 1)
    for l in range(1, L + 1):
        ra[l] = hin[l - 1] @ V[l - 1].t() + C[l - 1]
        if l > 1:
            ra[l] = rh[l - 1] @ W[l - 1].t() + ra[l]
        if l < L:
            rh[l] = f1[l - 1] * ra[l]
    out["rmu"] = ra[L]
    rd = None                                                                              # Rd_L = 0
    for l in range(L, 0, -1):
        rdw = None
        if l < L:
            rdw = rd.t() @ hin[l - 1]
        if l > 1:
            t = d[l].t() @ rh[l - 1]
            rdw = t if rdw is None else rdw + t
        out["rdw_%d" % l] = rdw
        out["rdb_%d" % l] = rd.sum(0) if l < L else torch.zeros_like(C[l - 1])
        if l > 1:
            t = d[l] @ V[l - 1]
            if l < L:
                t = rd @ W[l - 1] + t
            rd = t * f1[l - 2]
            if fpp:
                rd = rd + e[l - 1] * f2[l - 2] * ra[l - 1]
    return out


def reference(inp):
    """(truth in float64, fp32 yardstick, per-element scale) of every output, on the inputs' own device."""
    a = (inp["dims"], inp["x"], inp["h"], inp["W"], inp["g"], inp["V"], inp["C"])
    return closed_form(*a, torch.float64), closed_form(*a, torch.float32), closed_form(*a, torch.float64, absolute=True)


def depth(name, L):
    """Chained products from the inputs to the tensor."""
    kind, _, l = name.partition("_")
    if kind == "rmu":
        return L
    l = int(l)
    return {"d": L - l, "e": L - l, "dw": L - l + 1, "db": L - l + 1, "rdw": 2 * L, "rdb": 2 * L}[kind]


def _rms(t):
    return float(t.pow(2).mean().sqrt())


def gates(out, truth, yard, scale, L, stats=None):
    """The failures of gates (a)-(d) (module docstring) over every tensor of `truth`.  stats (a dict), when given, receives the worst
    figures with their tensors: "b" = max |err| / scale / depth (allowed 5e-7), "c" = rms(err) over max(rms(yard - truth),
    2^-24 rms(truth) / m) (allowed m), "d" = max |err| over max(max |yard - truth|, 2^-23 max |truth| / 3) (allowed 3)."""
    fails = []
    worst = {"b": (0.0, None), "c": (0.0, None), "d": (0.0, None)}

    def note(k, v, name):
        if v > worst[k][0]:
            worst[k] = (v, name)

    for name, t in truth.items():
        o = out[name].double().reshape(t.shape)
        n = t.numel()
        if not bool(torch.isfinite(o).all()):
            fails.append((name, "a: not finite"))
            continue
        err, yerr, sc = o - t, yard[name].double() - t, scale[name]
        zero = sc == 0
        if bool((o[zero] != 0).any()):
            fails.append((name, "b: not exactly 0 where the scale is 0", float(o[zero].abs().max())))
        dp = depth(name, L)
        if bool((~zero).any()):
            rel = float((err[~zero].abs() / sc[~zero]).max())
            note("b", rel / max(dp, 1), name)
            if rel > PER_GEMM * dp:
                fails.append((name, "b: max |err| / scale", rel, PER_GEMM * dp))
        if n >= 64:
            m = 1.25 if n >= 1024 else 2.0
            e, y, fl = _rms(err), _rms(yerr), 2.0 ** -24 * _rms(t)
            if e > 0:
                note("c", e / max(y, fl / m), name)
            if e > max(m * y, fl):
                fails.append((name, "c: rms(err)", e, "yardstick", y, "allowed", max(m * y, fl)))
        if n >= 1024:
            e, y, fl = float(err.abs().max()), float(yerr.abs().max()), 2.0 ** -23 * float(t.abs().max())
            if e > 0:
                note("d", e / max(y, fl / 3.0), name)
            if e > max(3.0 * y, fl):
                fails.append((name, "d: max |err|", e, "yardstick", y, "allowed", max(3.0 * y, fl)))
    if stats is not None:
        stats.update(worst)
    return fails


def record(case, stats, prefix="gpu", **extra):
    """The measured figures of one case into the margins file (tests/parity.py)."""
    import parity
    parity.record(prefix + "/mlp_grad_abi/" + case, c_ratio=stats["c"][0], c_tensor=stats["c"][1], d_ratio=stats["d"][0], d_tensor=stats["d"][1],
                  b_value=stats["b"][0], b_tensor=stats["b"][1], **extra)


# ---- the call ------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ptrs(ts, n=None):
    ts = list(ts)
    ts = ts + [ts[-1]] * ((n or 0) - len(ts))
    return (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


class Guarded:
    """A float32 output of `shape` inside a larger NaN-filled buffer, GUARD floats on each side."""

    def __init__(self, shape, device):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=device)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)

    def guards_nan(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[-GUARD:]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


class Workspace:
    """A slice of exactly `need` bytes (at least 256: the CPU build asks for 0 and runs on any buffer) at a 256-aligned address inside a
    larger uint8 buffer filled with `fill`."""

    def __init__(self, need, fill, device):
        self.n = max(int(need), 256)
        self.fill = fill
        self.buf = torch.full((self.n + 2 * WS_PAD,), fill, dtype=torch.uint8, device=device)
        self.off = 256 + (-self.buf.data_ptr()) % 256
        assert 256 <= self.off < WS_PAD and (self.buf.data_ptr() + self.off) % 256 == 0

    def ptr(self, shift=0):
        return ctypes.c_void_p(self.buf.data_ptr() + self.off + shift)

    def outside_untouched(self):
        return bool((self.buf[:self.off] == self.fill).all()) and bool((self.buf[self.off + self.n:] == self.fill).all())


def query(lib, device, stream, which, dims, M, L=None):
    """(return code, bytes) of the size query of mms_mlp_grad ("grad") or mms_mlp_grad_rop ("rop")."""
    L = len(dims) - 1 if L is None else L
    cd = (ctypes.c_int32 * len(dims))(*dims)
    n = ctypes.c_int64(-1)
    if which == "grad":
        rc = lib.mms_mlp_grad(device, L, M, cd, *([None] * 8), None, ctypes.byref(n), stream)
    else:
        rc = lib.mms_mlp_grad_rop(device, L, M, cd, *([None] * 11), None, ctypes.byref(n), stream)
    return rc, int(n.value)


def outputs(dims, M, device):
    """name -> Guarded for every output of the two entries."""
    L = len(dims) - 1
    o = {"rmu": Guarded((M, dims[L]), device)}
    for l in range(1, L + 1):
        for k in ("dw_%d", "rdw_%d"):
            o[k % l] = Guarded((dims[l], dims[l - 1]), device)
        for k in ("db_%d", "rdb_%d"):
            o[k % l] = Guarded((dims[l],), device)
        if l < L:
            for k in ("d_%d", "e_%d"):
                o[k % l] = Guarded((M, dims[l]), device)
    return o


def call_grad(lib, device, stream, inp, o, ws, nbytes, save=True, M=None, L=None, shift=0):
    """The raw mms_mlp_grad on the Guarded outputs `o`; returns the return code.  M, L: what is passed in place of the inputs' own."""
    dims = inp["dims"]
    Lr = len(dims) - 1
    Lp = Lr if L is None else L
    cd = (ctypes.c_int32 * (max(Lp, Lr) + 1))(*(list(dims) + [dims[-1]] * (Lp - Lr)))
    n = None if L is None else max(Lp, Lr)           # (pointer arrays of exactly the ABI's lengths unless `layers` is overridden)
    t = lambda k, cnt: _ptrs([o[k % l].t for l in range(1, cnt + 1)], n)
    return lib.mms_mlp_grad(device, Lp, inp["M"] if M is None else M, cd, _p(inp["x"]), _ptrs(inp["h"], n), _ptrs(inp["W"], n), _p(inp["g"]),
                            t("dw_%d", Lr), t("db_%d", Lr), t("d_%d", Lr - 1) if save else None, t("e_%d", Lr - 1) if save else None,
                            ws.ptr(shift), ctypes.byref(ctypes.c_int64(nbytes)), stream)


def call_rop(lib, device, stream, inp, o, ws, nbytes, M=None, L=None, shift=0):
    """The raw mms_mlp_grad_rop on the Guarded outputs `o`, fed with o's d_l and e_l; returns the return code."""
    dims = inp["dims"]
    Lr = len(dims) - 1
    Lp = Lr if L is None else L
    cd = (ctypes.c_int32 * (max(Lp, Lr) + 1))(*(list(dims) + [dims[-1]] * (Lp - Lr)))
    n = None if L is None else max(Lp, Lr)           # (pointer arrays of exactly the ABI's lengths unless `layers` is overridden)
    t = lambda k, cnt: _ptrs([o[k % l].t for l in range(1, cnt + 1)], n)
    return lib.mms_mlp_grad_rop(device, Lp, inp["M"] if M is None else M, cd, _p(inp["x"]), _ptrs(inp["h"], n), _ptrs(inp["W"], n),
                                _ptrs(inp["V"], n), _ptrs(inp["C"], n), _p(inp["g"]), t("d_%d", Lr - 1), t("e_%d", Lr - 1), _p(o["rmu"].t),
                                t("rdw_%d", Lr), t("rdb_%d", Lr), ws.ptr(shift), ctypes.byref(ctypes.c_int64(nbytes)), stream)


def run_abi(lib, device, stream, inp, fill=0x00, save=True):
    """The size queries, then mms_mlp_grad with d_out and e_out, then mms_mlp_grad_rop fed with those (save=False: mms_mlp_grad alone
    with d_out = e_out = NULL).  Every output sits in a NaN-filled buffer with GUARD floats on each side, each workspace is a slice of
    exactly the queried size at a 256-aligned offset inside a larger buffer of `fill` bytes.  Returns {"out": name -> tensor,
    "guards": all guards still NaN, "ws_outside": the bytes outside both slices unchanged, "bytes": (grad, rop) queried sizes}."""
    dims, M = inp["dims"], inp["M"]
    dev = inp["x"].device
    sizes = []
    for which in ("grad", "rop"):
        rc, n = query(lib, device, stream, which, dims, M)
        _lib.check(rc, None, "mms_mlp_%s size query" % which, lib)
        sizes.append(n)
    o = outputs(dims, M, dev)
    wg = Workspace(sizes[0], fill, dev)
    _lib.check(call_grad(lib, device, stream, inp, o, wg, wg.n, save=save), None, "mms_mlp_grad", lib)
    wss = [wg]
    if save:
        wr = Workspace(sizes[1], fill, dev)
        _lib.check(call_rop(lib, device, stream, inp, o, wr, wr.n), None, "mms_mlp_grad_rop", lib)
        wss.append(wr)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    names = [k for k in o if save or k.startswith(("dw_", "db_"))]
    return {"out": {k: o[k].t for k in names}, "guards": all(o[k].guards_nan() for k in o),
            "untouched": all(o[k].all_nan() for k in o if k not in names), "ws_outside": all(w.outside_untouched() for w in wss),
            "bytes": tuple(sizes)}

"""Per-instantiation checks of the exact-fp32 layer kernels (include/mms.h: mms_linear2_act, mms_linear_group_act without the LayerNorm
folds; csrc/policy_kernels.hip: launch_linear_act) -- one check list for both builds: tests/test_linear_act.py runs it on libmms_cpu.so,
tests/test_linear_act_gpu.py on libmms.so.

Every function takes (L, device_index, stream, torch_device) and drives the C ABI through ctypes.  launch_linear_act picks one of
eleven unfolded kernels from the shape and the activation alone; expected_kernel() restates its rule, and the case table below is
built so that every one of them, both branches of the fast kernel's tile map at either tile height, and every path of its software
pipeline (one to four k-slices, an odd and an even number of them, a last slice of one to four 8-k groups) is reached.  No dispatch
override is read or set: with MMS_LINEAR_SMALL_MAX, MMS_LINEAR_TALL_TILES or MMS_LINEAR_GENERIC in the environment the table would not
select what it says (tests/test_linear_act_gpu.py refuses to run then).

Data as in the project's other layer tests: x ~ 2 N(0, 1), w uniform in +- 1 / sqrt(K), b ~ 0.1 N(0, 1), different for every network
of a group.  The truth is act(x w^T + b) in float64 on the same fp32 inputs.  What every case asserts:
  a. per element   |y - truth| <= min((K + 2) u, 5e-7) (sum |x||w| + |b|) + a      u = 2^-24
     (K + 2) u is the ordering-free bound of tests/gru_check.py (each of the K + 1 terms takes part in at most K roundings of partial
     sums, one of the bias and one of its own product), 5e-7 the gate of test_gpu_parity.py::test_linear2_act_kernel for K <= 1028;
     all four activations are 1-Lipschitz, so the pre-activation's error passes through at most unchanged, and a is what evaluating
     the activation may add: 0 for identity and ReLU, 1.2e-7 for ELU (expf(v) - 1: test_split16_layers_error's allowance), TANH_ABS for
     tanh (check_tanh below).  A dropped float4 of k, a skipped bias or a wrong tile moves elements by about 1 / K of the scale.
  b. y_g is rows 1 .. M of an [M + 2, N] block of NaN: rows 0 and M + 1 are still NaN afterwards, every element inside is finite.
  c. x_g, w_g and b_g each start 16-byte aligned inside a larger allocation of NaN with at least 64 floats of it on either side: a
     read outside a matrix -- the fast kernel's TAIL loads read a clamped address and multiply by zero -- shows as NaN in the output.
  d. two calls of the first case that reaches each kernel are bit-identical (no atomics).
  f. recorded, not gated (parity.record): rms error / rms error of torch's fp32 F.linear + activation on the CPU."""
import ctypes
import functools
import math

import torch

import parity
from massive_marl_benchmark_amd import _lib

U = 2.0 ** -24
NAN = float("nan")
PAD = 64                                    # floats of NaN on either side of every operand
TANH_ABS = 8 * 2.0 ** -23                   # check_tanh's gate, and the tanh allowance of gate a
ACT_ALLOW = {0: 0.0, 1: 1.2e-7, 2: 0.0, 3: TANH_ABS}
ACT64 = {0: lambda v: v, 1: torch.nn.functional.elu, 2: torch.relu, 3: torch.tanh}
ENV_OVERRIDES = ("MMS_LINEAR_SMALL_MAX", "MMS_LINEAR_TALL_TILES", "MMS_LINEAR_GENERIC")


# ---- 1. the launcher's rule ----------------------------------------------------------------------------------------------------
def expected_kernel(G, M, N, K, act):
    """launch_linear_act's choice (no LayerNorm fold, no override in the environment) for G networks of [M, K] x [N, K] and the entry's
    act argument (0..3, + 16: blocked summation): 'fast<tail|full,elu|act,MI=1|2>', 'generic<1>', 'generic<2>' or 'generic<1,blocked>'"""
    grid = math.ceil(N / 128) * math.ceil(M / 128) * G
    small = grid <= 255 and M > 64
    fast = M % (64 if small else 128) == 0 and N % 128 == 0 and K >= 8
    if fast:
        return "fast<%s,%s,MI=%d>" % ("tail" if K % 32 != 0 else "full", "elu" if (act & 15) == 1 else "act", 1 if small else 2)
    if act & 16:
        return "generic<1,blocked>"
    return "generic<1>" if small else "generic<2>"


def expected_tile_map(M, name):
    """the fast kernel's tile map: 'xcd' where the number of row tiles is a multiple of 8, else 'linear'; None for the generic kernels"""
    if not name.startswith("fast"):
        return None
    MI = 2 if name.endswith("MI=2>") else 1
    return "xcd" if (M // (64 * MI)) % 8 == 0 else "linear"


ALL_KERNELS = frozenset(["fast<%s,%s,MI=%d>" % (t, e, mi) for t in ("tail", "full") for e in ("elu", "act") for mi in (1, 2)]
                        + ["generic<1>", "generic<2>", "generic<1,blocked>"])

# ---- 2. the case table ---------------------------------------------------------------------------------------------------------
# one, two, three and four k-slices (and 388: thirteen); the tail list ends in 1..4 eight-k groups at one slice (8, 12 / 20 / 28) and
# at two (36 / 44 / 52 / 60), and in one group at three (68), four (100) and thirteen (388) slices
KS = (32, 64, 96, 128) + (8, 12, 20, 28, 36, 44, 52, 60, 68, 100, 388)


def _every_k(G, M, N):
    """ELU at every K, and a second activation rotating through identity, ReLU and tanh (each meets a K with and one without a tail)"""
    return [(G, M, N, K, (1, (0, 2, 3)[i % 3])) for i, K in enumerate(KS)]


ALL_ACTS = (0, 1, 2, 3)
CASES = (_every_k(2, 192, 256)                        # fast MI = 1: three 64-row tiles, linear tile map
         + _every_k(32, 256, 512)                     # fast MI = 2: 256 blocks, one over the small-grid limit; 32 networks (blockIdx.x / per_net)
         + [(1, 512, 384, K, (1, 0)) for K in (64, 36)]          # XCD tile map at MI = 1: 8 row tiles, 3 column tiles
         + [(11, 1024, 384, K, (1, 0)) for K in (64, 36)]        # ... at MI = 2: 264 blocks, 8 row tiles, 3 column tiles
         + [(1, 1, 1, 4, ALL_ACTS),                              # generic<2>: a single element
            (3, 64, 129, 36, ALL_ACTS),                          #   M not above 64
            (32, 257, 300, 68, ALL_ACTS),                        #   288 blocks, ragged M and N, three slices
            (32, 256, 512, 4, ALL_ACTS)]                         #   K below the fast kernel's minimum of 8
         + [(2, 65, 127, K, ALL_ACTS) for K in (4, 36, 64, 100)]  # generic<1>: small grid, ragged
         + [(1, 300, 200, 1028, ALL_ACTS),                       #   small grid, long K
            (1, 128, 128, 4, ALL_ACTS),                          #   K below the fast minimum
            (3, 130, 100, 68, (16, 18, 19))])                    # generic<1,blocked>: identity, ReLU, tanh (ELU: gru_check.check_linear_blocked)
BLOCKED_FAST = (2, 192, 256, 100)                    # act = 17 at a fast shape: the bits of act = 1

# mms_linear2_act, (problems, M, N, K, act): every kernel it can reach (its act is 0..3: no blocked summation) with one and with two
# problems.  128-row tiles need more than 255 blocks: 16 x 16 for one problem, 2 x 8 x 16 for two.
LINEAR2_CASES = ([(n, 192, 256, K, act) for (K, act) in ((64, 1), (36, 1), (64, 2), (36, 3)) for n in (1, 2)]
                 + [(n, 2048 // n, 2048, K, act) for (K, act) in ((64, 1), (36, 1), (64, 3), (36, 2)) for n in (1, 2)]
                 + [(n, M, N, K, act) for (M, N, K, act) in ((1, 1, 4, 0), (64, 129, 36, 2), (65, 127, 36, 3)) for n in (1, 2)])
LINEAR2_SHARED_X = (2, 192, 256, 36, 1)             # this one with x0 == x1 (include/mms.h allows it: the first layer)
BUILDS_AGREE_CASES = ((2, 192, 256, 100, (1, 2)), (32, 256, 512, 68, (1, 3)), (32, 257, 300, 68, ALL_ACTS))


def _first_of_each_kernel():
    seen, first = set(), set()
    for (G, M, N, K, acts) in CASES:
        for act in acts:
            name = expected_kernel(G, M, N, K, act)
            if name not in seen:
                seen.add(name)
                first.add((G, M, N, K, act))
    return frozenset(first)


TWICE = _first_of_each_kernel()


def coverage():
    """What the tables reach by the launcher's rule: (kernels of CASES, {MI: tile maps} of CASES, kernels of LINEAR2_CASES with one
    problem, ... with two)"""
    names, maps, lin = set(), {1: set(), 2: set()}, {1: set(), 2: set()}
    for (G, M, N, K, acts) in CASES:
        for act in acts:
            name = expected_kernel(G, M, N, K, act)
            names.add(name)
            if name.startswith("fast"):
                maps[2 if name.endswith("MI=2>") else 1].add(expected_tile_map(M, name))
    for (n, M, N, K, act) in LINEAR2_CASES:
        lin[n].add(expected_kernel(n, M, N, K, act))
    return names, maps, lin[1], lin[2]


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _sync(tdev):
    if torch.device(tdev).type == "cuda":
        torch.cuda.synchronize()


def _where(tdev):
    return "gpu" if torch.device(tdev).type == "cuda" else "cpu"


def _ptrs(addrs):
    return (ctypes.c_void_p * len(addrs))(*addrs)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rms(t):
    return float(t.pow(2).mean().sqrt())


def _guarded(val, tdev):
    """val inside a flat allocation of NaN with at least PAD floats of it on either side, starting 16-byte aligned: (allocation, address)"""
    n = val.numel()
    buf = torch.full((n + 2 * PAD + 4,), NAN, device=tdev)
    assert buf.data_ptr() % 4 == 0
    off = PAD + (-(buf.data_ptr() // 4 + PAD)) % 4
    buf[off:off + n].copy_(val.reshape(-1))
    addr = buf.data_ptr() + 4 * off
    assert addr % 16 == 0 and off >= PAD and buf.numel() - off - n >= PAD
    return buf, addr


@functools.lru_cache(maxsize=2)
def problem(G, M, N, K, shared_x=False):
    """Data of G networks and, computed once for every activation, entry and build that use it: the pre-activation in float64, the scale
    sum |x||w| + |b| of gate a, and torch's fp32 F.linear.  shared_x: every network reads network 0's x."""
    g = torch.Generator().manual_seed(1000003 * G + 10007 * M + 101 * N + K)
    x = torch.randn(G, M, K, generator=g) * 2
    if shared_x:
        x[1:] = x[0]
    w = (torch.rand(G, N, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(G, N, generator=g) * 0.1
    xd, wd, bd = x.double(), w.double(), b.double()
    pre = torch.bmm(xd, wd.transpose(1, 2)) + bd[:, None]
    scale = torch.bmm(xd.abs(), wd.abs().transpose(1, 2)) + bd.abs()[:, None]
    yard = torch.stack([torch.nn.functional.linear(x[i], w[i], b[i]) for i in range(G)])
    return dict(G=G, M=M, N=N, K=K, x=x, w=w, b=b, pre=pre, scale=scale, yard=yard, shared_x=shared_x)


def place(P, tdev):
    """the operands of P on tdev, each inside its NaN guards (gate c): {name: [(allocation, address)] * G}"""
    D = {k: [_guarded(P[k][g], tdev) for g in range(P["G"])] for k in ("x", "w", "b")}
    if P.get("shared_x"):
        D["x"] = [D["x"][0]] * P["G"]
    return D


def _dest(P, n, tdev, M=None):
    """n destinations: [M + 2, N] of NaN, y_g = rows 1 .. M"""
    M = P["M"] if M is None else M
    ys = [torch.full((M + 2, P["N"]), NAN, device=tdev) for _ in range(n)]
    return ys, [y.data_ptr() + 4 * P["N"] for y in ys]


def _collect(ys, M, what):
    """gate b, then the rows inside on the CPU"""
    for g, y in enumerate(ys):
        assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[M + 1]).all()), ("a row outside y was written", what, g)
        assert bool(torch.isfinite(y[1:M + 1]).all()), ("non-finite output (an operand's guard read, or an element not written)", what, g)
    return torch.stack([y[1:M + 1] for y in ys]).cpu()


def run_group(L, di, stream, tdev, P, D, act):
    """one mms_linear_group_act call on all networks of P: [G, M, N] on the CPU"""
    G, M, N, K = P["G"], P["M"], P["N"], P["K"]
    ys, ya = _dest(P, G, tdev)
    adr = lambda k: _ptrs([a for _, a in D[k]])
    rc = L.mms_linear_group_act(di, G, M, N, K, adr("x"), adr("w"), adr("b"), _ptrs(ya), act, None, None, None, stream)
    _sync(tdev)
    _lib.check(rc, None, "mms_linear_group_act", L)
    return _collect(ys, M, ("group", G, M, N, K, act))


def run_linear2(L, di, stream, tdev, P, D, act, n):
    """one mms_linear2_act call on the first n (1 or 2) networks of P: [n, M, N] on the CPU"""
    M, N, K = P["M"], P["N"], P["K"]
    ys, ya = _dest(P, n, tdev)
    a = lambda k, g: D[k][g][1] if g < n else None
    rc = L.mms_linear2_act(di, M, N, K, a("x", 0), a("w", 0), a("b", 0), ya[0], a("x", 1), a("w", 1), a("b", 1), ya[1] if n > 1 else None, act, stream)
    _sync(tdev)
    _lib.check(rc, None, "mms_linear2_act", L)
    return _collect(ys, M, ("linear2", n, M, N, K, act))


def judge(tdev, P, out, act, label, n=None):
    """Gate a on `out` (the first n networks of P), and the torch ratio recorded.  Returns the per-element bound."""
    n = P["G"] if n is None else n
    K, code = P["K"], act & 15
    truth = ACT64[code](P["pre"][:n])
    bound = min((K + 2) * U, 5e-7) * P["scale"][:n] + ACT_ALLOW[code]
    err = (out.double() - truth).abs()
    worst = float((err / bound).max())
    yerr = (ACT64[code](P["yard"][:n]).double() - truth).abs()
    e, ye = _rms(err), _rms(yerr)
    ratio = e / ye if ye > 0 else (0.0 if e == 0 else float("inf"))
    print("%s/linear_act_%s: elem_over_bound %.3g, rms %.3g, rms_torch %.3g, rms_over_torch %.3g, max_err %.3g" % (_where(tdev), label, worst, e, ye, ratio, float(err.max())))
    parity.record("%s/linear_act_%s" % (_where(tdev), label), elem_over_bound=worst, rms=e, rms_torch=ye, rms_over_torch=ratio, max_err=float(err.max()))
    assert worst <= 1.0, ("per-element bound", label, worst)
    return bound


# ---- 3. the cases ---------------------------------------------------------------------------------------------------------------
def check_case(L, di, stream, tdev, G, M, N, K, acts):
    """One row of CASES through mms_linear_group_act: gates a, b, c of the module docstring per activation, gate d where this row is
    the first to reach a kernel.  Returns {act: (y, bound)} for the comparison of the two builds."""
    P = problem(G, M, N, K)
    D = place(P, tdev)
    res = {}
    for act in acts:
        name = expected_kernel(G, M, N, K, act)
        print("G %d, M %d, N %d, K %d, act %d -> %s%s" % (G, M, N, K, act, name, ", tile map " + expected_tile_map(M, name) if name.startswith("fast") else ""))
        out = run_group(L, di, stream, tdev, P, D, act)
        if (G, M, N, K, act) in TWICE:
            assert torch.equal(_bits(run_group(L, di, stream, tdev, P, D, act)), _bits(out)), ("two calls differ", name)
        res[act] = (out, judge(tdev, P, out, act, "G%d_M%d_N%d_K%d_act%d" % (G, M, N, K, act)))
    return res


def check_linear2(L, di, stream, tdev, n, M, N, K, act):
    """One row of LINEAR2_CASES through mms_linear2_act with n problems: gates a, b, c; two calls bit-identical; the same data through
    mms_linear_group_act gives the same kernel the same arguments, so the same bits, in the HIP build (the CPU build's two entries
    sum in different orders: both are held to gate a)."""
    shared = (n, M, N, K, act) == LINEAR2_SHARED_X
    P = problem(2, M, N, K, shared)
    D = place(P, tdev)
    if shared:
        assert D["x"][0][1] == D["x"][1][1]
    name = expected_kernel(n, M, N, K, act)
    print("linear2 with %d problem%s, M %d, N %d, K %d, act %d%s -> %s" % (n, "s" if n > 1 else "", M, N, K, act, ", x0 == x1" if shared else "", name))
    out = run_linear2(L, di, stream, tdev, P, D, act, n)
    assert torch.equal(_bits(run_linear2(L, di, stream, tdev, P, D, act, n)), _bits(out)), ("two calls differ", name)
    judge(tdev, P, out, act, "linear2_%d_M%d_N%d_K%d_act%d" % (n, M, N, K, act), n)
    if n == 2:
        grp = run_group(L, di, stream, tdev, P, D, act)
        if _where(tdev) == "gpu":
            assert torch.equal(_bits(grp), _bits(out)), ("the two entries differ on the same arguments", name)
        judge(tdev, P, grp, act, "group2_M%d_N%d_K%d_act%d" % (M, N, K, act))


def check_linear2_has_no_blocked(L, di, stream, tdev):
    """mms_linear2_act takes act 0..3 only: 16 + act is refused and nothing is written (generic<1,blocked> is reached through
    mms_linear_group_act alone)"""
    P = problem(2, 65, 127, 36)
    D = place(P, tdev)
    ys, ya = _dest(P, 1, tdev)
    rc = L.mms_linear2_act(di, 65, 127, 36, D["x"][0][1], D["w"][0][1], D["b"][0][1], ya[0], None, None, None, None, 17, stream)
    _sync(tdev)
    assert rc != 0 and "mms_linear2_act" in _lib.last_error(None, L)
    assert bool(torch.isnan(ys[0]).all())


def check_blocked_flag_ignored_on_fast_path(L, di, stream, tdev):
    """act = 17 at a shape that takes a fast kernel: the bits of act = 1 (include/mms.h: the tiled fast paths are what they are without it)"""
    G, M, N, K = BLOCKED_FAST
    assert expected_kernel(G, M, N, K, 17) == expected_kernel(G, M, N, K, 1) == "fast<tail,elu,MI=1>"
    P = problem(G, M, N, K)
    D = place(P, tdev)
    plain, blocked = run_group(L, di, stream, tdev, P, D, 1), run_group(L, di, stream, tdev, P, D, 17)
    assert torch.equal(_bits(plain), _bits(blocked))
    judge(tdev, P, blocked, 17, "G%d_M%d_N%d_K%d_act17" % BLOCKED_FAST)


def check_empty(L, di, stream, tdev):
    """gate e: M == 0 returns 0 and leaves a poisoned y as it was, through both entries"""
    P = problem(2, 65, 127, 36)
    D = place(P, tdev)
    ys, ya = _dest(P, 2, tdev, M=0)
    adr = lambda k: _ptrs([a for _, a in D[k]])
    rcs = [L.mms_linear_group_act(di, 2, 0, 127, 36, adr("x"), adr("w"), adr("b"), _ptrs(ya), 1, None, None, None, stream),
           L.mms_linear2_act(di, 0, 127, 36, D["x"][0][1], D["w"][0][1], D["b"][0][1], ya[0], D["x"][1][1], D["w"][1][1], D["b"][1][1], ya[1], 1, stream),
           L.mms_linear2_act(di, 0, 127, 36, D["x"][0][1], D["w"][0][1], D["b"][0][1], ya[0], None, None, None, None, 3, stream)]
    _sync(tdev)
    assert rcs == [0, 0, 0], (rcs, _lib.last_error(None, L))
    assert all(bool(torch.isnan(y).all()) for y in ys), "an empty call wrote"


# ---- 4. tanh by itself -----------------------------------------------------------------------------------------------------------
TANH_ROWS = 16384
TANH_SHAPES = ((1, 4), (128, 8))            # (N, K): generic<1>; fast<tail,act,MI=1> (the fast kernels need K >= 8), XCD tile map


def tanh_sweep():
    """16384 pre-activations: 12286 evenly over [-12, 12], 2047 log-spaced magnitudes in [1e-8, 1] with either sign, +-50, +-0"""
    dense = torch.linspace(-12.0, 12.0, 12286, dtype=torch.float64)
    mag = torch.logspace(-8.0, 0.0, 2047, dtype=torch.float64)
    v = torch.cat([dense, mag, -mag, torch.tensor([50.0, -50.0, 0.0, -0.0], dtype=torch.float64)]).float()
    assert v.numel() == TANH_ROWS
    return v


def check_tanh(L, di, stream, tdev):
    """The epilogue's tanh (act = 3) alone: x = (v, 0, ..), w = (1, 0, ..), b = 0, so that the pre-activation IS v, through one generic
    and one fast kernel, against float64 tanh(v).  Gate: absolute error <= 8 * 2^-23 = 9.6e-7 for every v of tanh_sweep().

    Where it comes from (u = 2^-24; csrc/layer_common.h evaluates sign(v) (1 - t) / (1 + t), t = __expf(-2 |v|) in (0, 1]; the CPU build
    calls tanhf): a relative error r of t moves the quotient by 2 t / (1 + t)^2 r = sech^2(v) r / 2.  t carries at most 2 ulp = 4u from
    the exponential itself and |2 v| u from the rounding of its scaled argument: sech^2(v) (4u + 2 |v| u) / 2 <= 2.5u (|v| sech^2(v) <=
    0.45).  1 - t is exact for t >= 1/2 and rounds once below, 1 + t rounds once (u of the quotient each, which is <= 1), and the
    division is good to 2.5 ulp = 5u of the quotient if the build relaxes it.  In all <= 9.5u to first order at the very worst, and
    <= 2.5u near v = 0, where every term but the exponential's scales with the result -- inside 32u = 8 * 2^-23 with room for the
    second-order terms, while a wrong constant or a dropped term shows as 1e-3 and more.  (Until tests/test_split16_paths_gpu.py the
    form was 1 - 2 / (E + 1), E = __expf(2 v): rounded twice at magnitude 1 whatever |v|, 1.7 x 2^-23 measured -- inside this gate,
    outside the layers' per-element bound in rows of tiny activations.)
    Saturation: v = +-50 gives exactly +-1 (t underflows to 0).  Returns the worst absolute error."""
    v = tanh_sweep()
    truth = torch.tanh(v.double())
    worst = {}
    for (N, K) in TANH_SHAPES:
        x = torch.zeros(1, TANH_ROWS, K)
        x[0, :, 0] = v
        w = torch.zeros(1, N, K)
        w[0, :, 0] = 1.0
        P = dict(G=1, M=TANH_ROWS, N=N, K=K, x=x, w=w, b=torch.zeros(1, N))
        name = expected_kernel(1, TANH_ROWS, N, K, 3)
        out = run_group(L, di, stream, tdev, P, place(P, tdev), 3)[0]
        err = (out.double() - truth[:, None]).abs()
        at = int(err.max(1).values.argmax())
        worst[name] = float(err.max())
        print("%s/linear_act_tanh N %d, K %d -> %s: worst absolute error %.3g (%.2f x 2^-23) at v = %.9g, gate %.3g"
              % (_where(tdev), N, K, name, worst[name], worst[name] * 2.0 ** 23, float(v[at]), TANH_ABS))
        sat = out[v.abs() == 50.0]
        assert torch.equal(sat, torch.tensor([[1.0], [-1.0]]).expand(2, N)), ("saturation", name, sat[:, 0])
    parity.record("%s/linear_act_tanh" % _where(tdev), gate=TANH_ABS, **{"worst_abs_err_" + k: e for k, e in worst.items()})
    assert set(worst) == {"generic<1>", "fast<tail,act,MI=1>"}
    assert max(worst.values()) <= TANH_ABS, ("tanh: absolute error above 8 * 2^-23", worst)
    return max(worst.values())


# ---- 5. the two builds ------------------------------------------------------------------------------------------------------------
def builds_agree(gpu, cpu):
    """{act: (y, bound)} of check_case from both builds on the same data: each lies within its bound of the truth, so they differ by at
    most the sum of the two bounds (tests/gru_check.py: builds_agree).  Returns the worst difference / that sum."""
    worst = 0.0
    for act in gpu:
        (a, ba), (b, bb) = gpu[act], cpu[act]
        worst = max(worst, float(((a.double() - b.double()).abs() / (ba + bb)).max()))
    assert worst <= 1.0, worst
    return worst

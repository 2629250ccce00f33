"""Per-entry checks of the grouped MAPPO / HAPPO inference kernels (include/mms.h: mms_row_stats_group, mms_row_stats_chan_group,
mms_row_moments_group, mms_layernorm_group, mms_marl_heads_act, mms_marl_heads_finish and the LayerNorm-fold forms of
mms_linear_group_act, mms_linear_group_act_split, mms_linear_group_act_split16) -- one check list for both builds:
tests/test_marl_kernels.py runs it on libmms_cpu.so, tests/test_marl_kernels_gpu.py on libmms.so.

Every function takes (L, device_index, stream, torch_device) and drives the C ABI through ctypes.  References are float64 torch of
the same operation on the same fp32 inputs; every tolerance is derived in the docstring of the check that uses it (u = 2^-24, the
unit roundoff of fp32).  Every output buffer is filled with NaN (0xFF bytes for operand planes) before the launch and has one guard
row behind it, which must still be poison afterwards.  Shapes alone select the kernels: no dispatch override is read or set.
Each check prints and records (parity.record) its worst observed error / bound."""
import ctypes
import math

import torch

import parity
from massive_marl_benchmark_amd import _lib

EPS = 1e-5
U = 2.0 ** -24
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
HEAD_DIMS = (1, 3, 4, 5, 8, 16)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _ptrs(ts):
    """HOST array of device pointers (None entries: NULL); None: a NULL array"""
    if ts is None:
        return None
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _i32(v):
    return None if v is None else (ctypes.c_int32 * len(v))(*v)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def _sync(tdev):
    if torch.device(tdev).type == "cuda":
        torch.cuda.synchronize()


def _ok(L, rc, what):
    _lib.check(rc, None, what, L)


def _poison(rows, cols, tdev):
    """[rows + 1, cols] of NaN: the output and its guard row"""
    return torch.full((rows + 1, cols), float("nan"), device=tdev)


def _guard_intact(buf, rows):
    return bool(torch.isnan(buf[rows:]).all())


def _where(tdev):
    return "gpu" if torch.device(tdev).type == "cuda" else "cpu"


def _report(tdev, name, **ratios):
    """observed error / bound per quantity (all must be <= 1)"""
    print("%s/marl_kernels_%s: %s" % (_where(tdev), name, ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    parity.record("%s/marl_kernels_%s" % (_where(tdev), name), **ratios)


def _ratio(err, tol):
    """largest err / tol (0 where both are 0); inf if any error or tolerance is not finite -- a NaN (an output still poisoned, or
    computed from one) never passes a gate"""
    if not (bool(torch.isfinite(err).all()) and bool(torch.isfinite(tol).all())):
        return float("inf")
    r = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def _ln64(x64, eps=EPS):
    """nn.LayerNorm's statistics in float64: mean, biased variance, 1 / sqrt(var + eps)"""
    mean = x64.mean(-1)
    var = ((x64 - mean[..., None]) ** 2).mean(-1)
    return mean, var, (var + eps).rsqrt()


# ---- 1. row statistics from synthetic partials ------------------------------------------------------------------------------------
def _stats_data(M, slots, seed, mean=None, std=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, M, slots, 64, generator=g, dtype=torch.float64)
    for gi in range(3):                                                    # different data per group
        x[gi] = x[gi] * ((0.5 + gi) if std is None else std) + ((0.3 * gi) if mean is None else mean)
    return x


def _stats_partials(x, chan):
    """[3][slots, M, 2] fp32: (sum, M2 about the slot's own mean) or (sum, sum of squares), formed in float64 and rounded once"""
    second = ((x - x.mean(-1, keepdim=True)) ** 2).sum(-1) if chan else (x ** 2).sum(-1)
    return torch.stack([x.sum(-1), second], -1).permute(0, 2, 1, 3).float().contiguous()


def row_stats_run(L, di, stream, tdev, chan, part):
    """the entry on partials [3, slots, M, 2]: (mean, rstd) as [3, M, 2] float64 on the CPU"""
    G, slots, M, _ = part.shape
    pd = [part[g].to(tdev) for g in range(G)]
    stat = [_poison(M, 2, tdev) for _ in range(G)]
    if chan:
        _ok(L, L.mms_row_stats_chan_group(di, G, M, slots, _ptrs(pd), _ptrs(stat), EPS, stream), "mms_row_stats_chan_group")
    else:
        _ok(L, L.mms_row_stats_group(di, G, M, slots, 64 * slots, _ptrs(pd), _ptrs(stat), EPS, stream), "mms_row_stats_group")
    _sync(tdev)
    assert all(_guard_intact(s, M) for s in stat), "guard row written"
    return torch.stack([s[:M] for s in stat]).cpu().double()


def row_stats_bounds(x, part, chan):
    """(mean64, rstd64, mean tolerance, relative rstd tolerance), each [3, M]"""
    G, M, slots, _ = x.shape
    flat = x.reshape(G, M, -1)
    mean64, var64, rstd64 = _ln64(flat)
    mean_tol = (slots + 2) * U * part[..., 0].double().abs().sum(1) / (64.0 * slots)
    if chan:
        rel = torch.full_like(mean64, (slots + 4) * 2.0 ** -23)
    else:
        rel = 1.5 * (slots + 2) * U * (flat ** 2).mean(-1) / (var64 + EPS) + 2.0 ** -23
    return mean64, rstd64, mean_tol, rel


def check_row_stats(L, di, stream, tdev, chan, Ms=(1, 255, 257, 1000), slot_counts=(1, 2, 3, 8, 16, 17, 18, 33)):
    """mms_row_stats_chan_group (chan) / mms_row_stats_group against the float64 statistics (biased variance, eps inside the root) of
    x [M, 64 slots] whose per-slot partials were formed in float64 and rounded to fp32.  groups = 3 with different data per group;
    slots 16 / 17 / 18 straddle the two branches of chan_combine.  Roundings the kernels make, u = 2^-24 each:
      mean: one per partial sum on input, slots - 1 additions, the division by the width (a reciprocal and a product in one build):
        slots + 2 roundings of numbers bounded by sum_k |sum_k|, over the width: (slots + 2) u sum_k |sum_k| / (64 slots).
      Chan rstd: M2 = sum_k (m2_k + 64 d_k^2) is a sum of non-negative terms (no cancellation): slots + 3 roundings on it plus the
        mean's own, then the division, the root and the reciprocal; d rstd / rstd = d M2 / (2 M2): (slots + 4) 2^-23 covers them.
      mms_row_stats_group rstd: var = E[x^2] - mean^2 CANCELS: (slots + 2) u E[x^2] on the first term and 2 (slots + 2) u mean^2 <=
        2 (slots + 2) u E[x^2] on the second, halved by the root and relative to var + eps: 1.5 (slots + 2) u E[x^2] / (var + eps),
        + 2^-23 for the root and the reciprocal."""
    worst_m = worst_r = 0.0
    out = {}
    for M in Ms:
        for slots in slot_counts:
            x = _stats_data(M, slots, seed=1000 * M + slots)
            part = _stats_partials(x, chan)
            got = row_stats_run(L, di, stream, tdev, chan, part)
            mean64, rstd64, mean_tol, rel = row_stats_bounds(x, part, chan)
            rm = _ratio((got[..., 0] - mean64).abs(), mean_tol)
            rr = _ratio((got[..., 1] / rstd64 - 1).abs(), rel)
            assert rm <= 1.0 and rr <= 1.0, ("chan" if chan else "plain", M, slots, rm, rr)
            worst_m, worst_r = max(worst_m, rm), max(worst_r, rr)
            out[(M, slots)] = got
    _report(tdev, "row_stats_%s" % ("chan" if chan else "plain"), mean=worst_m, rstd=worst_r)
    return out


def _chan_f32(part):
    """the Chan combination of partials [slots, M, 2] in numpy float32 on the CPU, operation by operation as include/mms.h states it"""
    import numpy as np
    p = part.numpy()
    slots, M, _ = p.shape
    f = np.float32
    total = np.zeros(M, f)
    for k in range(slots):
        total = total + p[k, :, 0]
    width = f(64.0) * f(slots)
    mean = total / width
    m2 = np.zeros(M, f)
    for k in range(slots):
        d = p[k, :, 0] * f(1.0 / 64.0) - mean
        m2 = m2 + (p[k, :, 1] + f(64.0) * d * d)
    rstd = f(1.0) / np.sqrt(m2 / width + f(EPS))
    return torch.from_numpy(np.stack([mean, rstd], -1)).double()


def check_chan_large_mean(L, di, stream, tdev, M=257, slot_counts=(8, 17)):
    """Rows of mean 10 and standard deviation 1e-2 (|mean| / std = 1000: E[x^2] - mean^2 would lose every digit) through
    mms_row_stats_chan_group.  The reference for the size of the error is the same Chan combination in numpy float32 on the CPU:
    err_kernel <= 2 err_numpy_f32 + 2^-22, both against float64 (mean: relative to |mean|; rstd: relative), worst row of all groups."""
    res = {}
    for slots in slot_counts:
        x = _stats_data(M, slots, seed=77 + slots, mean=10.0, std=1e-2)
        part = _stats_partials(x, True)
        got = row_stats_run(L, di, stream, tdev, True, part)
        ref32 = torch.stack([_chan_f32(part[g]) for g in range(3)])
        mean64, _, rstd64 = _ln64(x.reshape(3, M, -1))
        rel = lambda s: (((s[..., 0] - mean64).abs() / mean64.abs()).max().item(), ((s[..., 1] / rstd64 - 1).abs()).max().item())
        (km, kr), (nm, nr) = rel(got), rel(ref32)
        print("chan, mean 10 std 1e-2, slots %d: kernel mean %.3g rstd %.3g; numpy float32 mean %.3g rstd %.3g" % (slots, km, kr, nm, nr))
        assert km <= 2 * nm + 2.0 ** -22 and kr <= 2 * nr + 2.0 ** -22, (slots, km, nm, kr, nr)
        res["mean_kernel_s%d" % slots], res["mean_numpy_f32_s%d" % slots] = km, nm
        res["rstd_kernel_s%d" % slots], res["rstd_numpy_f32_s%d" % slots] = kr, nr
    parity.record("%s/marl_kernels_row_stats_chan_large_mean" % _where(tdev), **res)
    return res


# ---- 2. mms_row_moments_group and mms_layernorm_group ------------------------------------------------------------------------------
def _ln_data(M, K, seed):
    """block [2][M, 3, K] (the rows under test are agent 1's), gamma, beta [2][K].  From M = 5 on, row 1 is the constant 0.75 (its sums
    are exact in fp32: var = 0, rstd = eps^-1/2 on both builds) and row 2 is scaled by 2^20."""
    g = torch.Generator().manual_seed(seed)
    block = [torch.randn(M, 3, K, generator=g) * (1.0 + gi) + 0.5 * gi for gi in range(2)]
    if M >= 5:
        for b in block:
            b[1] = 0.75
            b[2] *= 2.0 ** 20
    gamma = [1.0 + 0.3 * torch.randn(K, generator=g) for _ in range(2)]
    beta = [0.2 * torch.randn(K, generator=g) for _ in range(2)]
    return block, gamma, beta


def ln_bounds(x64, gamma64, beta64, K, eps=EPS):
    """float64 LayerNorm of rows x64 [M, K] and the tolerances of section 2: (mean, var, rstd, y, mean_tol [M], y_tol [M, K])"""
    mean, var, rstd = _ln64(x64, eps)
    xhat = (x64 - mean[:, None]) * rstd[:, None]
    y = xhat * gamma64 + beta64
    mean_tol = (K / 64.0 + 8) * U * x64.abs().amax(-1)
    y_tol = 2.0 ** -22 * (xhat.abs() * gamma64.abs() + beta64.abs()) + (1e-5 * xhat.abs() + (mean_tol * rstd)[:, None]) * gamma64.abs()
    return mean, var, rstd, y, mean_tol, y_tol


def check_layernorm(L, di, stream, tdev, K, Ms=(1, 5, 130)):
    """mms_row_moments_group and mms_layernorm_group at row width K, groups = 2, against float64, in every layout: x_pitch = K; x_pitch
    = 3 K (agent 1's rows of an [M, 3, K] block, the base pointer K floats in: rows not 16-byte aligned for the odd widths); Kp = K and
    Kp = K rounded up to 4 (columns K..Kp exactly 0); in place.  One row of the constant 0.75 (var = 0) and one scaled by 2^20.
      mean: a row is summed as 64 lane chains of K / 64 terms and a six-level butterfly, then divided: (K / 64 + 8) u max|x|.
      rstd: |rstd sqrt(var64 + eps) - 1| <= 1e-5, the project's gate for LayerNorm statistics (test_split16_planes).
      output y = (x - mean) rstd gamma + beta: four roundings, 2^-22 (|xhat| |gamma| + |beta|), plus what the statistics carry in:
        1e-5 |xhat| |gamma| from rstd and mean_tol rstd |gamma| from the mean."""
    worst = dict(mean=0.0, rstd=0.0, y=0.0)
    out = {}
    Kp4 = (K + 3) & ~3
    # The constant row is inside the gates on both builds.  On the CPU build it is also exact (0.75 k is exact in fp32 and the division
    # is IEEE's: mean = 0.75, y = beta); the device divides by v_rcp and a product, which may leave the mean one ulp off 0.75.
    exact = torch.device(tdev).type == "cpu"
    for M in Ms:
        block, gamma, beta = _ln_data(M, K, seed=31 * K + M)
        bd = [b.to(tdev) for b in block]
        xc = [b[:, 1, :].contiguous() for b in bd]
        gd, btd = [t.to(tdev) for t in gamma], [t.to(tdev) for t in beta]
        ref = [ln_bounds(xc[g].double(), gd[g].double(), btd[g].double(), K) for g in range(2)]
        layouts = {"pitch K": (xc, K, None), "pitch 3K": (bd, 3 * K, 4 * K)}

        def src(name):
            ts, pitch, off = layouts[name]
            arr = _ptrs(ts) if off is None else (ctypes.c_void_p * 2)(*[t.data_ptr() + off for t in ts])
            return arr, pitch

        for name in layouts:
            arr, pitch = src(name)
            stat = [_poison(M, 2, tdev) for _ in range(2)]
            _ok(L, L.mms_row_moments_group(di, 2, M, K, pitch, arr, _ptrs(stat), EPS, stream), "mms_row_moments_group")
            _sync(tdev)
            for g in range(2):
                mean, var, rstd, _, mean_tol, _ = ref[g]
                assert _guard_intact(stat[g], M), (K, M, name)
                rm = _ratio((stat[g][:M, 0].double() - mean).abs(), mean_tol)
                rr = float((stat[g][:M, 1].double() * (var + EPS).sqrt() - 1).abs().max()) / 1e-5
                assert rm <= 1.0 and rr <= 1.0, ("moments", K, M, name, g, rm, rr)
                if M >= 5 and exact:
                    assert float(stat[g][1, 0]) == 0.75 and abs(float(stat[g][1, 1]) * EPS ** 0.5 - 1) <= 2.0 ** -22, (K, M, name)
                worst["mean"], worst["rstd"] = max(worst["mean"], rm), max(worst["rstd"], rr)
            out[(M, name, "stat")] = [s[:M].cpu() for s in stat]
        forms = [(n, kp) for n in layouts for kp in sorted({K, Kp4})] + [("in place", K)]
        for name, Kp in forms:
            if name == "in place":
                y = [_poison(M, K, tdev) for _ in range(2)]
                for g in range(2):
                    y[g][:M] = xc[g]
                arr, pitch = _ptrs(y), K
            else:
                y = [_poison(M, Kp, tdev) for _ in range(2)]
                arr, pitch = src(name)
            _ok(L, L.mms_layernorm_group(di, 2, M, K, Kp, pitch, arr, _ptrs(gd), _ptrs(btd), _ptrs(y), EPS, stream), "mms_layernorm_group")
            _sync(tdev)
            for g in range(2):
                _, _, _, y64, _, y_tol = ref[g]
                assert _guard_intact(y[g], M), (K, M, name, Kp)
                assert bool((y[g][:M, K:] == 0).all()), ("padding columns", K, M, name, Kp)
                ry = _ratio((y[g][:M, :K].double() - y64).abs(), y_tol)
                assert ry <= 1.0, ("layernorm", K, M, name, Kp, g, ry)
                if M >= 5 and exact:
                    assert torch.equal(y[g][1, :K], btd[g]), "the constant row must come out as beta"
                worst["y"] = max(worst["y"], ry)
            out[(M, name, Kp)] = [t[:M].cpu() for t in y]
    _report(tdev, "layernorm_K%d" % K, **worst)
    return out


# ---- 3. mms_marl_heads_act ---------------------------------------------------------------------------------------------------------
def heads_data(H, M, A, seed, tdev):
    """h [M, H], gamma, beta [H], w [A_g, H], b [A_g], std [A_g] in [0.1, 0.5] per group; the means stay well inside |mean| <= 1"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g)
    G = len(A)
    d = dict(H=H, A=list(A), h=[r(M, H) * (0.5 + 0.25 * (i % 4)) + 0.2 * (i % 3) for i in range(G)], gamma=[1.0 + 0.3 * r(H) for _ in range(G)],
             beta=[0.2 * r(H) for _ in range(G)], w=[0.2 * r(a, H) / H ** 0.5 for a in A], b=[0.1 * r(a) for a in A],
             std=[0.1 + 0.4 * torch.rand(a, generator=g) for a in A])
    return {k: ([t.to(tdev) for t in v] if k not in ("H", "A") else v) for k, v in d.items()}


def heads_call(L, di, stream, tdev, pr, M, eps, *, std=None, pad=0, counters=None, seed=11, row_offset=0, row0=0, groups=None, want_logp=True):
    """One mms_marl_heads_act call on rows row0 .. row0 + M of the chosen groups; out / logp rows have pitch A + pad, NaN-filled, with a
    guard row.  eps < 0 passes no gamma / beta at all.  Returns (out, logp) lists of the [M + 1, pitch] buffers."""
    gs = list(range(len(pr["A"]))) if groups is None else groups
    A = [pr["A"][g] for g in gs]
    h = [pr["h"][g][row0:row0 + M] for g in gs]
    out = [_poison(M, a + pad, tdev) for a in A]
    logp = [_poison(M, a + pad, tdev) for a in A] if want_logp else None
    ln = eps >= 0
    rc = L.mms_marl_heads_act(di, len(gs), M, pr["H"], _ptrs(h), _ptrs([pr["gamma"][g] for g in gs]) if ln else None,
                              _ptrs([pr["beta"][g] for g in gs]) if ln else None, _ptrs([pr["w"][g] for g in gs]), _ptrs([pr["b"][g] for g in gs]),
                              _i32(A), _ptrs(std), _ptrs(out), _ptrs(logp), _i32([a + pad for a in A]) if pad else None, _ptrs(counters),
                              seed, row_offset, eps, stream)
    _ok(L, rc, "mms_marl_heads_act")
    _sync(tdev)
    for a, o in zip(A, out):
        assert _guard_intact(o, M) and bool(torch.isnan(o[:M, a:]).all()), "guard row or gap columns written"
    return out, logp


def heads_reference(pr, g, M, eps):
    """float64 LayerNorm + Linear of group g and the bound of section 3: (mean64 [M, A], tol, scale)"""
    H = pr["H"]
    h, w, b = pr["h"][g][:M].double(), pr["w"][g].double(), pr["b"][g].double()
    if eps >= 0:
        gm, bt = pr["gamma"][g].double(), pr["beta"][g].double()
        _, _, _, x, _, x_tol = ln_bounds(h, gm, bt, H, eps)
    else:
        x, x_tol = h, torch.zeros_like(h)
    scale = x.abs() @ w.abs().t()
    tol = (H / 64.0 + 8) * U * scale + b.abs() * U + x_tol @ w.abs().t()
    return x @ w.t() + b, tol, scale + b.abs()


def logp_check(out, mean, logp, sd):
    """the per-dimension log-density identity: (worst error / bound, z)"""
    z = (out.double() - mean.double()) / sd.double()
    ref = -0.5 * z * z - sd.double().log() - HALF_LOG_2PI
    tol = 2.0 ** -22 * (1 + z * z) + z.abs() * 2.0 ** -22 * mean.double().abs() / sd.double()
    return _ratio((logp.double() - ref).abs(), tol), z


def check_heads(L, di, stream, tdev, H, M, A=(1, 3, 8, 16), seed=5):
    """mms_marl_heads_act at hidden width H on M rows, the output widths A mixed in one launch, against float64 LayerNorm + Linear
    (eps >= 0) and against float64 Linear (eps < 0, called without gamma / beta).
      mean_j = b_j + sum_k w_jk LN(h)_k: the dot product is 64 lane chains of H / 64 terms and a butterfly:
        (H / 64 + 8) u sum_k |LN(h)_k| |w_jk| + |b_j| u, plus the LayerNorm's own error of section 2 carried through |w_jk|.
    Paths: out_pitch > A (the gap columns stay NaN); std == NULL (the plain output, counters untouched); std[g] == NULL for the odd
    groups only; counters == NULL equals counters of zero, bit for bit; counters of the sampled groups become 1.
    Sampled rows: out = mean + std z, and logp = -0.5 z^2 - log(std) - 0.5 log(2 pi) per dimension with z = (out - mean) / std from the
    stored numbers: z^2 / 2 and log(std) round at 2^-24 of themselves, and the rounding of `out` (2^-24 |out|) moves z by 2^-24 |out| /
    std: 2^-22 (1 + z^2) + |z| 2^-22 |mean| / std, with |mean| <= 1 and std in [0.1, 0.5]."""
    pr = heads_data(H, M, A, seed + 7 * H + M, tdev)
    G = len(A)
    worst = dict(mean=0.0, mean_plain=0.0, logp=0.0)
    res = {}
    for eps in (EPS, -1.0):
        key = "mean" if eps >= 0 else "mean_plain"
        cnt = [torch.full((M,), 5, dtype=torch.int64, device=tdev) for _ in range(G)]
        det, _ = heads_call(L, di, stream, tdev, pr, M, eps, std=None, pad=3, counters=cnt)
        assert all(bool((c == 5).all()) for c in cnt), "std == NULL must leave the counters alone"
        for g in range(G):
            ref, tol, _ = heads_reference(pr, g, M, eps)
            r = _ratio((det[g][:M, :A[g]].double() - ref).abs(), tol)
            assert r <= 1.0, (H, M, eps, g, r)
            worst[key] = max(worst[key], r)
        res[key] = [det[g][:M, :A[g]].cpu() for g in range(G)]
        # std for the even groups only
        std = [pr["std"][g] if g % 2 == 0 else None for g in range(G)]
        cnt = [torch.zeros(M, dtype=torch.int64, device=tdev) for _ in range(G)]
        smp, lp = heads_call(L, di, stream, tdev, pr, M, eps, std=std, pad=3, counters=cnt)
        nocnt, lp0 = heads_call(L, di, stream, tdev, pr, M, eps, std=std, pad=3, counters=None)
        for g in range(G):
            a = A[g]
            assert torch.equal(nocnt[g][:M, :a], smp[g][:M, :a]), "counters == NULL must equal counters of zero"
            if g % 2:
                assert torch.equal(smp[g][:M, :a], det[g][:M, :a]) and bool(torch.isnan(lp[g]).all()) and bool((cnt[g] == 0).all()), g
                continue
            assert torch.equal(lp0[g][:M, :a], lp[g][:M, :a]) and bool((cnt[g] == 1).all()), g
            assert bool(torch.isnan(lp[g][:M, a:]).all()) and _guard_intact(lp[g], M), "logp gap columns or guard row written"
            r, z = logp_check(smp[g][:M, :a], det[g][:M, :a], lp[g][:M, :a], pr["std"][g])
            assert float(z.abs().max()) < 7.0, (H, M, eps, g)
            worst["logp"] = max(worst["logp"], r)
        again, _ = heads_call(L, di, stream, tdev, pr, M, eps, std=std, pad=3, counters=cnt)      # counters now 1: another draw
        assert not torch.equal(again[0][:M, :A[0]], smp[0][:M, :A[0]]) and bool((cnt[0] == 2).all())
    _report(tdev, "heads_H%d_M%d_G%d" % (H, M, G), **worst)
    assert worst["logp"] <= 1.0, ("logp identity", H, M, worst["logp"])         # (last: everything else has been checked by now)
    return res


def check_heads_sampling_exact(L, di, stream, tdev, H=100, M=33, A=(1, 3, 8, 16)):
    """The noise stream is keyed (seed + g, row_offset + r, counter, j), all exact: row r under row_offset o equals row r + o under
    offset 0; group g under `seed` equals group 0 under seed + g; a second call with the advanced counters draws again."""
    pr = heads_data(H, M, A, 99, tdev)
    G = len(A)
    zeros = lambda n: [torch.zeros(n, dtype=torch.int64, device=tdev) for _ in range(G)]
    cnt = zeros(M)
    base, lp = heads_call(L, di, stream, tdev, pr, M, EPS, std=pr["std"], counters=cnt, seed=11)
    o = 5
    part, lpp = heads_call(L, di, stream, tdev, pr, M - o, EPS, std=pr["std"], counters=zeros(M - o), seed=11, row_offset=o, row0=o)
    for g in range(G):
        assert torch.equal(part[g][:M - o], base[g][o:M]) and torch.equal(lpp[g][:M - o], lp[g][o:M]), ("row_offset", g)
        one, lp1 = heads_call(L, di, stream, tdev, pr, M, EPS, std=[pr["std"][g]], counters=[torch.zeros(M, dtype=torch.int64, device=tdev)],
                              seed=11 + g, groups=[g])
        assert torch.equal(one[0][:M], base[g][:M]) and torch.equal(lp1[0][:M], lp[g][:M]), ("seed + g", g)
    second, _ = heads_call(L, di, stream, tdev, pr, M, EPS, std=pr["std"], counters=cnt, seed=11)
    for g in range(G):
        assert not torch.equal(second[g][:M], base[g][:M]) and bool((cnt[g] == 2).all()), g


def check_heads_moments(L, di, stream, tdev, M=4096, A=16, H=64):
    """65 536 draws (M = 4096, A = 16): z = (out - mean) / std has |mean(z)| <= 4 / sqrt(n) and |var(z) - 1| <= 4 sqrt(2 / n) -- four
    standard errors of the sample mean and of the sample variance of a unit normal."""
    pr = heads_data(H, M, (A,), 123, tdev)
    det, _ = heads_call(L, di, stream, tdev, pr, M, EPS, std=None)
    smp, lp = heads_call(L, di, stream, tdev, pr, M, EPS, std=pr["std"], counters=[torch.zeros(M, dtype=torch.int64, device=tdev)])
    r, z = logp_check(smp[0][:M], det[0][:M], lp[0][:M], pr["std"][0])
    n = z.numel()
    m, v = float(z.mean()), float(z.var(unbiased=False))
    _report(tdev, "heads_moments", mean_z=abs(m) / (4 / n ** 0.5), var_z=abs(v - 1) / (4 * (2.0 / n) ** 0.5), logp=r)
    assert n == 65536 and abs(m) <= 4 / n ** 0.5 and abs(v - 1) <= 4 * (2.0 / n) ** 0.5, (m, v)
    assert r <= 1.0, ("logp identity", r)


def check_heads_contract(L, di, stream, tdev):
    """include/mms.h: with eps < 0 mms_marl_heads_act reads no gamma / beta (check_heads calls it without them on both builds); with
    eps >= 0 both are required, and a call without them is refused before anything is written."""
    pr = heads_data(64, 8, (3,), 1, tdev)
    out = _poison(8, 3, tdev)
    for gamma, beta in ((None, _ptrs(pr["beta"])), (_ptrs(pr["gamma"]), None), (_ptrs([None]), _ptrs(pr["beta"]))):
        rc = L.mms_marl_heads_act(di, 1, 8, 64, _ptrs(pr["h"]), gamma, beta, _ptrs(pr["w"]), _ptrs(pr["b"]), _i32([3]), None, _ptrs([out]), None, None, None, 0, 0, EPS, stream)
        assert rc != 0 and _lib.last_error(None, L)
        _sync(tdev)
        assert bool(torch.isnan(out).all())
    rc = L.mms_marl_heads_act(di, 1, 8, 64, _ptrs(pr["h"]), _ptrs([None]), _ptrs([None]), _ptrs(pr["w"]), _ptrs(pr["b"]), _i32([3]), None, _ptrs([out]), None, None, None, 0, 0,
                              -1.0, stream)
    _ok(L, rc, "mms_marl_heads_act without gamma / beta entries, eps < 0")
    _sync(tdev)
    assert not bool(torch.isnan(out[:8]).any()) and _guard_intact(out, 8)


# ---- 4. the folded split layers ----------------------------------------------------------------------------------------------------
def expected_tiling(cus, G, M, N):
    """launch_linear_split16's rule (the same in both split kernels): 256-row tiles (MT = 4) when they give every CU a tile.
    Returns (MT, tiles, persistent blocks)."""
    tiles256 = G * (M // 256) * (N // 128) if M % 256 == 0 else 0
    MT = 4 if tiles256 >= cus else 2
    tiles = G * (M // (64 * MT)) * (N // 128)
    return MT, tiles, min(tiles, cus)


def _plane_bytes(fmt, rows, K):
    return rows * ((K + 31) // 32) * (128 if fmt == "f16x2" else 192)


def fold_operands(L, di, stream, tdev, fmt, G, M, N, K, head_dims, seed):
    """Operands of one folded layer + its output heads, built the way GroupedPolicyInference builds them: mms_fold_planes16_group (W~
    planes, s, c, row bounds; the heads' folded weight, hs, hc), mms_fold_scales16_group (y_scale and its inverse), and the input's
    planes + LayerNorm statistics from mms_split_planes16_group (f16x2) or mms_split_planes_group + mms_row_moments_group (bf16x3, whose
    weight planes are the split of the fold's wt)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g)
    to = lambda ts: [t.to(tdev) for t in ts]
    z = lambda *sh: torch.zeros(*sh, device=tdev)
    f16 = fmt == "f16x2"
    o = dict(fmt=fmt, G=G, M=M, N=N, K=K, A=list(head_dims))
    o["h"] = to([r(M, K) * (0.5 + 0.1 * (i % 5)) + 0.2 * (i % 3) for i in range(G)])
    w, gam, bet, bias = to([r(N, K) / K ** 0.5 for _ in range(G)]), to([1.0 + 0.3 * r(K) for _ in range(G)]), to([0.2 * r(K) for _ in range(G)]), to([0.1 * r(N) for _ in range(G)])
    o["wp"] = [torch.zeros(_plane_bytes(fmt, N, K), dtype=torch.uint8, device=tdev) for _ in range(G)]
    o["winv"], o["s"], o["c"], rb = ([z(N) for _ in range(G)] for _ in range(4))
    o["wt"] = [z(N, K) for _ in range(G)]
    _ok(L, L.mms_fold_planes16_group(di, G, _i64([N] * G), _i32([K] * G), _ptrs(w), _ptrs(gam), _ptrs(bet), _ptrs(bias), _ptrs(o["wp"]) if f16 else None,
                                     _ptrs(o["winv"]) if f16 else None, _ptrs(o["s"]), _ptrs(o["c"]), _ptrs(rb), _ptrs(o["wt"]), stream), "mms_fold_planes16_group")
    o["ysc"], o["yinv"] = [z(M) for _ in range(G)], [z(M) for _ in range(G)]
    _ok(L, L.mms_fold_scales16_group(di, G, _ptrs(rb), _i32([N] * G), M, None, _ptrs(o["ysc"]), _ptrs(o["yinv"]), stream), "mms_fold_scales16_group")
    o["xp"] = [torch.zeros(_plane_bytes(fmt, M, K), dtype=torch.uint8, device=tdev) for _ in range(G)]
    o["stat"] = [z(M, 2) for _ in range(G)]
    o["xinv"] = [z(M) for _ in range(G)]
    if f16:
        xs = [z(M) for _ in range(G)]
        _ok(L, L.mms_split_planes16_group(di, G, M, K, 0, _ptrs(o["h"]), _ptrs(o["xp"]), _ptrs(xs), _ptrs(o["xinv"]), 0, 0, None, None, None, _ptrs(o["stat"]),
                                          EPS, stream), "mms_split_planes16_group")
    else:
        _ok(L, L.mms_split_planes_group(di, G, N, K, 0, _ptrs(o["wt"]), _ptrs(o["wp"]), stream), "mms_split_planes_group")
        _ok(L, L.mms_split_planes_group(di, G, M, K, 0, _ptrs(o["h"]), _ptrs(o["xp"]), stream), "mms_split_planes_group")
        _ok(L, L.mms_row_moments_group(di, G, M, K, 0, _ptrs(o["h"]), _ptrs(o["stat"]), EPS, stream), "mms_row_moments_group")
    hw = to([0.3 * r(a, N) / N ** 0.5 for a in head_dims])
    g2, b2, hb = to([1.0 + 0.3 * r(N) for _ in range(G)]), to([0.2 * r(N) for _ in range(G)]), to([0.1 * r(a) for a in head_dims])
    o["head_w"] = [z(a, N) for a in head_dims]
    o["hs"], o["hc"] = [z(a) for a in head_dims], [z(a) for a in head_dims]
    _ok(L, L.mms_fold_planes16_group(di, G, _i64(list(head_dims)), _i32([N] * G), _ptrs(hw), _ptrs(g2), _ptrs(b2), _ptrs(hb), None, None, _ptrs(o["hs"]), _ptrs(o["hc"]),
                                     None, _ptrs(o["head_w"]), stream), "mms_fold_planes16_group (heads)")
    o["std"] = to([0.1 + 0.4 * torch.rand(a, generator=g) for a in head_dims])
    _sync(tdev)
    return o


def fold_layer(L, di, stream, tdev, o, out_mode):
    """One launch of the folded layer.  out_mode 1: (y planes as bytes with a guard row of 0xFF, ln_part_out [slots + 1, M, 2]);
    out_mode 2: (head_part [slots + 1, M, HS] per group, ln_part_out)."""
    G, M, N, K, fmt = o["G"], o["M"], o["N"], o["K"], o["fmt"]
    slots = N // 64
    part = [_poison(slots, M * 2, tdev) for _ in range(G)]
    y = hp = None
    if out_mode == 1:
        row = _plane_bytes(fmt, 1, N)
        y = [torch.full(((M + 1) * row,), 0xFF, dtype=torch.uint8, device=tdev) for _ in range(G)]
    else:
        hp = [_poison(slots, M * ((a + 3) & ~3), tdev) for a in o["A"]]
    head = (_ptrs(o["head_w"]), _ptrs(hp), _i32(o["A"])) if out_mode == 2 else (None, None, None)
    if fmt == "f16x2":
        rc = L.mms_linear_group_act_split16(di, G, M, N, K, _ptrs(o["xp"]), _ptrs(o["wp"]), _ptrs(o["c"]), _ptrs(y), _ptrs(o["xinv"]), _ptrs(o["winv"]),
                                            _ptrs(o["ysc"]) if out_mode == 1 else None, 1, out_mode, _ptrs(o["s"]), _ptrs(o["stat"]), _ptrs(part), *head, stream)
    else:
        rc = L.mms_linear_group_act_split(di, G, M, N, K, _ptrs(o["xp"]), _ptrs(o["wp"]), _ptrs(o["c"]), _ptrs(y), 1, out_mode, _ptrs(o["s"]), _ptrs(o["stat"]),
                                          _ptrs(part), *head, stream)
    _ok(L, rc, "folded split layer, out_mode %d" % out_mode)
    _sync(tdev)
    assert all(_guard_intact(p, slots) for p in part), "ln_part_out guard written"
    return (y if out_mode == 1 else hp), part


def planes_to_f64(o, g, planes):
    """the activations an out_mode 1 layer left, [M, N] float64 (H32: (hi + lo 2^-11) / y_scale; P32: the three planes' sum)"""
    M, N = o["M"], o["N"]
    body = planes[:M * _plane_bytes(o["fmt"], 1, N)]
    assert bool((planes[body.numel():] == 0xFF).all()), "y guard row written"
    if o["fmt"] == "f16x2":
        v = body.view(torch.float16).view(M, N // 32, 2, 32).double()
        assert float(v[:, :, 0].abs().max()) <= 2.0 ** 14, "an activation's hi plane left the bound"
        return (v[:, :, 0] + v[:, :, 1] / 2048.0).reshape(M, N) * o["yinv"][g].double()[:, None]
    v = body.view(torch.bfloat16).view(M, N // 32, 3, 32).double()
    return v.sum(2).reshape(M, N)


def check_folded_layer(L, di, stream, tdev, fmt, G, M, N, K, head_dims=None, seed=3, label=None):
    """mms_linear_group_act_split16 (fmt "f16x2") / mms_linear_group_act_split ("bf16x3") with the LayerNorm folds, per output.
    Which tiling runs (MT = 2 or 4, one or several tiles per persistent block) is decided by the shape and the device's CU count
    (expected_tiling); the GPU tests choose (M, N) from the CU count and print what they expect.
    out_mode 1, y reconstructed from the planes:
      y against float64 ELU(rstd (W~ h - mean s) + c) on the call's own fp32 (mean, rstd), s, c, W~: within 5e-7 (rstd (|W~||h| +
        |mean||s|) + |c|) + 1.2e-7, test_split16_layers_error's per-element gate carried through the fold (+ 1.2e-7: expf(v) - 1).
      ln_part_out[slot, r] against float64 (sum, M2 about the slot's own mean) of the reconstructed y: the planes keep y to 2^-22 |y|
        and the kernel sums 64 fp32 terms: 64 2^-21 max|y_slot| for the sum, 2 x 64 2^-21 max|y_slot| max|y_slot - mean_slot| for M2
        (d M2 = 2 sum d_n dy_n).  A wrong slot, half or row base misses by the size of y itself.
      mms_row_stats_chan_group on them against the float64 LayerNorm statistics of y: section 1's bounds plus the partials' own
        tolerances carried through the combination: mean: + sum_k tol_sum_k / N; rstd (relative): + (sum_k tol_m2_k + 2 |mean_k - mean|
        tol_sum_k) / (2 N (var + eps)), from M2 = sum_k (m2_k + 64 (sum_k / 64 - mean)^2).  The carried terms are worst cases and leave
        that gate loose, so the same output is ALSO held to section 1's bounds alone against the float64 Chan combination of the fp32
        partials the kernel read.
    out_mode 2, the same operands, head_dims mixed over the groups:
      head_part[slot, r, j] against the float64 dot of the reconstructed y with head_w[j] over the slot: (2^-21 + 64 2^-24) sum_n
        |y_n| |head_w_jn| (the planes' 2^-22 against the kernel's unrounded y, the products and the 64-term sum); the padding columns
        A..HS stay NaN; ln_part_out equals the out_mode 1 run's bit for bit.
      mms_marl_heads_finish (out_pitch = A + 2) against float64 rstd (sum_slots dot - mean hs) + hc evaluated on the fp32 partials it
        reads (their Chan combination in float64): (slots + 4) u (rstd (sum_slots |dot| + |mean| |hs|) + |hc|); sampled: the logp
        identity of section 3, and logp equal to mms_marl_heads_act's bit for bit for equal keys and std."""
    if head_dims is None:
        head_dims = [HEAD_DIMS[(5 * g + g // 6) % 6] for g in range(G)]
    o = fold_operands(L, di, stream, tdev, fmt, G, M, N, K, head_dims, seed)
    slots = N // 64
    yp, part1 = fold_layer(L, di, stream, tdev, o, 1)
    hp, part2 = fold_layer(L, di, stream, tdev, o, 2)
    # the heads' finish: deterministic, then sampled; mms_marl_heads_act on the same keys
    pad = 2
    pitch = _i32([a + pad for a in head_dims])
    raw = lambda ts: [t[:slots] for t in ts]
    det = [_poison(M, a + pad, tdev) for a in head_dims]
    _ok(L, L.mms_marl_heads_finish(di, G, M, slots, _ptrs(raw(part2)), _ptrs(raw(hp)), _ptrs(o["hs"]), _ptrs(o["hc"]), _i32(head_dims), None, _ptrs(det), None, pitch,
                                   None, 11, 3, EPS, stream), "mms_marl_heads_finish")
    smp, lp = [_poison(M, a + pad, tdev) for a in head_dims], [_poison(M, a + pad, tdev) for a in head_dims]
    cnt = [torch.zeros(M, dtype=torch.int64, device=tdev) for _ in range(G)]
    _ok(L, L.mms_marl_heads_finish(di, G, M, slots, _ptrs(raw(part2)), _ptrs(raw(hp)), _ptrs(o["hs"]), _ptrs(o["hc"]), _i32(head_dims), _ptrs(o["std"]), _ptrs(smp),
                                   _ptrs(lp), pitch, _ptrs(cnt), 11, 3, EPS, stream), "mms_marl_heads_finish (sampled)")
    stat = [_poison(M, 2, tdev) for _ in range(G)]
    _ok(L, L.mms_row_stats_chan_group(di, G, M, slots, _ptrs(raw(part1)), _ptrs(stat), EPS, stream), "mms_row_stats_chan_group")
    pr = heads_data(64, M, head_dims, 17, tdev)
    pr["std"] = o["std"]
    _, lp_act = heads_call(L, di, stream, tdev, pr, M, EPS, std=o["std"], pad=pad, counters=[torch.zeros(M, dtype=torch.int64, device=tdev) for _ in range(G)],
                           seed=11, row_offset=3)
    _sync(tdev)
    worst = dict(y=0.0, part_sum=0.0, part_m2=0.0, stat_mean=0.0, stat_rstd=0.0, stat_mean_of_part=0.0, stat_rstd_of_part=0.0, head_part=0.0, finish=0.0, logp=0.0)
    res = dict(y=[], head_part=[], finish=[], y_scale=[], dot_scale=[], finish_scale=[])
    for g in range(G):
        A, HS = head_dims[g], (head_dims[g] + 3) & ~3
        tag = (fmt, G, M, N, K, g)
        y = planes_to_f64(o, g, yp[g])
        h, wt, s, c = o["h"][g].double(), o["wt"][g].double(), o["s"][g].double(), o["c"][g].double()
        mean_in, rstd_in = o["stat"][g][:, 0].double()[:, None], o["stat"][g][:, 1].double()[:, None]
        pre = rstd_in * (h @ wt.t() - mean_in * s) + c
        y64 = torch.where(pre > 0, pre, torch.expm1(pre))
        scale = rstd_in * (h.abs() @ wt.abs().t() + mean_in.abs() * s.abs()) + c.abs()
        ry = _ratio((y - y64).abs(), 5e-7 * scale + 1.2e-7)
        assert ry <= 1.0, ("y", tag, ry)
        # the slot partials
        ys = y.view(M, slots, 64)
        sum64 = ys.sum(-1)
        dev = ys - (sum64 / 64)[..., None]
        m2_64 = (dev ** 2).sum(-1)
        tol_sum = 64 * 2.0 ** -21 * ys.abs().amax(-1)
        tol_m2 = 2 * tol_sum * dev.abs().amax(-1)
        p1 = part1[g][:slots].view(slots, M, 2)
        rs, rq = _ratio((p1[..., 0].t().double() - sum64).abs(), tol_sum), _ratio((p1[..., 1].t().double() - m2_64).abs(), tol_m2)
        assert rs <= 1.0 and rq <= 1.0, ("ln_part_out", tag, rs, rq)
        assert _guard_intact(part1[g], slots) and torch.equal(part2[g][:slots], part1[g][:slots]), ("ln_part_out of out_mode 2", tag)
        # ... combined: the next LayerNorm's statistics
        mean64, var64, rstd64 = _ln64(y)
        mean_tol = (slots + 2) * U * sum64.abs().sum(-1) / N + tol_sum.sum(-1) / N
        rel = (slots + 4) * 2.0 ** -23 + (tol_m2 + 2 * (sum64 / 64 - mean64[:, None]).abs() * tol_sum).sum(-1) / (2 * N * (var64 + EPS))
        assert _guard_intact(stat[g], M)
        rm, rr = _ratio((stat[g][:M, 0].double() - mean64).abs(), mean_tol), _ratio((stat[g][:M, 1].double() / rstd64 - 1).abs(), rel)
        assert rm <= 1.0 and rr <= 1.0, ("chan statistics", tag, rm, rr)
        # ... and against the float64 Chan combination of the fp32 partials it read: section 1's bounds alone
        pd1 = p1.double()
        mu_p = pd1[..., 0].sum(0) / N
        d_p = pd1[..., 0] / 64 - mu_p
        rstd_p = ((pd1[..., 1] + 64 * d_p * d_p).sum(0) / N + EPS).rsqrt()
        rm1 = _ratio((stat[g][:M, 0].double() - mu_p).abs(), (slots + 2) * U * pd1[..., 0].abs().sum(0) / N)
        rr1 = _ratio((stat[g][:M, 1].double() / rstd_p - 1).abs(), torch.full_like(rstd_p, (slots + 4) * 2.0 ** -23))
        assert rm1 <= 1.0 and rr1 <= 1.0, ("chan statistics of the partials", tag, rm1, rr1)
        # the head partials
        hw = o["head_w"][g].double().view(A, slots, 64)
        dots = torch.einsum("msn,asn->sma", ys, hw)
        dscale = torch.einsum("msn,asn->sma", ys.abs(), hw.abs())
        hpg = hp[g][:slots].view(slots, M, HS)
        assert _guard_intact(hp[g], slots) and bool(torch.isnan(hpg[..., A:]).all()), ("head_part padding or guard", tag)
        rh = _ratio((hpg[..., :A].double() - dots).abs(), (2.0 ** -21 + 64 * U) * dscale)
        assert rh <= 1.0, ("head_part", tag, rh)
        # the finish, on the partials it reads
        p2 = part2[g][:slots].view(slots, M, 2).double()
        mu = p2[..., 0].sum(0) / N
        d = p2[..., 0] / 64 - mu
        rstd = ((p2[..., 1] + 64 * d * d).sum(0) / N + EPS).rsqrt()
        hs, hc = o["hs"][g].double(), o["hc"][g].double()
        ref = rstd[:, None] * (hpg[..., :A].double().sum(0) - mu[:, None] * hs) + hc
        fscale = rstd[:, None] * (hpg[..., :A].double().abs().sum(0) + mu.abs()[:, None] * hs.abs()) + hc.abs()
        assert _guard_intact(det[g], M) and bool(torch.isnan(det[g][:M, A:]).all()) and _guard_intact(smp[g], M) and bool(torch.isnan(smp[g][:M, A:]).all())
        rf = _ratio((det[g][:M, :A].double() - ref).abs(), (slots + 4) * U * fscale)
        assert rf <= 1.0, ("finish", tag, rf)
        rl, z = logp_check(smp[g][:M, :A], det[g][:M, :A], lp[g][:M, :A], o["std"][g])
        assert float(z.abs().max()) < 7.0 and bool((cnt[g] == 1).all()), ("finish, sampled", tag)
        assert torch.equal(lp[g][:M, :A], lp_act[g][:M, :A]) and bool(torch.isnan(lp[g][:M, A:]).all()), ("logp against mms_marl_heads_act", tag)
        for k, v in (("y", ry), ("part_sum", rs), ("part_m2", rq), ("stat_mean", rm), ("stat_rstd", rr), ("stat_mean_of_part", rm1), ("stat_rstd_of_part", rr1), ("head_part", rh),
                     ("finish", rf), ("logp", rl)):
            worst[k] = max(worst[k], v)
        if g < 3:                                       # what the comparison of the two builds looks at
            res["y"].append(y.cpu()); res["y_scale"].append(scale.cpu())
            res["head_part"].append(hpg[..., :A].double().cpu()); res["dot_scale"].append(dscale.cpu())
            res["finish"].append(det[g][:M, :A].double().cpu()); res["finish_scale"].append(fscale.cpu())
    _report(tdev, "fold_%s_%s" % (fmt, label or "G%d_M%d_N%d_K%d" % (G, M, N, K)), **worst)
    assert worst["logp"] <= 1.0, ("finish, sampled: logp identity", fmt, G, M, N, K, worst["logp"])   # (last: every group's other checks ran)
    return res


# ---- 5. the fp32 fold kernel -------------------------------------------------------------------------------------------------------
def check_linear_fold32(L, di, stream, tdev, ln_in, ln_out, K, shapes=((128, 128), (256, 384), (128, 384), (256, 128))):
    """mms_linear_group_act with the LayerNorm folds (ln_in: ln_s + ln_stat_in; ln_out: ln_part_out; K = 64: no tail, K = 388: K % 32
    != 0 -- the six instantiations of the fold epilogue), groups = 3, per output:
      y against float64 ELU(rstd (W~ h - mean s) + c) (ln_in) or ELU(x W^T + b): 5e-7 (rstd (|W~||h| + |mean||s|) + |c|), the
        per-element gate of section 4 without the planes' floor.
      ln_part_out (sum, sum of squares per 64-column slot) against float64 of the call's own fp32 y: 64 u sum |y| and 64 u sum y^2.
      mms_row_stats_group on them against the float64 statistics of y: section 1's bounds plus the partials' tolerances carried
        through: mean: + sum_k tol_sum_k / N; rstd (relative): + (sum_k tol_sq_k + 2 |mean| sum_k tol_sum_k) / (2 N (var + eps)).  Those
        carried worst cases leave that gate loose, so the same output is ALSO held to section 1's bounds alone against float64
        statistics of the fp32 partials the kernel read."""
    G = 3
    worst = dict(y=0.0, part_sum=0.0, part_sq=0.0, stat_mean=0.0, stat_rstd=0.0, stat_mean_of_part=0.0, stat_rstd_of_part=0.0)
    for M, N in shapes:
        slots = N // 64
        gen = torch.Generator().manual_seed(1000 * K + M + N + 2 * ln_in + ln_out)
        r = lambda *sh: torch.randn(*sh, generator=gen)
        to = lambda ts: [t.to(tdev) for t in ts]
        z = lambda *sh: torch.zeros(*sh, device=tdev)
        h = to([r(M, K) * (0.5 + 0.25 * i) + 0.2 * i for i in range(G)])
        w, gam, bet, bias = to([r(N, K) / K ** 0.5 for _ in range(G)]), to([1.0 + 0.3 * r(K) for _ in range(G)]), to([0.2 * r(K) for _ in range(G)]), to([0.1 * r(N) for _ in range(G)])
        s = c = stat = None
        wm, bv = w, bias
        if ln_in:
            s, c, wt, stat = [z(N) for _ in range(G)], [z(N) for _ in range(G)], [z(N, K) for _ in range(G)], [z(M, 2) for _ in range(G)]
            _ok(L, L.mms_fold_planes16_group(di, G, _i64([N] * G), _i32([K] * G), _ptrs(w), _ptrs(gam), _ptrs(bet), _ptrs(bias), None, None, _ptrs(s), _ptrs(c), None,
                                             _ptrs(wt), stream), "mms_fold_planes16_group")
            _ok(L, L.mms_row_moments_group(di, G, M, K, 0, _ptrs(h), _ptrs(stat), EPS, stream), "mms_row_moments_group")
            wm, bv = wt, c
        y = [_poison(M, N, tdev) for _ in range(G)]
        part = [_poison(slots, 2 * M, tdev) for _ in range(G)] if ln_out else None
        _ok(L, L.mms_linear_group_act(di, G, M, N, K, _ptrs(h), _ptrs(wm), _ptrs(bv), _ptrs(y), 1, _ptrs(s), _ptrs(stat), _ptrs(part), stream), "mms_linear_group_act")
        st2 = [_poison(M, 2, tdev) for _ in range(G)]
        if ln_out:
            _ok(L, L.mms_row_stats_group(di, G, M, slots, N, _ptrs([p[:slots] for p in part]), _ptrs(st2), EPS, stream), "mms_row_stats_group")
        _sync(tdev)
        for g in range(G):
            tag = (ln_in, ln_out, K, M, N, g)
            h64, w64, b64 = h[g].double(), wm[g].double(), bv[g].double()
            if ln_in:
                mean_in, rstd_in = stat[g][:, 0].double()[:, None], stat[g][:, 1].double()[:, None]
                pre = rstd_in * (h64 @ w64.t() - mean_in * s[g].double()) + b64
                scale = rstd_in * (h64.abs() @ w64.abs().t() + mean_in.abs() * s[g].double().abs()) + b64.abs()
            else:
                pre = h64 @ w64.t() + b64
                scale = h64.abs() @ w64.abs().t() + b64.abs()
            y64 = torch.where(pre > 0, pre, torch.expm1(pre))
            assert _guard_intact(y[g], M)
            ry = _ratio((y[g][:M].double() - y64).abs(), 5e-7 * scale)
            assert ry <= 1.0, ("y", tag, ry)
            worst["y"] = max(worst["y"], ry)
            if not ln_out:
                continue
            ys = y[g][:M].double().view(M, slots, 64)
            sum64, sq64 = ys.sum(-1), (ys ** 2).sum(-1)
            tol_sum, tol_sq = 64 * U * ys.abs().sum(-1), 64 * U * sq64
            p = part[g][:slots].view(slots, M, 2)
            assert _guard_intact(part[g], slots) and _guard_intact(st2[g], M)
            rs, rq = _ratio((p[..., 0].t().double() - sum64).abs(), tol_sum), _ratio((p[..., 1].t().double() - sq64).abs(), tol_sq)
            assert rs <= 1.0 and rq <= 1.0, ("ln_part_out", tag, rs, rq)
            flat = y[g][:M].double()
            mean64, var64, rstd64 = _ln64(flat)
            mean_tol = (slots + 2) * U * sum64.abs().sum(-1) / N + tol_sum.sum(-1) / N
            rel = 1.5 * (slots + 2) * U * (flat ** 2).mean(-1) / (var64 + EPS) + 2.0 ** -23 + \
                (tol_sq.sum(-1) + 2 * mean64.abs() * tol_sum.sum(-1)) / (2 * N * (var64 + EPS))
            rm, rr = _ratio((st2[g][:M, 0].double() - mean64).abs(), mean_tol), _ratio((st2[g][:M, 1].double() / rstd64 - 1).abs(), rel)
            assert rm <= 1.0 and rr <= 1.0, ("row statistics", tag, rm, rr)
            # ... and against float64 statistics of the fp32 partials it read: section 1's bounds alone
            pd = p.double()
            mu_p, ex2_p = pd[..., 0].sum(0) / N, pd[..., 1].sum(0) / N
            var_p = (ex2_p - mu_p * mu_p).clamp_min(0)
            rm1 = _ratio((st2[g][:M, 0].double() - mu_p).abs(), (slots + 2) * U * pd[..., 0].abs().sum(0) / N)
            rr1 = _ratio((st2[g][:M, 1].double() * (var_p + EPS).sqrt() - 1).abs(), 1.5 * (slots + 2) * U * ex2_p / (var_p + EPS) + 2.0 ** -23)
            assert rm1 <= 1.0 and rr1 <= 1.0, ("row statistics of the partials", tag, rm1, rr1)
            for k, v in (("part_sum", rs), ("part_sq", rq), ("stat_mean", rm), ("stat_rstd", rr), ("stat_mean_of_part", rm1), ("stat_rstd_of_part", rr1)):
                worst[k] = max(worst[k], v)
    _report(tdev, "linear_fold32_in%d_out%d_K%d" % (ln_in, ln_out, K), **worst)


# ---- 6. the two builds against each other --------------------------------------------------------------------------------------------
def row_stats_builds_agree(a, b, chan):
    """Section 1's outputs of two builds (dicts of check_row_stats).  The summation orders agree (the slots in order, in both kernels and
    both builds), but the results are not bit-equal and cannot be asked to be: the device code is built with reciprocal-based division
    and root (csrc/Makefile: -fno-hip-fp32-correctly-rounded-divide-sqrt; sum / width is v_rcp and a product, 1 / sqrt is v_rsq), the
    HIP compiler contracts 64 d d + m2 and sq / width - mean^2 into fused multiply-adds, and the CPU build does neither
    (-ffp-contract=off, IEEE division).  So both outputs are held to twice section 1's bound (each build within the bound of the
    float64 value)."""
    worst = 0.0
    for (M, slots), ga in a.items():
        gb = b[(M, slots)]
        x = _stats_data(M, slots, seed=1000 * M + slots)
        _, rstd64, mean_tol, rel = row_stats_bounds(x, _stats_partials(x, chan), chan)
        r = max(_ratio((ga[..., 0] - gb[..., 0]).abs(), 2 * mean_tol), _ratio((ga[..., 1] - gb[..., 1]).abs() / rstd64, 2 * rel))
        assert r <= 1.0, (chan, M, slots, r)
        worst = max(worst, r)
    return worst


def layernorm_builds_agree(a, b, K, Ms):
    """Sections 2's outputs of two builds at 1e-5 of the per-output scale (max|x| for the mean, rstd itself, |xhat||gamma| + |beta| for
    y): the builds sum a row in different orders (64 lane chains and a butterfly against one chain), the bound and its reasoning are
    test_sac_actor_gpu.py::test_kernel_against_cpu_build's.  y also carries the difference of the two means times rstd |gamma|, each
    mean within section 2's mean_tol of float64: + 2 mean_tol rstd |gamma|.  That term is all there is on the constant row (xhat = 0,
    rstd = eps^-1/2 = 316: one ulp between the means is 2e-5 |gamma| in y, against 1e-5 |beta|)."""
    worst = 0.0
    for M in Ms:
        block, gamma, beta = _ln_data(M, K, seed=31 * K + M)
        for key, va in a.items():
            if key[0] != M:
                continue
            for g in range(2):
                x64 = block[g][:, 1, :].double()
                mean, _, rstd, y64, mean_tol, _ = ln_bounds(x64, gamma[g].double(), beta[g].double(), K)
                da, db = va[g].double(), b[key][g].double()
                if key[2] == "stat":
                    r = max(_ratio((da[:, 0] - db[:, 0]).abs(), 1e-5 * x64.abs().amax(-1)), _ratio((da[:, 1] - db[:, 1]).abs(), 1e-5 * rstd))
                else:
                    xhat = (x64 - mean[:, None]) * rstd[:, None]
                    r = _ratio((da[:, :K] - db[:, :K]).abs(), (1e-5 * xhat.abs() + 2 * (mean_tol * rstd)[:, None]) * gamma[g].double().abs() + 1e-5 * beta[g].double().abs())
                assert r <= 1.0, (K, key, g, r)
                worst = max(worst, r)
    return worst


def heads_builds_agree(a, b, H, M, A=(1, 3, 8, 16), seed=5):
    """Section 3's means of two builds at 1e-5 (sum_k |LN(h)_k||w_jk| + |b_j|)."""
    pr = heads_data(H, M, A, seed + 7 * H + M, "cpu")
    worst = 0.0
    for key, eps in (("mean", EPS), ("mean_plain", -1.0)):
        for g in range(len(A)):
            _, _, scale = heads_reference(pr, g, M, eps)
            r = _ratio((a[key][g].double() - b[key][g].double()).abs(), 1e-5 * scale)
            assert r <= 1.0, (H, M, key, g, r)
            worst = max(worst, r)
    return worst


def fold_builds_agree(a, b):
    """Section 4's outputs of two builds (the first three groups) at 1e-5 of the per-output scale."""
    worst = 0.0
    for what, scale in (("y", "y_scale"), ("head_part", "dot_scale"), ("finish", "finish_scale")):
        for g in range(len(a[what])):
            r = _ratio((a[what][g] - b[what][g]).abs(), 1e-5 * a[scale][g])
            assert r <= 1.0, (what, g, r)
            worst = max(worst, r)
    return worst

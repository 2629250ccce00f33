"""The weight-refresh entries per output and on both load paths: mms_fold_planes16_group, mms_fold_scales16_group
(csrc/fold16_kernels.hip), mms_weight_planes16_group, mms_chain_refresh16 (split16_planes_kernel in per-group mode and
chain_refresh16_kernel, csrc/split16_kernels.hip) and the grouped form of mms_split_planes_group -- one check list for both builds:
tests/test_refresh_kernels.py runs it on libmms_cpu.so, tests/test_refresh_kernels_gpu.py on libmms.so.  Every function takes
(L, device_index, stream, torch_device) and drives the C ABI through ctypes.

Which launch runs which instantiation.  The launchers choose ONE instantiation for a whole launch, from the launch's composition alone
(no dispatch override exists, none is read or set here):
  launch_fold_planes16          fold_planes16_kernel<true> iff EVERY group has K % 4 == 0 and 16-byte aligned w, gamma, beta, wt (a NULL
                                counts as aligned); one group with K % 4 != 0, or one pointer 4 bytes off, makes it <false> for all groups.
  launch_split16_planes_group   (per-group mode) split16_planes_kernel<true> iff every group has K % 4 == 0 and a 16-byte aligned w.
  launch_split_planes_group     split_planes_kernel<true> iff x_pitch % 4 == 0 and every group's x is 16-byte aligned.
So the same matrices are run (a) in an all-aligned launch (<true>: what GroupedPolicyInference and ActorCritic launch), (b) in a launch
that also carries a K = 5 group (<false>) and (c) from buffers shifted by 4 bytes (<false>; data_ptr() % 16 == 4 is asserted), and the
three results are compared with each other.  Inside <true>, a last 8-element piece with fewer than 8 elements (K = 100, 388: 4) takes
the guarded element loads.  The CPU build has one loop for all of this; there the arrangements check the host side of the entries.

Gates.  u = 2^-24, the unit roundoff of fp32.  References are float64 torch on the same fp32 inputs.  A sum of n fp32 terms in which
one term goes through at most D additions is within D u sum |terms| of the exact sum of the rounded terms (first order); each term is
a product rounded once, or not at all where the compiler contracts it into the addition: (D + 2) u sum |terms| covers both.
  D, HIP build: a lane adds 8 elements per trip of the row loop, ceil(pieces / 64) trips (pieces = 4 ceil(K / 32) pieces of 8), then the
     six-level butterfly: D = 8 ceil(pieces / 64) + 6 (the first addition, to 0, is exact, which pays for the bias added last).
  D, CPU build: one chain over the row, D = K.
  l1 of mms_weight_planes16_group: P <= 64 lanes per row, ceil(pieces / P) trips and log2(P) levels, on both builds (the CPU build
     follows the lane order): for P < 64 that is 8 + log2(P) <= 14, so the HIP D above bounds it for every K.
  rb = sqrt(l2) sqrt(K) + |c|: l2 is a sum of squares (non-negative terms, D additions and one rounding per square: (D + 1) u relative),
     halved by the root; the two roots, their product and the conversion of K: + 4 u; |c| carries c's own gate; the last addition rounds
     at u |rb|:  ((D + 1) / 2 + 4) u |W~ row|_2 sqrt(K) + gate(c) + u |rb|.
Everything else is exact and compared bit for bit: wt = fp32(w gamma) is one rounding; the planes, scales and inverse scales are those
of mms_split_planes16_group on the same matrix (powers of two, hi = f16(t), lo = f16((t - hi) 2^11)); a maximum has no order.

Inputs are drawn so that one wrong element is larger than a gate (fold_mat: |w| in [0.25, 1], |gamma| in [0.7, 1.3], |beta| in
[0.1, 0.2], bias in [-1, 1]), and that is asserted on the reference (separation): for every row the gates of s, c and rb are at most half
the row's smallest |w gamma| (s, rb) and smallest |w beta| (c) -- a dropped, doubled or misplaced element cannot pass.  (The bias is one
term of c but not part of that condition: a bias in [-1, 1] may be as small as it likes; a dropped bias vector shows in all rows but a
few.)  For rb, whose dependence on one element is quadratic, the change of the reference when the row's smallest element is dropped,
(|row|_2 - sqrt(|row|_2^2 - t^2)) sqrt(K), is in addition asserted to be at least twice the rb gate: with the HIP build's D at every K,
with the CPU build's D = K up to K = 520 (gate / change 0.31 there).  That gate grows as K^1.5 and passes half the change at K of about
700 (K = 1024: gate 0.028 against a change of 0.022) -- at 1023 and 1024 the CPU build's rb is held by the typical element (|w gamma| of
0.6 moves rb by 0.28), not by the smallest.  Every output buffer is filled with a sentinel (NaN; 0xAB bytes for planes) before the
launch and carries GUARD rows behind row N[g]; outputs not asked for, and the guard rows, must still be sentinel afterwards.
Each check prints and records (parity.record, "<gpu|cpu>/refresh_kernels/...") its worst observed error / gate."""
import ctypes
import math

import numpy as np
import torch

import marl_kernels_check as mk
import parity
import planes16_check as pc
from marl_kernels_check import _i32, _i64, _ok, _ptrs, _ratio, _sync, _where

U = 2.0 ** -24
GUARD = 2
SENT_BYTE = 0xAB
SLACK32 = float(np.float32(1.001))                # kBoundSlack as the kernels hold it
FOLD_IN = ("gamma", "beta", "bias")
FOLD_OUT = ("planes", "inv", "s", "c", "rb", "wt")
ALIGNED_K = (4, 64, 100, 388, 512, 520, 1024)     # 100, 388: a 4-element last piece; 512: exactly 64 pieces; 520: lane 0 alone takes a second trip
UNALIGNED_K = (1, 5, 46, 47, 513, 1023)
FOLD_N = (1, 3, 5, 130)


def _report(tdev, name, **vals):
    print("%s/refresh_kernels/%s: %s" % (_where(tdev), name, ", ".join("%s %.3g" % kv for kv in sorted(vals.items()))))
    parity.record("%s/refresh_kernels/%s" % (_where(tdev), name), **vals)


def _is_cpu(tdev):
    return torch.device(tdev).type == "cpu"


def depth(tdev, K):
    """D of the module docstring for a row of K elements"""
    if _is_cpu(tdev):
        return K
    pieces = 4 * ((K + 31) // 32)
    return 8 * ((pieces + 63) // 64) + 6


def depth_hip(K):
    return depth("cuda", K)


def _h32(rows, K):
    return rows * ((K + 31) // 32) * 128


def _signed(gen, lo, hi, *shape):
    mag = lo + (hi - lo) * torch.rand(*shape, generator=gen)
    return torch.where(torch.rand(*shape, generator=gen) < 0.5, -mag, mag).float()


def _shifted(t, tdev, fill=None):
    """a copy of t (or, fill given, a tensor of t's shape filled with it) that starts 4 bytes behind a 16-byte boundary"""
    flat = torch.zeros(t.numel() + 1, dtype=torch.float32, device=tdev)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:].view(t.shape)
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    assert v.data_ptr() % 16 == 4
    return v


def _nan(tdev, *shape):
    t = torch.full(shape, float("nan"), device=tdev)
    assert t.data_ptr() % 16 == 0
    return t


def _split16_one(L, di, stream, tdev, x):
    """mms_split_planes16_group on the single matrix x [rows, K] (CPU fp32): (planes uint8, scale, inv) on the CPU"""
    rows, K = x.shape
    xd = x.to(tdev).contiguous()
    planes = torch.full((_h32(rows, K),), SENT_BYTE, dtype=torch.uint8, device=tdev)
    scale, inv = _nan(tdev, rows), _nan(tdev, rows)
    _ok(L, L.mms_split_planes16_group(di, 1, rows, K, 0, _ptrs([xd]), _ptrs([planes]), _ptrs([scale]), _ptrs([inv]), 0, 0, None, None, None, None, 0.0, stream),
        "mms_split_planes16_group")
    _sync(tdev)
    return planes.cpu(), scale.cpu(), inv.cpu()


def _pad_columns_zero(planes, rows, K):
    KC = (K + 31) // 32
    v = planes.view(torch.float16).view(rows, KC, 2, 32).permute(0, 2, 1, 3).reshape(rows, 2, KC * 32)
    return bool((v[:, :, K:] == 0).all())


# ---- 1. mms_fold_planes16_group ----------------------------------------------------------------------------------------------------
def fold_mat(N, K, seed, rows=None):
    """one group's operands: N rows are folded, the buffers hold `rows` (default N)"""
    gen = torch.Generator().manual_seed(seed)
    R = N if rows is None else rows
    return dict(N=N, K=K, w=_signed(gen, 0.25, 1.0, R, K), gamma=_signed(gen, 0.7, 1.3, K), beta=_signed(gen, 0.1, 0.2, K),
                bias=(2 * torch.rand(R, generator=gen) - 1).float())


def fold_set(Ks, Ns=FOLD_N, seed=100):
    return [fold_mat(N, K, seed + 1000 * K + N) for K in Ks for N in Ns]


def fold_run(L, di, stream, tdev, mats, null_arrays=(), absent=None, shift=False):
    """One mms_fold_planes16_group launch over `mats`.  null_arrays: names passed as a NULL array; absent[g]: names whose entry of group g
    is NULL.  shift: w, gamma, beta and wt 4 bytes off a 16-byte boundary.  Checks the sentinels (outputs not asked for, guard rows) and
    returns per group dict(eff = the operands the launch saw, and each output's live rows on the CPU, None where not asked for)."""
    G = len(mats)
    absent = absent or [set() for _ in range(G)]
    has = lambda name, g: name not in null_arrays and name not in absent[g] and (name in FOLD_OUT or mats[g].get(name) is not None)
    put = (lambda t: _shifted(t, tdev)) if shift else (lambda t: t.to(tdev).contiguous())
    dev = {"w": [put(m["w"]) for m in mats], "bias": [None if m.get("bias") is None else m["bias"].to(tdev) for m in mats]}
    for name in ("gamma", "beta"):
        dev[name] = [None if m.get(name) is None else put(m[name]) for m in mats]
    for t in dev["w"]:
        assert t.data_ptr() % 16 == (4 if shift else 0)
    bufs = []
    for m in mats:
        R, K = m["w"].shape
        b = dict(planes=torch.full((_h32(R + GUARD, K),), SENT_BYTE, dtype=torch.uint8, device=tdev))
        for name in ("inv", "s", "c", "rb"):
            b[name] = _nan(tdev, R + GUARD)
        b["wt"] = _shifted(torch.empty(R + GUARD, K), tdev, fill=float("nan")) if shift else _nan(tdev, R + GUARD, K)
        assert b["planes"].data_ptr() % 16 == 0
        bufs.append(b)
    arr_in = lambda name: None if name in null_arrays else _ptrs([dev[name][g] if has(name, g) else None for g in range(G)])
    arr_out = lambda name: None if name in null_arrays else _ptrs([bufs[g][name] if has(name, g) else None for g in range(G)])
    _ok(L, L.mms_fold_planes16_group(di, G, _i64([m["N"] for m in mats]), _i32([m["K"] for m in mats]), _ptrs(dev["w"]), arr_in("gamma"), arr_in("beta"),
                                     arr_in("bias"), arr_out("planes"), arr_out("inv"), arr_out("s"), arr_out("c"), arr_out("rb"), arr_out("wt"), stream),
        "mms_fold_planes16_group")
    _sync(tdev)
    res = []
    for g, m in enumerate(mats):
        N, K = m["N"], m["K"]
        out = dict(eff=dict(N=N, K=K, w=m["w"][:N], **{name: (m[name] if has(name, g) else None) for name in FOLD_IN}))
        if out["eff"]["bias"] is not None:
            out["eff"]["bias"] = out["eff"]["bias"][:N]
        for name in FOLD_OUT:
            b = bufs[g][name]
            live = N if has(name, g) else 0
            if name == "planes":
                assert bool((b[_h32(live, K):] == SENT_BYTE).all()), ("planes: rows behind N[g], or planes not asked for, written", g, N, K)
                out[name] = b[:_h32(N, K)].cpu() if live else None
            else:
                assert bool(torch.isnan(b[live:]).all()), ("%s: rows behind N[g], or an output not asked for, written" % name, g, N, K)
                out[name] = b[:N].cpu() if has(name, g) else None
        res.append(out)
    return res


def fold_reference(eff, mutation=None):
    """float64 statement of the fold on one group's operands.  mutation ("element": the smallest |w gamma| of row 0 zeroed; "tail": the
    elements of the last, partial 8-element piece zeroed) changes the REFERENCE's inputs: the self-check of the gates."""
    N, K = eff["N"], eff["K"]
    w32 = eff["w"]
    wt32 = w32 * eff["gamma"][None, :] if eff["gamma"] is not None else w32.clone()
    w = w32.double().clone()
    gam = eff["gamma"].double() if eff["gamma"] is not None else torch.ones(K, dtype=torch.float64)
    if mutation == "element":
        w[0, int((w[0] * gam).abs().argmin())] = 0.0
    elif mutation == "tail":
        assert K % 8 != 0
        w[:, K - K % 8:] = 0.0
    ts = w * gam[None, :]
    tc = w * eff["beta"].double()[None, :] if eff["beta"] is not None else torch.zeros_like(w)
    b = eff["bias"].double() if eff["bias"] is not None else torch.zeros(N, dtype=torch.float64)
    c = tc.sum(1) + b
    l2 = ts.pow(2).sum(1).sqrt()
    return dict(wt=wt32, ts=ts, tc=tc, s=ts.sum(1), c=c, l2=l2, rb=l2 * K ** 0.5 + c.abs(), abs_s=ts.abs().sum(1), abs_c=tc.abs().sum(1) + b.abs())


def fold_gates(ref, K, D):
    """the gates of s, c and rb (module docstring), per row"""
    gs = (D + 2) * U * ref["abs_s"]
    gc = (D + 2) * U * ref["abs_c"]
    grb = ((D + 1) / 2.0 + 4) * U * ref["l2"] * K ** 0.5 + gc + U * ref["rb"].abs()
    return dict(s=gs, c=gc, rb=grb)


def fold_ratios(out, ref, K, D):
    """worst error / gate of the outputs that are there"""
    gates = fold_gates(ref, K, D)
    return {k: _ratio((out[k].double() - ref[k]).abs(), gates[k]) for k in ("s", "c", "rb") if out[k] is not None}


def assert_separation(tdev, eff, ref):
    """the condition on the inputs (module docstring): no gate above half the row's smallest term.  Returns the worst gate / term."""
    K = eff["K"]
    gates = fold_gates(ref, K, depth(tdev, K))
    min_s, min_c = ref["ts"].abs().amin(1), ref["tc"].abs().amin(1)
    worst = max(float((gates["s"] / min_s).max()), float((gates["c"] / min_c).max()), float((gates["rb"] / min_s).max()))
    assert worst <= 0.5, ("a gate is above half the smallest term: change the seed", eff["N"], K, worst)
    drop = (ref["l2"] - (ref["l2"] ** 2 - min_s ** 2).clamp_min(0).sqrt()) * K ** 0.5
    for D in {depth_hip(K)} | ({depth(tdev, K)} if K <= 520 else set()):
        w_rb = float((fold_gates(ref, K, D)["rb"] / drop).max())
        assert w_rb <= 0.5, ("the rb gate is above half of what the smallest element moves rb by: change the seed", eff["N"], K, D, w_rb)
    return worst


def fold_verify(L, di, stream, tdev, outs, separation=False):
    """Every group of one launch against the reference: wt bit for bit, planes and inv those of mms_split_planes16_group on W~, plane
    columns past K zero, s / c / rb inside their gates.  Returns the worst error / gate per output."""
    worst = dict(s=0.0, c=0.0, rb=0.0)
    sep = 0.0
    for g, out in enumerate(outs):
        eff = out["eff"]
        N, K = eff["N"], eff["K"]
        if N == 0:
            continue
        ref = fold_reference(eff)
        if separation:
            sep = max(sep, assert_separation(tdev, eff, ref))
        if out["wt"] is not None:
            assert torch.equal(out["wt"], ref["wt"]), ("wt != fp32(w gamma)", g, N, K)
        if out["planes"] is not None or out["inv"] is not None:
            p2, _, i2 = _split16_one(L, di, stream, tdev, ref["wt"])
        if out["planes"] is not None:                    # (as fp16 values, as planes16_check compares: the device may leave -0 in a lo plane)
            assert torch.equal(out["planes"].view(torch.float16), p2.view(torch.float16)), ("planes", g, N, K)
            assert _pad_columns_zero(out["planes"], N, K), ("plane columns past K", g, N, K)
        if out["inv"] is not None:
            assert torch.equal(out["inv"].view(torch.int32), i2.view(torch.int32)), ("inv", g, N, K)
        r = fold_ratios(out, ref, K, depth(tdev, K))
        assert all(v <= 1.0 for v in r.values()), ("fold outputs against float64", g, N, K, r)
        for k, v in r.items():
            worst[k] = max(worst[k], v)
    if separation:
        worst["separation"] = sep
    return worst


def _same(a, b, names):
    """how many elements of the named outputs differ between two results of the same matrices, and by how much at most"""
    n, d = 0, 0.0
    for oa, ob in zip(a, b):
        for name in names:
            if oa[name] is None:
                continue
            ta, tb = oa[name], ob[name]
            if ta.dtype == torch.uint8:
                n += int((ta != tb).sum())
            else:
                ne = ta.view(torch.int32) != tb.view(torch.int32)
                n += int(ne.sum())
                if bool(ne.any()):
                    d = max(d, float((ta.double() - tb.double()).abs().max()))
    return n, d


def check_fold_aligned_paths(L, di, stream, tdev):
    """The all-aligned set (ALIGNED_K x FOLD_N, 28 matrices, one launch: fold_planes16_kernel<true>) per output against float64, and
    the same matrices (b) beside a K = 5 group and (c) from w / gamma / beta / wt buffers 4 bytes off (both <false>): wt, planes and inv
    bit-identical across the three, s / c / rb inside their gates in each, and (b) and (c), two launches of one instantiation, equal in
    s / c / rb bit for bit.
    s / c / rb of <true> against <false>: the instantiations differ in their loads only and every lane sums the same elements in the
    same order, but the results are identical only in c and rb.  Measured on the MI355X (973 rows): c and rb equal bit for bit in all
    rows; s differs in 636 rows, by at most 7.6e-6 (one or two ulp of s; s is within 0.10 of its gate on either path).  The cause is
    the compiler's, not the kernel's: the device code is built with contraction on, and it turns a different number of the row loop's
    `s += w gamma` into fused multiply-adds in the two instantiations (their code has 17 against 23 v_fmac_f32), so a product is
    rounded before the addition in one and not in the other -- what the + 2 of the gate is there for.  So the identity of s / c / rb
    across the load paths is recorded (differing_* / largest_difference_*), and asserted only where there is one loop: on the CPU build."""
    mats = fold_set(ALIGNED_K)
    a = fold_run(L, di, stream, tdev, mats)
    worst = fold_verify(L, di, stream, tdev, a, separation=True)
    b = fold_run(L, di, stream, tdev, mats + [fold_mat(3, 5, 77)])
    c = fold_run(L, di, stream, tdev, mats, shift=True)
    for name, other in (("beside_K5", b), ("shifted", c)):
        w2 = fold_verify(L, di, stream, tdev, other)
        for k in ("s", "c", "rb"):
            worst[k] = max(worst[k], w2[k])
        n_exact, _ = _same(a, other[:len(mats)], ("wt", "planes", "inv"))
        assert n_exact == 0, ("wt / planes / inv differ between the aligned launch and the %s one" % name, n_exact)
        for k in ("s", "c", "rb"):
            worst["differing_%s_%s" % (k, name)], worst["largest_difference_%s_%s" % (k, name)] = _same(a, other[:len(mats)], (k,))
    n_ff, _ = _same(b[:len(mats)], c, ("s", "c", "rb"))
    assert n_ff == 0, ("s / c / rb differ between two launches of the same instantiation", n_ff)
    worst["rows"] = sum(m["N"] for m in mats)
    _report(tdev, "fold_planes_aligned_paths", **worst)
    if _is_cpu(tdev):
        assert not any(v for k, v in worst.items() if k.startswith("differing_")), ("s / c / rb depend on the arrangement of the launch", worst)
    return worst


def check_fold_unaligned(L, di, stream, tdev):
    """UNALIGNED_K x FOLD_N (24 matrices, one launch, <false> by width: rows that start at any 4-byte offset, ragged last pieces, K = 1
    and 5 below one piece, 513 and 1023 with a second trip) per output against float64."""
    worst = fold_verify(L, di, stream, tdev, fold_run(L, di, stream, tdev, fold_set(UNALIGNED_K, seed=300)), separation=True)
    _report(tdev, "fold_planes_unaligned", **worst)
    return worst


def check_fold_heads_shaped(L, di, stream, tdev):
    """The heads' launch of GroupedPolicyInference._derived: K = 128, N = [8, 8, 1, 1, 0] into buffers of 8 rows (+ guards): the groups
    of one row and of none get surplus blocks (grid.x = 2 for all), whose waves redo the last row without storing (`live == false`);
    rows 1..7 of the one-row groups and everything of the empty group stay sentinel.  Aligned, and beside a K = 5 group."""
    worst = dict(s=0.0, c=0.0, rb=0.0)
    for extra in ([], [fold_mat(3, 5, 78)]):
        mats = [fold_mat(N, 128, 500 + g, rows=8) for g, N in enumerate((8, 8, 1, 1, 0))]
        w2 = fold_verify(L, di, stream, tdev, fold_run(L, di, stream, tdev, mats + extra), separation=True)
        worst = {k: max(worst[k], w2[k]) for k in worst}
    _report(tdev, "fold_planes_heads_shaped", **worst)


FOLD_OPTIONAL = {
    "gamma_only": dict(null_arrays=("beta",)),
    "beta_only": dict(null_arrays=("gamma",)),
    "no_bias": dict(null_arrays=("bias",)),
    "no_planes_no_inv": dict(null_arrays=("planes", "inv")),
    "no_wt": dict(null_arrays=("wt",)),
    "no_rb": dict(null_arrays=("rb",)),
    "plain_matrix_s_only": dict(null_arrays=("gamma", "beta", "bias", "planes", "inv", "c", "rb", "wt")),
    "mixed_per_group": dict(absent=[{"gamma", "s"}, {"beta", "planes", "inv", "c"}, {"bias", "wt", "rb"}, {"planes"}]),
}


def check_fold_optional(L, di, stream, tdev, which, aligned):
    """One launch per optional-argument form (FOLD_OPTIONAL: arrays passed as NULL, and NULL entries mixed per group in one launch), on
    four matrices that select <true> (aligned) or <false> (one K = 47 among them).  The reference leaves out what the launch left out
    (no gamma: W~ = w; no beta: c = bias; no bias: c = W beta; neither: c = 0); outputs not asked for stay sentinel (fold_run)."""
    shapes = ((5, 64), (3, 100), (6, 520), (7, 128 if aligned else 47))
    mats = [fold_mat(N, K, 900 + g) for g, (N, K) in enumerate(shapes)]
    worst = fold_verify(L, di, stream, tdev, fold_run(L, di, stream, tdev, mats, **FOLD_OPTIONAL[which]))
    _report(tdev, "fold_planes_optional_%s_%s" % (which, "aligned" if aligned else "unaligned"), **worst)


def check_fold_boundary_rows(L, di, stream, tdev):
    """planes16_check's rows (largest |w gamma| = each of planes16_check.BOUNDS at a random column, an all-zero row) through the fold,
    once with gamma = 1 and once with gamma = 2^-3 on w 2^3 (the product is exact): inv == 2^(frexp - 14) and the planes those of scale
    2^(14 - frexp) exactly (numpy float16 emulation); the all-zero row has inv 1 (scale 1), zero planes, s = 0 and rb = |c| = |bias|.
    K = 46 and 64 in one launch (<false>), K = 64 alone (<true>)."""
    for Ks in ((46, 64), (64,)):
        mats, want = [], []
        for K in Ks:
            x, big = pc.inputs(K)
            for gam in (1.0, 0.125):
                gen = torch.Generator().manual_seed(K)
                mats.append(dict(N=pc.ROWS, K=K, w=torch.from_numpy(x / np.float32(gam)), gamma=torch.full((K,), gam), beta=None,
                                 bias=(2 * torch.rand(pc.ROWS, generator=gen) - 1).float()))
                want.append((x, big))
        outs = fold_run(L, di, stream, tdev, mats)
        for out, (x, big) in zip(outs, want):
            K = out["eff"]["K"]
            scale, inv = pc.expected_scales(big)
            assert torch.equal(out["wt"], torch.from_numpy(x)), (Ks, K)
            assert np.array_equal(out["inv"].numpy().view(np.uint32), inv.view(np.uint32)), (Ks, K, out["inv"], inv)
            planes = torch.from_numpy(pc.emulate_planes(x, scale).view(np.int16)).view(torch.float16).reshape(-1)
            assert torch.equal(out["planes"].view(torch.float16), planes), (Ks, K)
            zero = [r for r in range(pc.ROWS) if big[r] == 0]
            assert zero
            for r in zero:
                assert float(out["inv"][r]) == 1.0 and float(out["s"][r]) == 0.0 and float(out["rb"][r]) == abs(float(out["eff"]["bias"][r])) == abs(float(out["c"][r]))
                assert bool((out["planes"].view(torch.float16).view(pc.ROWS, -1)[r] == 0).all())


def check_fold_gates_see_mutations(L, di, stream, tdev, mutation, K):
    """The gates' self-check: the build's outputs against a float64 reference whose inputs lost one element of row 0 (its smallest
    |w gamma|) or the elements of the last, partial piece (every row): s, c and rb must miss their gates at least twice over (element:
    row 0; tail: the worst row, which is what fold_verify asserts on)."""
    mats = [fold_mat(5, K, 4000 + K)]
    out = fold_run(L, di, stream, tdev, mats)[0]
    ref = fold_reference(out["eff"], mutation)
    clean = fold_ratios(out, fold_reference(out["eff"]), K, depth(tdev, K))
    assert max(clean.values()) <= 1.0, clean
    if mutation == "element":
        out = {k: (v[:1] if k in ("s", "c", "rb") else v) for k, v in out.items()}
        ref = {k: v[:1] for k, v in ref.items()}
    r = fold_ratios(out, ref, K, depth(tdev, K))
    _report(tdev, "fold_planes_mutation_%s_K%d" % (mutation, K), **r)
    assert sorted(r) == ["c", "rb", "s"] and min(r.values()) >= 2.0, (mutation, K, r)
    return r


# ---- 2. mms_fold_scales16_group ----------------------------------------------------------------------------------------------------
SCALES_M = (0, 1, 255, 256, 257)
SCALES_CASES = ((0, None, 0.0), (1, 0, 3.7), (255, 254, 0.011), (256, 0, 913.0), (257, 256, 1.3e-4), (1000, 700, 57.0), (1000, 0, 2.9e4), (1000, 999, 0.37),
                (5, None, 0.0), (5, None, 1e-35))       # (n, index of the largest, the largest); the last two: a zero network and one below 1e-30


def scales_data():
    """rb per group [n + 1] (one element behind n holds 1e30: a read past n would win the maximum) and the expected (scale, inv)"""
    gen = torch.Generator().manual_seed(21)
    rbs, want, margin = [], [], 1.0
    for n, at, peak in SCALES_CASES:
        rb = torch.full((n + 1,), 1e30)
        if at is None:
            rb[:n] = peak
        else:
            rb[:n] = (0.1 + 0.8 * torch.rand(n, generator=gen)) * peak
            rb[at] = peak
        m = float(rb[:n].double().max()) if n else 0.0
        bound = m * SLACK32
        if bound > 1e-30:
            f, e = math.frexp(bound)
            assert 0.5 * (1 + 2.0 ** -20) <= f <= 1 - 2.0 ** -20, ("1.001 max is too close to a power of two: change the data", n, peak, f)
            margin = min(margin, 2 * f - 1, 1 - f)
            want.append((2.0 ** (14 - e), 2.0 ** (e - 14)))
        else:
            want.append((2.0 ** 100, 2.0 ** -100))          # the zero network: the bound floored at 1e-30, the shift clamped
        rbs.append(rb)
    return rbs, want, margin


def check_fold_scales(L, di, stream, tdev):
    """mms_fold_scales16_group: n[g] in {0, 1, 255, 256, 257, 1000} in one launch (more than one trip of the 256-thread loop; the largest
    row bound first, last, and at an index >= 256), M in SCALES_M (no batch rows, one block, a ragged second block), scale1 / ysc / yinv
    each present, NULL as an array, or NULL per group.  Expected exactly 2^(14 - e), 2^(e - 14) with e = frexp(1.001 max) from the float64
    maximum; 1.001 max is asserted to sit 2^-20 (relative) inside its binade, so the one fp32 rounding of the product cannot move e.
    Zero networks (all rb zero, rb = 1e-35, n = 0) get 2^100 / 2^-100.  scale inv == 1; M guard elements stay NaN."""
    rbs, want, margin = scales_data()
    G = len(rbs)
    rbd = [t.to(tdev) for t in rbs]
    n = [c[0] for c in SCALES_CASES]
    res = {}
    forms = (set(), {"scale1"}, {"ysc"}, {"yinv"}, "mixed")
    for M in SCALES_M:
        for fi, form in enumerate(forms):
            bufs = dict(scale1=[_nan(tdev, 1 + GUARD) for _ in range(G)], ysc=[_nan(tdev, M + GUARD) for _ in range(G)], yinv=[_nan(tdev, M + GUARD) for _ in range(G)])
            if form == "mixed":
                has = lambda name, g: (g + ("scale1", "ysc", "yinv").index(name)) % 3 != 0
                arr = lambda name: _ptrs([bufs[name][g] if has(name, g) else None for g in range(G)])
            else:
                has = lambda name, g, form=form: name not in form
                arr = lambda name, form=form: None if name in form else _ptrs(bufs[name])
            _ok(L, L.mms_fold_scales16_group(di, G, _ptrs(rbd), _i32(n), M, arr("scale1"), arr("ysc"), arr("yinv"), stream), "mms_fold_scales16_group")
            _sync(tdev)
            for g in range(G):
                sc, iv = want[g]
                assert sc * iv == 1.0
                for name, rows, val in (("scale1", 1, sc), ("ysc", M, sc), ("yinv", M, iv)):
                    b = bufs[name][g]
                    if not has(name, g):
                        assert bool(torch.isnan(b).all()), (name, "not asked for, written", M, form, g)
                        continue
                    assert bool(torch.isnan(b[rows:]).all()), (name, "guard", M, form, g)
                    assert bool((b[:rows] == val).all()), (name, M, form, g, n[g], b[:min(rows, 4)].tolist(), val)
            if not form:
                res[M] = dict(scale1=torch.stack([b[:1] for b in bufs["scale1"]]).cpu(), ysc=torch.stack([b[:M] for b in bufs["ysc"]]).cpu(),
                              yinv=torch.stack([b[:M] for b in bufs["yinv"]]).cpu())
    # (exact outputs: there is no error to report; what is recorded is how much room the inputs leave)
    _report(tdev, "fold_scales", launches=len(SCALES_M) * len(forms), networks=G, closest_bound_to_a_power_of_two=margin)
    return res


def check_zero_network_layer(L, di, stream, tdev, M=128, N=128, K=64):
    """A layer of a zero network as the refresh leaves it -- W~ = 0, s = c = 0, rb = 0, so y_scale = 2^100 and its inverse 2^-100 -- through
    mms_linear_group_act_split16 (out_mode 1, the LayerNorm folds): zero planes and finite (zero-sum) partials: the scale of a zero
    network does no harm."""
    gen = torch.Generator().manual_seed(8)
    z = lambda *sh: torch.zeros(*sh, device=tdev)
    o = dict(fmt="f16x2", G=1, M=M, N=N, K=K, A=[1])
    h = [(torch.randn(M, K, generator=gen) * 0.7 + 0.2).to(tdev)]
    o["wp"] = [torch.full((_h32(N, K),), SENT_BYTE, dtype=torch.uint8, device=tdev)]
    o["winv"], o["s"], o["c"], rb = ([_nan(tdev, N)] for _ in range(4))
    w0, g1, b0, bias0 = [z(N, K)], [torch.ones(K, device=tdev)], [z(K)], [z(N)]
    _ok(L, L.mms_fold_planes16_group(di, 1, _i64([N]), _i32([K]), _ptrs(w0), _ptrs(g1), _ptrs(b0), _ptrs(bias0), _ptrs(o["wp"]),
                                     _ptrs(o["winv"]), _ptrs(o["s"]), _ptrs(o["c"]), _ptrs(rb), None, stream), "mms_fold_planes16_group")
    o["ysc"], o["yinv"] = [_nan(tdev, M)], [_nan(tdev, M)]
    _ok(L, L.mms_fold_scales16_group(di, 1, _ptrs(rb), _i32([N]), M, None, _ptrs(o["ysc"]), _ptrs(o["yinv"]), stream), "mms_fold_scales16_group")
    o["xp"] = [torch.zeros(_h32(M, K), dtype=torch.uint8, device=tdev)]
    o["stat"], o["xinv"], xs = [z(M, 2)], [z(M)], [z(M)]
    _ok(L, L.mms_split_planes16_group(di, 1, M, K, 0, _ptrs(h), _ptrs(o["xp"]), _ptrs(xs), _ptrs(o["xinv"]), 0, 0, None, None, None, _ptrs(o["stat"]), mk.EPS, stream),
        "mms_split_planes16_group")
    _sync(tdev)
    assert bool((rb[0] == 0).all()) and bool((o["winv"][0] == 1).all()) and bool((o["wp"][0].view(torch.float16) == 0).all())
    assert bool((o["ysc"][0] == 2.0 ** 100).all()) and bool((o["yinv"][0] == 2.0 ** -100).all())
    y, part = mk.fold_layer(L, di, stream, tdev, o, 1)
    body = y[0][:_h32(M, N)]
    assert bool((y[0][body.numel():] == 0xFF).all()), "y guard row written"
    assert bool((body.view(torch.float16) == 0).all()), "a zero network's activations must be zero planes"
    p = part[0][:N // 64]
    assert bool(torch.isfinite(p).all()), "ln_part_out of a zero network must be finite"


# ---- 3. mms_weight_planes16_group --------------------------------------------------------------------------------------------------
WP_ALIGNED = ((70, 4), (33, 36), (21, 100), (11, 200), (5, 388), (1, 512), (0, 1024), (7, 1024), (130, 2500), (3, 64))
# lanes per row P = 4, 8, 16, 32, 64, 64, 64, 64, 64, 8: rows per block 4 x 64 / P = 64, 32, 16, 8, 4, ...: no N is a multiple of its own;
# 33 blocks for the last but one, so every other group has surplus blocks; one N = 0 and one N = 1


def wp_mats(shapes, seed=600):
    out = []
    for g, (N, K) in enumerate(shapes):
        gen = torch.Generator().manual_seed(seed + 7 * K + N)
        out.append(dict(N=N, K=K, w=_signed(gen, 0.25, 1.0, max(N, 1), K)))
    return out


def wp_run(L, di, stream, tdev, mats, l1_absent=None, shift=False):
    """One mms_weight_planes16_group launch.  l1_absent: "all" (a NULL array) or a set of groups whose l1 entry is NULL."""
    G = len(mats)
    l1_absent = l1_absent or set()
    has_l1 = lambda g: l1_absent != "all" and g not in l1_absent
    put = (lambda t: _shifted(t, tdev)) if shift else (lambda t: t.to(tdev).contiguous())
    wd = [put(m["w"]) for m in mats]
    bufs = [dict(planes=torch.full((_h32(m["N"] + GUARD, m["K"]),), SENT_BYTE, dtype=torch.uint8, device=tdev), scale=_nan(tdev, m["N"] + GUARD),
                 inv=_nan(tdev, m["N"] + GUARD), l1=_nan(tdev, m["N"] + GUARD)) for m in mats]
    l1 = None if l1_absent == "all" else _ptrs([bufs[g]["l1"] if has_l1(g) else None for g in range(G)])
    _ok(L, L.mms_weight_planes16_group(di, G, _i64([m["N"] for m in mats]), _i32([m["K"] for m in mats]), _ptrs(wd), _ptrs([b["planes"] for b in bufs]),
                                       _ptrs([b["scale"] for b in bufs]), _ptrs([b["inv"] for b in bufs]), l1, stream), "mms_weight_planes16_group")
    _sync(tdev)
    res = []
    for g, m in enumerate(mats):
        N, K, b = m["N"], m["K"], bufs[g]
        assert bool((b["planes"][_h32(N, K):] == SENT_BYTE).all()), ("planes behind row N[g] written", g, N, K)
        for name in ("scale", "inv", "l1"):
            live = N if (name != "l1" or has_l1(g)) else 0
            assert bool(torch.isnan(b[name][live:]).all()), ("%s behind row N[g], or not asked for, written" % name, g, N, K)
        res.append(dict(N=N, K=K, w=m["w"][:N], planes=b["planes"][:_h32(N, K)].cpu(), scale=b["scale"][:N].cpu(), inv=b["inv"][:N].cpu(),
                        l1=b["l1"][:N].cpu() if has_l1(g) else None))
    return res


def wp_verify(L, di, stream, tdev, outs):
    """planes, scale, inv bit-equal to a single-matrix mms_split_planes16_group; l1 against float64 sum |w| inside (D + 2) u sum |w|
    with the HIP D on both builds (module docstring), and that gate at most half the row's smallest |w|."""
    worst = sep = 0.0
    for g, o in enumerate(outs):
        N, K = o["N"], o["K"]
        if N == 0:
            continue
        p2, s2, i2 = _split16_one(L, di, stream, tdev, o["w"])
        assert torch.equal(o["planes"], p2) and torch.equal(o["scale"].view(torch.int32), s2.view(torch.int32)) and torch.equal(o["inv"].view(torch.int32), i2.view(torch.int32)), (g, N, K)
        assert _pad_columns_zero(o["planes"], N, K), (g, N, K)
        if o["l1"] is None:
            continue
        a = o["w"].double().abs()
        gate = (depth_hip(K) + 2) * U * a.sum(1)
        sep = max(sep, float((gate / a.amin(1)).max()))
        r = _ratio((o["l1"].double() - a.sum(1)).abs(), gate)
        assert r <= 1.0, ("l1", g, N, K, r)
        worst = max(worst, r)
    assert sep <= 0.5, ("the l1 gate is above half the smallest |w|: change the seed", sep)
    return dict(l1=worst, separation=sep)


def check_weight_planes(L, di, stream, tdev):
    """mms_weight_planes16_group in per-group mode.  WP_ALIGNED in one launch (split16_planes_kernel<true>; every lanes-per-row value P in
    one grid, N = 0 and N = 1 among the groups, N never a multiple of the rows per block); K in {5, 46, 1023} beside two of the aligned
    matrices (<false> by width); WP_ALIGNED from w 4 bytes off (<false> by address).  The aligned and the forced-unaligned results of the
    same matrix are bit-identical, l1 included.  l1 present, NULL per group, and NULL as an array.  Returns the l1 of the first launch
    (the two builds agree on it bit for bit: the CPU build follows the lane order)."""
    mats = wp_mats(WP_ALIGNED)
    a = wp_run(L, di, stream, tdev, mats)
    worst = wp_verify(L, di, stream, tdev, a)
    mixed = wp_mats(((6, 5), (19, 46), (9, 1023))) + [mats[1], mats[5], mats[7]]
    b = wp_run(L, di, stream, tdev, mixed, l1_absent={1, 4})
    w2 = wp_verify(L, di, stream, tdev, b)
    c = wp_run(L, di, stream, tdev, mats, shift=True)
    w3 = wp_verify(L, di, stream, tdev, c)
    d = wp_run(L, di, stream, tdev, mats, l1_absent="all")
    wp_verify(L, di, stream, tdev, d)
    same = lambda x, y: all(torch.equal(x[k], y[k]) if k == "planes" else torch.equal(x[k].view(torch.int32), y[k].view(torch.int32))
                            for k in ("planes", "scale", "inv", "l1") if x[k] is not None and y[k] is not None)
    for x, y in list(zip(a, c)) + list(zip(a, d)) + [(a[1], b[3]), (a[5], b[4]), (a[7], b[5])]:
        assert same(x, y), ("aligned and forced-unaligned results differ", x["N"], x["K"])
    worst = dict(l1=max(worst["l1"], w2["l1"], w3["l1"]), separation=max(worst["separation"], w2["separation"], w3["separation"]))
    _report(tdev, "weight_planes", **worst)
    return {(o["N"], o["K"]): o["l1"] for o in a if o["N"]}


# ---- 4. mms_chain_refresh16 --------------------------------------------------------------------------------------------------------
CHAIN_SHAPES = ((1, 1), (2, 2), (5, 3), (8, 4))           # E = nchains L = 1, 4, 15, 32 = MMS_MAX_GROUPS: up to eight trips of the wave loop
CHAIN_N = (0, 1, 63, 64, 65, 1024)
CHAIN_ROWS = (0, 1, 255, 256, 257)
CHAIN_BOUND0 = (0.0, 1e-3, 5.0 / 3.0, 8.0)
CHAIN_MARGIN = 2.0 ** -18                                 # >= the issue's 2^-20: L <= 4 layers of three fp32 roundings carry 12 u = 2^-20.4 into the last bound


def chain_data(nch, Lh, seed):
    """Per entry e: l1 [n + 1] > 0 with the largest in the last element, bias [n + 1] with the largest magnitude last and negative (one
    element behind n holds +-1e30: a read past n would win), n[e] cycling through CHAIN_N (n = 0: the entry is (0, 0))."""
    gen = torch.Generator().manual_seed(seed)
    E = nch * Lh
    n = [CHAIN_N[(e + seed) % len(CHAIN_N)] for e in range(E)]
    l1, bias = [], []
    for e in range(E):
        m, b = 0.4 + 2.0 * float(torch.rand((), generator=gen)), 0.05 + float(torch.rand((), generator=gen))
        a = torch.full((n[e] + 1,), 1e30)
        c = torch.full((n[e] + 1,), -1e30)
        if n[e]:
            a[:n[e]] = (0.1 + 0.8 * torch.rand(n[e], generator=gen)) * m
            c[:n[e]] = (2 * torch.rand(n[e], generator=gen) - 1) * 0.9 * b
            a[n[e] - 1], c[n[e] - 1] = m, -b
        l1.append(a)
        bias.append(c)
    return n, l1, bias


def chain_expected(nch, Lh, n, l1, bias, has_bias, bound0):
    """(chain [nch, Lh, 2] fp32: the exact maxima; scale, inv [nch, Lh] from the float64 recursion bound <- (mult bound + add) 1.001, each
    bound asserted CHAIN_MARGIN (relative) inside its binade: fused or unfused, the fp32 evaluation lands on the same exponent)"""
    chain = torch.zeros(nch * Lh, 2)
    for e in range(nch * Lh):
        if n[e]:
            chain[e, 0] = l1[e][:n[e]].max()
            if has_bias(e):
                chain[e, 1] = bias[e][:n[e]].abs().max()
    scale, inv = torch.ones(nch, Lh), torch.ones(nch, Lh)
    margin = 1.0
    for c in range(nch):
        bound = float(np.float32(bound0))
        for l in range(Lh):
            bound = (float(chain[c * Lh + l, 0]) * bound + float(chain[c * Lh + l, 1])) * SLACK32
            if bound > 0:
                f, e = math.frexp(bound)
                assert 0.5 * (1 + CHAIN_MARGIN) <= f <= 1 - CHAIN_MARGIN, ("a bound is too close to a power of two: change the seed", nch, Lh, c, l, bound0, f)
                margin = min(margin, 2 * f - 1, 1 - f)
                scale[c, l], inv[c, l] = 2.0 ** (14 - e), 2.0 ** (e - 14)
    return chain.view(nch, Lh, 2), scale, inv, margin


def check_chain_refresh(L, di, stream, tdev):
    """mms_chain_refresh16 over CHAIN_SHAPES x CHAIN_ROWS x CHAIN_BOUND0, the bias array present, NULL, or NULL for every other entry
    (in turn).  chain == the exact maxima bit for bit (the order of a maximum is free); chain_scale / chain_inv == the powers of two of
    the float64 bound recursion for every row; scale inv == 1; NaN guards behind `chain` and behind [nchains, L, rows]; equal to what
    mms_split_planes16_group leaves for rows whose largest magnitude is bound0 (E = 15 and 32 included); bound0 = 0 in front of an entry
    without bias gives scale 1.  Returns every launch's outputs (the two builds agree bit for bit)."""
    res = {}
    turn, margin = 0, 1.0
    for nch, Lh in CHAIN_SHAPES:
        E = nch * Lh
        for rows in CHAIN_ROWS:
            for bound0 in CHAIN_BOUND0:
                form = ("all", "none", "alternate")[turn % 3]
                turn += 1
                n, l1, bias = chain_data(nch, Lh, seed=turn)
                has_bias = {"all": lambda e: True, "none": lambda e: False, "alternate": lambda e: e % 2 == 1}[form]
                want_chain, want_s, want_i, mg = chain_expected(nch, Lh, n, l1, bias, has_bias, bound0)
                margin = min(margin, mg)
                l1d, bd = [t.to(tdev) for t in l1], [t.to(tdev) for t in bias]
                chain = _nan(tdev, 2 * E + GUARD)
                cs, ci = _nan(tdev, E * rows + GUARD), _nan(tdev, E * rows + GUARD)
                barr = None if form == "none" else _ptrs([bd[e] if has_bias(e) else None for e in range(E)])
                p = lambda t: ctypes.c_void_p(t.data_ptr())
                _ok(L, L.mms_chain_refresh16(di, nch, Lh, _ptrs(l1d), barr, _i32(n), p(chain), bound0, rows, p(cs) if rows else None, p(ci) if rows else None, stream),
                    "mms_chain_refresh16")
                _sync(tdev)
                tag = (nch, Lh, rows, bound0, form)
                assert bool(torch.isnan(chain[2 * E:]).all()) and bool(torch.isnan(cs[E * rows:]).all()) and bool(torch.isnan(ci[E * rows:]).all()), ("guards", tag)
                got = chain[:2 * E].view(nch, Lh, 2).cpu()
                assert torch.equal(got.view(torch.int32), want_chain.view(torch.int32)), ("chain", tag, got, want_chain)
                gs, gi = cs[:E * rows].view(nch, Lh, rows).cpu(), ci[:E * rows].view(nch, Lh, rows).cpu()
                assert bool((gs == want_s[..., None]).all()) and bool((gi == want_i[..., None]).all()), ("chain scales", tag, gs[..., :1], want_s)
                assert bool((gs * gi == 1.0).all()), tag
                if bound0 == 0.0:
                    for c in range(nch):
                        if not (has_bias(c * Lh) and n[c * Lh]):
                            assert bool((gs[c, 0] == 1.0).all()), ("bound0 = 0 in front of an entry without bias must give scale 1", tag, c)
                if rows:
                    # the input split on rows whose largest magnitude is bound0
                    K = 40
                    gen = torch.Generator().manual_seed(turn)
                    x = (torch.rand(rows, K, generator=gen) * 2 - 1) * bound0 * 0.9
                    x[:, 3] = bound0
                    xd = x.to(tdev)
                    xp = torch.zeros(_h32(rows, K), dtype=torch.uint8, device=tdev)
                    xs, xi = _nan(tdev, rows), _nan(tdev, rows)
                    cs2, ci2 = _nan(tdev, E * rows + GUARD), _nan(tdev, E * rows + GUARD)
                    _ok(L, L.mms_split_planes16_group(di, 1, rows, K, 0, _ptrs([xd]), _ptrs([xp]), _ptrs([xs]), _ptrs([xi]), nch, Lh, _ptrs([chain]), _ptrs([cs2]), _ptrs([ci2]),
                                                      None, 0.0, stream), "mms_split_planes16_group")
                    _sync(tdev)
                    assert torch.equal(cs2[:E * rows].cpu().view(torch.int32), gs.reshape(-1).view(torch.int32)) and \
                        torch.equal(ci2[:E * rows].cpu().view(torch.int32), gi.reshape(-1).view(torch.int32)), ("the input split's chain", tag)
                    assert bool(torch.isnan(cs2[E * rows:]).all()) and bool(torch.isnan(ci2[E * rows:]).all()), ("the input split's chain guards", tag)
                res[tag] = (got, gs.clone(), gi.clone())
    # (exact outputs: there is no error to report; what is recorded is how much room the inputs leave)
    _report(tdev, "chain_refresh", launches=len(res), closest_bound_to_a_power_of_two=margin)
    return res


# ---- 5. mms_split_planes_group, several groups -------------------------------------------------------------------------------------
def check_split_planes_group(L, di, stream, tdev):
    """mms_split_planes_group with G = 3 at (7, 36), (130, 64), (5, 1028): group 1's x is 4 bytes off a 16-byte boundary, which makes
    the launch split_planes_kernel<false> for all three (and, all aligned, <true>).  Every group's fp32 values are EXACTLY the sum of
    their three bf16 planes, columns past K are zero, the guard behind the last row stays; extremes in row 0."""
    for rows, K in ((7, 36), (130, 64), (5, 1028)):
        KC = (K + 31) // 32
        for shift in (True, False):
            gen = torch.Generator().manual_seed(rows + K)
            xs = [torch.randn(rows, K, generator=gen) * (0.5 + g) for g in range(3)]
            for x in xs:
                x[0, :8] = torch.tensor([0.0, -0.0, 1e-30, -3e38, 1.0 + 2 ** -23, 2 ** -126, 65504.0, -1e-20])
            xd = [_shifted(x, tdev) if (g == 1 and shift) else x.to(tdev).contiguous() for g, x in enumerate(xs)]
            assert xd[1].data_ptr() % 16 == (4 if shift else 0) and xd[0].data_ptr() % 16 == 0
            planes = [torch.full(((rows + GUARD) * KC * 192,), SENT_BYTE, dtype=torch.uint8, device=tdev) for _ in range(3)]
            _ok(L, L.mms_split_planes_group(di, 3, rows, K, 0, _ptrs(xd), _ptrs(planes), stream), "mms_split_planes_group")
            _sync(tdev)
            for g in range(3):
                assert bool((planes[g][rows * KC * 192:] == SENT_BYTE).all()), ("guard", rows, K, g, shift)
                v = planes[g][:rows * KC * 192].cpu().view(torch.bfloat16).view(rows, KC, 3, 32).float()
                back = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]).reshape(rows, KC * 32)
                assert torch.equal(back[:, :K], xs[g]), ("not the sum of its planes", rows, K, g, shift)
                assert bool((v.permute(0, 1, 3, 2).reshape(rows, KC * 32, 3)[:, K:] == 0).all()), ("columns past K", rows, K, g, shift)

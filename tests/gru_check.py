"""Per-entry checks of the grouped GRU cell step (include/mms.h: mms_gru_group) -- one check list for both builds: tests/test_gru.py
runs it on libmms_cpu.so, tests/test_gru_gpu.py on libmms.so.

Every function takes (L, device_index, stream, torch_device) and drives the C ABI through ctypes.  The truth is the closed form of
include/mms.h in float64 on the same fp32 inputs, the yardstick torch's fp32 nn.GRU on the CPU.  Every destination is filled with NaN
before the launch and sits in a block with one guard row behind it and, per layout, guard columns or the other layers / agents of a
state slot around it; all of that must still be poison afterwards.  Each check prints and records (parity.record) its worst observed
error / bound.

The per-element bound (u = 2^-24, the unit roundoff of fp32; everything evaluated in float64 from the magnitudes of the operands):
  A gate's pre-activation a = x . w_i + b_i + hm . w_h + b_h is a sum of K + H products and two biases.  However the K + H + 2 terms
  are ordered, each term takes part in at most K + H + 1 roundings of partial sums and one of its own product (the exact-fp32 MFMA
  rounds a product pair once, an fma none), so  da <= (K + H + 3) u (sum |x||w_i| + sum |hm||w_h| + |b_i| + |b_h|)  to first order.
  For the n gate the two halves are kept apart: da_ni over the x terms and b_in, da_nh over the hm terms and b_hn, the same factor.
  sigmoid' <= 1/4, and the exponential, the addition and the division of its evaluation stay within 4u absolute (a value in (0, 1));
  tanh' <= 1 and its evaluation within 4u likewise (csrc/policy_kernels.hip puts even the fast form at 1e-7 = 1.7u):
      dr, dz <= da / 4 + 4u
      dn     <= da_ni + |n_h| dr + da_nh + 4u         n = tanh(n_i + r n_h), r <= 1; the product and the sum's roundings are in the 4u
      dh'    <= dn + |n - hm| dz + 3u                 h' = n + z (hm - n): |1 - z| <= 1; two products and a sum of values <= 1
The rms gate is the project's (tests/mlp_grad_check.py gate (c)): rms(e) <= max(m rms(e_torch), 2^-24 rms(truth)), m = 1.25 for
1024 or more outputs and 2.0 below -- the spread between two equally good fp32 evaluations."""
import ctypes

import torch

import parity
from massive_marl_benchmark_amd import _lib

U = 2.0 ** -24
LAYOUTS = ("dense", "layers", "agents")


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _ptrs(ps):
    """HOST array of device addresses (None entries: NULL); None: a NULL array"""
    if ps is None:
        return None
    return (ctypes.c_void_p * len(ps))(*ps)


def _sync(tdev):
    if torch.device(tdev).type == "cuda":
        torch.cuda.synchronize()


def _where(tdev):
    return "gpu" if torch.device(tdev).type == "cuda" else "cpu"


def _report(tdev, name, **vals):
    print("%s/gru_%s: %s" % (_where(tdev), name, ", ".join("%s %.3g" % kv for kv in sorted(vals.items()))))
    parity.record("%s/gru_%s" % (_where(tdev), name), **vals)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _slot(layout, M, H):
    """(shape of the block with its guard row, offset of the [M, H] view in floats, its row pitch in floats):
       dense   [M + 1, H + 4]        rows with four guard columns behind them
       layers  [M + 1, 2, H]         layer 1 of an [M, recurrent_N = 2, H] state slot
       agents  [M + 1, 3, 2, H]      agent 1, layer 0 of an [N, agents = 3, recurrent_N = 2, H] slot"""
    if layout == "dense":
        return (M + 1, H + 4), 0, H + 4
    if layout == "layers":
        return (M + 1, 2, H), H, 2 * H
    return (M + 1, 3, 2, H), 2 * H, 6 * H


def _view(block, layout, M, H):
    _, off, pitch = _slot(layout, M, H)
    return block.view(block.shape[0], -1)[:M, off:off + H]


def _source(val, layout, tdev, seed):
    """val [M, H] placed in a block of the layout whose other elements are random numbers (reading one of them gives a wrong result)"""
    M, H = val.shape
    shape, _, _ = _slot(layout, M, H)
    blk = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    _view(blk, layout, M, H).copy_(val)
    return blk.to(tdev)


def _dest(layout, M, H, tdev):
    shape, _, _ = _slot(layout, M, H)
    return torch.full(shape, float("nan"), device=tdev)


def _only_view_written(block, layout, M, H):
    rest = block.clone()
    _view(rest, layout, M, H).fill_(float("nan"))
    return bool(torch.isnan(rest).all())


def make_data(G, M, K, H, seed):
    """G networks with torch's GRU initialisation (uniform in +- 1 / sqrt(H)), inputs ~ N(0, 1), states in (-1, 1), 0 / 1 masks"""
    g = torch.Generator().manual_seed(seed)
    s = 1.0 / H ** 0.5
    uni = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1)
    d = dict(G=G, M=M, K=K, H=H, x=torch.randn(G, M, K, generator=g), h=uni(G, M, H) * 0.999, w_ih=uni(G, 3 * H, K) * s, w_hh=uni(G, 3 * H, H) * s,
             b_ih=uni(G, 3 * H) * s, b_hh=uni(G, 3 * H) * s, mask=(torch.rand(G, M, generator=g) < 0.6).float())
    if M > 1:
        d["mask"][:, 0] = 0.0                                               # at least one row of each kind
        d["mask"][:, 1] = 1.0
    return d


def run(L, di, stream, tdev, d, layout="dense", use_mask=True, with_y=True, rows=None, groups=None, rc_only=False):
    """One mms_gru_group call on rows `rows` (a slice; None: all) of the networks `groups` (a list; None: all) of d, h read from and
    h_out written into blocks of `layout`, x at pitch K + 4, the mask at pitch 3.  Returns (h_out [G, M, H], y [G, M, H] or None) on the
    CPU after checking that nothing but the destinations' views was written."""
    gs = list(range(d["G"])) if groups is None else groups
    sl = slice(0, d["M"]) if rows is None else rows
    K, H = d["K"], d["H"]
    x = [d["x"][g, sl] for g in gs]
    M = x[0].shape[0]
    pad = lambda v: torch.cat([v, torch.randn(1, v.shape[1])])                                        # (a row more: M = 0 still has an address)
    xb = [pad(torch.cat([v, torch.randn(M, 4)], 1)).contiguous().to(tdev) for v in x]                # x_pitch = K + 4
    hb = [_source(d["h"][g, sl], layout, tdev, 100 + i) for i, g in enumerate(gs)]
    mb = [pad(torch.stack([d["mask"][g, sl], torch.full((M,), 0.5), torch.full((M,), 0.5)], 1)).contiguous().to(tdev) for g in gs]   # mask_pitch = 3
    par = {k: [d[k][g].contiguous().to(tdev) for g in gs] for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
    ob = [_dest(layout, M, H, tdev) for _ in gs]
    yb = [torch.full((M + 1, H), float("nan"), device=tdev) for _ in gs]
    _, off, pitch = _slot(layout, M, H)
    addr = lambda ts, o=0: _ptrs([t.data_ptr() + 4 * o for t in ts])
    rc = L.mms_gru_group(di, len(gs), M, K, H, addr(xb), K + 4, addr(hb, off), pitch, addr(mb) if use_mask else None, 3, addr(par["w_ih"]), addr(par["w_hh"]),
                         addr(par["b_ih"]), addr(par["b_hh"]), addr(ob, off), pitch, addr(yb) if with_y else None, stream)
    _sync(tdev)
    if rc_only:
        return rc
    _lib.check(rc, None, "mms_gru_group", L)
    for o, y in zip(ob, yb):
        assert _only_view_written(o, layout, M, H), ("h_out: something outside its [M, H] view was written", layout, M, H)
        assert bool(torch.isnan(y[M:]).all()) and (with_y or bool(torch.isnan(y).all())), ("y: guard row, or y although NULL", layout, M, H)
    out = torch.stack([_view(o, layout, M, H) for o in ob]).cpu() if M else torch.zeros(len(gs), 0, H)
    ys = torch.stack([y[:M] for y in yb]).cpu() if with_y else None
    return out, ys


def truth_and_bound(d, use_mask=True):
    """(h' in float64, the per-element bound of the module docstring), each [G, M, H]"""
    K, H = d["K"], d["H"]
    x, h, wi, wh, bi, bh = (d[k].double() for k in ("x", "h", "w_ih", "w_hh", "b_ih", "b_hh"))
    hm = h * d["mask"].double()[..., None] if use_mask else h
    gi = torch.einsum("gmk,gjk->gmj", x, wi) + bi[:, None]
    gh = torch.einsum("gmk,gjk->gmj", hm, wh) + bh[:, None]
    ai = torch.einsum("gmk,gjk->gmj", x.abs(), wi.abs()) + bi.abs()[:, None]
    ah = torch.einsum("gmk,gjk->gmj", hm.abs(), wh.abs()) + bh.abs()[:, None]
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n_h = gh[..., 2 * H:]
    n = torch.tanh(gi[..., 2 * H:] + r * n_h)
    out = (1 - z) * n + z * hm
    c = (K + H + 3) * U
    dr = c * (ai[..., :H] + ah[..., :H]) / 4 + 4 * U
    dz = c * (ai[..., H:2 * H] + ah[..., H:2 * H]) / 4 + 4 * U
    dn = c * ai[..., 2 * H:] + n_h.abs() * dr + c * ah[..., 2 * H:] + 4 * U
    return out, dn + (n - hm).abs() * dz + 3 * U


def torch_gru(d, use_mask=True):
    """torch's fp32 nn.GRU on the CPU, one step from hxs * masks as rnn.py:25-29 calls it: [G, M, H]"""
    outs = []
    with torch.no_grad():
        for g in range(d["G"]):
            gru = torch.nn.GRU(d["K"], d["H"], num_layers=1)
            for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
                getattr(gru, name.replace("w_", "weight_").replace("b_", "bias_") + "_l0").copy_(d[name][g])
            hm = d["h"][g] * d["mask"][g][:, None] if use_mask else d["h"][g]
            outs.append(gru(d["x"][g][None], hm[None].contiguous())[1][0])
    return torch.stack(outs)


def _rms(t):
    return float(t.pow(2).mean().sqrt())


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------
def check_against_f64(L, di, stream, tdev, H, M, K=None, G=3, layout="layers", label=None):
    """h' of G networks with different data on M rows against float64: the per-element bound and the rms gate of the module docstring;
    y equals h_out bit for bit.  Returns (h_out, bound) for the comparison of the two builds."""
    K = H if K is None else K
    d = make_data(G, M, K, H, seed=7 * H + M + K)
    out, y = run(L, di, stream, tdev, d, layout)
    assert _same_bits(out, y), ("y differs from h_out", H, M, K)
    truth, bound = truth_and_bound(d)
    err = (out.double() - truth).abs()
    assert bool(torch.isfinite(out).all()), ("non-finite output", H, M, K)
    worst = float((err / bound).max())
    yerr = (torch_gru(d).double() - truth).abs()
    n = out.numel()
    m = 1.25 if n >= 1024 else 2.0
    e, ye, fl = _rms(err), _rms(yerr), U * _rms(truth)
    _report(tdev, label or "f64_H%d_M%d_K%d_G%d" % (H, M, K, G), elem_over_bound=worst, rms=e, rms_torch=ye, rms_over_gate=e / max(m * ye, fl),
            max_err=float(err.max()), max_err_torch=float(yerr.max()))
    assert worst <= 1.0, ("per-element bound", H, M, K, worst)
    assert e <= max(m * ye, fl), ("rms gate", H, M, K, e, ye, fl)
    return out, bound


def check_empty(L, di, stream, tdev):
    """M == 0 succeeds and touches nothing"""
    d = make_data(3, 4, 36, 36, seed=5)
    out, _ = run(L, di, stream, tdev, d, "layers", rows=slice(0, 0))
    assert out.shape[1] == 0


# ---- 2. masks ------------------------------------------------------------------------------------------------------------------------
def check_masks(L, di, stream, tdev, H=36, M=130):
    """Random 0 / 1 masks: the call with masks equals, bit for bit, the call with the masked rows of h zeroed and mask = NULL -- on the
    rows with mask 0 (what include/mms.h promises) and on the others (1 * h = h)."""
    d = make_data(3, M, H, H, seed=11)
    a, _ = run(L, di, stream, tdev, d, "layers", use_mask=True)
    z = dict(d)
    z["h"] = d["h"] * d["mask"][..., None]
    b, _ = run(L, di, stream, tdev, z, "layers", use_mask=False)
    off = d["mask"] == 0
    assert int(off.sum()) > 0 and int((~off).sum()) > 0
    assert _same_bits(a[off], b[off]), "rows with mask 0 differ from rows of a zero state"
    assert _same_bits(a, b), "rows with mask 1 differ from the unmasked call"
    plain, _ = run(L, di, stream, tdev, d, "layers", use_mask=False)
    assert not _same_bits(a[off], plain[off]), "the mask changed nothing"


# ---- 3. pitches ----------------------------------------------------------------------------------------------------------------------
def check_pitches(L, di, stream, tdev, H=36, M=7):
    """h read from / h_out written into layer 1 of an [M, 2, H] block and agent 1, layer 0 of an [M, 3, 2, H] block give the bits of
    the dense rows (run() asserts that every other element of the blocks, the guard rows and a NULL y stay poison)."""
    d = make_data(3, M, H, H, seed=13)
    dense, y = run(L, di, stream, tdev, d, "dense")
    assert _same_bits(dense, y)
    for layout in ("layers", "agents"):
        got, y = run(L, di, stream, tdev, d, layout, with_y=(layout == "layers"))
        assert _same_bits(got, dense), layout
        assert y is None or _same_bits(y, dense), layout


# ---- 4. row independence, determinism ----------------------------------------------------------------------------------------------------
def check_rows_independent(L, di, stream, tdev, H=100):
    """Rows 5 .. 11 of network 1: alone (M = 7), inside M = 130 at rows 40 .. 46, and as network 17 of 32 -- the same bits; two runs
    of one call -- the same bits."""
    d = make_data(3, 130, H, H, seed=17)
    alone, _ = run(L, di, stream, tdev, d, "dense", rows=slice(5, 12), groups=[1])
    moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    for k in ("x", "h", "mask"):
        moved[k][1, 40:47] = d[k][1, 5:12]
    inside, _ = run(L, di, stream, tdev, moved, "layers")
    assert _same_bits(inside[1, 40:47], alone[0]), "a row's result depends on M or on where the row sits"
    many = [g % 3 for g in range(32)]
    many[17] = 1
    wide, _ = run(L, di, stream, tdev, d, "agents", rows=slice(0, 33), groups=many)
    assert _same_bits(wide[17, 5:12], alone[0]), "a row's result depends on the number of groups"
    again, _ = run(L, di, stream, tdev, moved, "layers")
    assert _same_bits(again, inside), "two runs of one call differ"


# ---- 5. contract -------------------------------------------------------------------------------------------------------------------------
def check_contract(L, di, stream, tdev):
    """Each bad call returns non-zero, names the entry in mms_last_error and leaves the poisoned destinations as they were."""
    M, K, H = 8, 8, 8
    t = lambda *s: torch.randn(*s).to(tdev)
    x, h, mask, wi, wh, bi, bh = t(M, K), t(M, H), t(M), t(3 * 1028, K), t(3 * 1028, 1028), t(3 * 1028), t(3 * 1028)
    out = torch.full((M + 1, 1028), float("nan"), device=tdev)
    y = torch.full((M + 1, 1028), float("nan"), device=tdev)
    big_x, big_h = t(M, 1028), t(M, 1028)
    one = lambda v, n=1: _ptrs([v.data_ptr()] * n)

    def call(groups=1, M=M, K=K, H=H, x=x, xp=None, h=h, hp=None, mask=mask, mp=1, wi=wi, wh=wh, bi=bi, bh=bh, out=out, op=None, y=y, n=None):
        n = max(groups, 1) if n is None else n
        arr = lambda v: None if v is None else (v if isinstance(v, ctypes.Array) else one(v, n))
        return L.mms_gru_group(di, groups, M, K, H, arr(x), K if xp is None else xp, arr(h), H if hp is None else hp, arr(mask), mp, arr(wi), arr(wh),
                               arr(bi), arr(bh), arr(out), 1028 if op is None else op, arr(y), stream)

    bad = {
        "h_out == h": dict(out=h, op=H),
        "h_out == x": dict(out=x, op=K),
        "y == h": dict(y=h),
        "H % 4 != 0": dict(H=6, hp=8),
        "K % 4 != 0": dict(K=6, xp=8),
        "H > 1024": dict(H=1028, x=big_x, xp=1028, K=1028, h=big_h, hp=1028),
        "groups == 0": dict(groups=0),
        "groups == 33": dict(groups=33),
        "two groups, one destination": dict(groups=2),
        "x NULL": dict(x=None),
        "h NULL": dict(h=None),
        "w_ih NULL": dict(wi=None),
        "w_hh NULL": dict(wh=None),
        "b_ih NULL": dict(bi=None),
        "b_hh NULL": dict(bh=None),
        "h_out NULL": dict(out=None),
        "a NULL entry": dict(x=_ptrs([None])),
        "a NULL mask entry": dict(mask=_ptrs([None])),
        "odd h_pitch": dict(hp=H + 1),
        "odd x_pitch": dict(xp=K + 1),
        "odd h_out_pitch": dict(op=1027),
        "h_pitch < H": dict(hp=4),
        "M < 0": dict(M=-1),
        "misaligned x": dict(x=_ptrs([x.data_ptr() + 4])),
    }
    for name, kw in bad.items():
        rc = call(**kw)
        _sync(tdev)
        assert rc != 0, name
        assert "mms_gru_group" in _lib.last_error(None, L), (name, _lib.last_error(None, L))
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(y).all()), ("written on error", name)
    assert L.mms_gru_group(-1 if di >= 0 else 0, 1, M, K, H, one(x), K, one(h), H, one(mask), 1, one(wi), one(wh), one(bi), one(bh), one(out), 1028, one(y), stream) != 0
    assert bool(torch.isnan(out).all())
    _lib.check(call(), None, "mms_gru_group", L)                                            # ... and the good call of the same arguments
    _lib.check(call(mask=None, y=None), None, "mms_gru_group without mask and y", L)
    _lib.check(call(y=_ptrs([None])), None, "mms_gru_group with a NULL y entry", L)
    _sync(tdev)
    assert bool(torch.isfinite(out[:M, :H]).all()) and bool(torch.isnan(out[:M, H:]).all()) and bool(torch.isnan(out[M:]).all())


# ---- 6. the layers in front of the GRU: mms_linear_group_act with blocked summation (act + 16) ------------------------------------------------
def check_linear_blocked(L, di, stream, tdev, M, N, K, G=3):
    """y = ELU(x w^T + b) with act = 1 + 16 (include/mms.h: every 32 k summed from zero where the generic kernel runs) at shapes that
    take the generic kernel, against float64: per element |e| <= (K + 2) u (sum |x||w| + |b|) + 4u (the ordering-free bound of the
    module docstring; ELU' <= 1, its expm1 within 4u), the rms gate against torch's fp32 Linear + ELU on the CPU, and no worse in rms
    than 1.25 x the plain chain (act = 1) on the same data; the guard row stays poison.  Returns the rms ratio blocked / plain."""
    g = torch.Generator().manual_seed(3 * M + N + K)
    x = torch.randn(G, M, K, generator=g) * 2
    w = (torch.rand(G, N, K, generator=g) * 2 - 1) / K ** 0.5
    b = torch.randn(G, N, generator=g) * 0.1
    xd, wd, bd = ([t[i].contiguous().to(tdev) for i in range(G)] for t in (x, w, b))
    dev = lambda ts: _ptrs([t.data_ptr() for t in ts])
    outs = {}
    for act in (17, 1):
        y = [torch.full((M + 1, N), float("nan"), device=tdev) for _ in range(G)]
        _lib.check(L.mms_linear_group_act(di, G, M, N, K, dev(xd), dev(wd), dev(bd), dev(y), act, None, None, None, stream), None, "mms_linear_group_act", L)
        _sync(tdev)
        assert all(bool(torch.isnan(t[M:]).all()) for t in y), "guard row written"
        outs[act] = torch.stack([t[:M] for t in y]).cpu()
    pre = torch.einsum("gmk,gnk->gmn", x.double(), w.double()) + b.double()[:, None]
    truth = torch.nn.functional.elu(pre)
    bound = (K + 2) * U * (torch.einsum("gmk,gnk->gmn", x.double().abs(), w.double().abs()) + b.double().abs()[:, None]) + 4 * U
    yard = torch.nn.functional.elu(torch.einsum("gmk,gnk->gmn", x, w) + b[:, None])
    err, plain, yerr = (outs[17].double() - truth).abs(), (outs[1].double() - truth).abs(), (yard.double() - truth).abs()
    worst = float((err / bound).max())
    m = 1.25 if truth.numel() >= 1024 else 2.0
    e, pe, ye, fl = _rms(err), _rms(plain), _rms(yerr), U * _rms(truth)
    _report(tdev, "linear_blocked_M%d_N%d_K%d" % (M, N, K), elem_over_bound=worst, rms=e, rms_plain=pe, rms_torch=ye, rms_over_gate=e / max(m * ye, fl))
    assert worst <= 1.0 and e <= max(m * ye, fl) and e <= 1.25 * pe, (M, N, K, worst, e, pe, ye)
    assert L.mms_linear_group_act(di, G, M, N, K, dev(xd), dev(wd), dev(bd), dev(y), 20, None, None, None, stream) != 0      # 4 + 16: no such activation
    return e / pe


# ---- 7. the two builds ---------------------------------------------------------------------------------------------------------------------
def builds_agree(gpu, cpu):
    """(h_out, bound) of check_against_f64 from both builds on the same data: each lies within the bound of the truth, so they differ by
    at most the sum of the two bounds.  Returns the worst difference / that sum."""
    (a, ba), (b, bb) = gpu, cpu
    worst = float(((a.double() - b.double()).abs() / (ba + bb)).max())
    assert worst <= 1.0, worst
    return worst

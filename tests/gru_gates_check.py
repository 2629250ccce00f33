"""Per-entry checks of the unfused GRU gate step (include/mms.h: mms_gru_gates_group) -- one check list for both builds:
tests/test_gru_gates.py runs it on libmms_cpu.so, tests/test_gru_gates_gpu.py on libmms.so.

Every function takes (L, device_index, stream, torch_device) and drives the C ABI through ctypes.  The truth is the closed form of
include/mms.h in float64 on the same fp32 gi, gh, h, b_hh and mask.  gi and gh sit in blocks of pitch 3H + 4 with random filler behind
every row, the mask at pitch 3, h and h_out in the state-slot layouts of tests/gru_check.py (_slot); every destination is filled with
NaN before the launch and has a guard row behind it, and all of that must still be poison afterwards.  Each check prints and records
(parity.record) its worst observed error / bound.

The per-element bound (u = 2^-24; evaluated in float64 from the magnitudes of the operands), derived as tests/gru_check.py derives its own:
  A gate's pre-activation is here two additions of GIVEN numbers, gi + ((m gh) + b_hh) -- m gh is exact for a 0 / 1 mask, and + 0 is --,
  so  da <= 2u (|gi| + |m gh| + |b_hh|)  to first order, for each of r, z and n (for n the inner sum a_n = m gh_n + b_n takes one of the two
  roundings, the outer one gi_n + r a_n the other; the rounding of the product r a_n is in the 4u below, as in gru_check.py).
  sigmoid' <= 1/4 and its evaluation stays within 4u absolute; tanh' <= 1 and its evaluation within 4u likewise:
      dr, dz <= da / 4 + 4u
      dn     <= da_n + |a_n| dr + 4u                  n = tanh(gi_n + r a_n), r <= 1
      dh'    <= dn + |n - hm| dz + 3u                 h' = n + z (hm - n): |1 - z| <= 1; two products and a sum of values <= 1"""
import ctypes

import torch

import gru_check as gk
import parity
from massive_marl_benchmark_amd import _lib

U = gk.U
LAYOUTS = gk.LAYOUTS
SHAPES = ((4, 1), (36, 7), (36, 130), (128, 128), (512, 130))         # (H, M): one thread per row, a ragged last block, more than one block each way
_ptrs, _sync, _same_bits, _slot, _view, _source, _dest, _only_view_written = (gk._ptrs, gk._sync, gk._same_bits, gk._slot, gk._view, gk._source, gk._dest,
                                                                              gk._only_view_written)


def _report(tdev, name, **vals):
    print("%s/gru_gates_%s: %s" % (gk._where(tdev), name, ", ".join("%s %.3g" % kv for kv in sorted(vals.items()))))
    parity.record("%s/gru_gates_%s" % (gk._where(tdev), name), **vals)


def make_data(G, M, H, seed):
    """Pre-activations of the size a GRU behind a LayerNorm produces (gi ~ N(0, 1), gh ~ N(0, 0.6)), states in (-1, 1), torch's bias
    initialisation, 0 / 1 masks with at least one row of each kind"""
    g = torch.Generator().manual_seed(seed)
    uni = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1)
    d = dict(G=G, M=M, H=H, gi=torch.randn(G, M, 3 * H, generator=g), gh=torch.randn(G, M, 3 * H, generator=g) * 0.6, h=uni(G, M, H) * 0.999,
             b_hh=uni(G, 3 * H) / H ** 0.5, mask=(torch.rand(G, M, generator=g) < 0.6).float())
    if M > 1:
        d["mask"][:, 0] = 0.0
        d["mask"][:, 1] = 1.0
    return d


def run(L, di, stream, tdev, d, layout="dense", out_layout=None, use_mask=True, with_y=True, rows=None, groups=None):
    """One mms_gru_gates_group call on rows `rows` (a slice; None: all) of the networks `groups` (a list; None: all) of d: h read from a
    block of `layout`, h_out written into one of `out_layout` (None: the same), gi / gh at pitch 3H + 4, the mask at pitch 3.  Returns
    (h_out [G, M, H], y [G, M, H] or None) on the CPU after checking that nothing but the destinations' views was written."""
    out_layout = layout if out_layout is None else out_layout
    gs = list(range(d["G"])) if groups is None else groups
    sl = slice(0, d["M"]) if rows is None else rows
    H = d["H"]
    M = d["h"][gs[0], sl].shape[0]
    pad = lambda v: torch.cat([v, torch.randn(1, v.shape[1])])                                        # (a row more: M = 0 still has an address)
    wide = lambda v: pad(torch.cat([v, torch.randn(M, 4)], 1)).contiguous().to(tdev)                  # g_pitch = 3H + 4, filler behind every row
    gib, ghb = [wide(d["gi"][g, sl]) for g in gs], [wide(d["gh"][g, sl]) for g in gs]
    hb = [_source(d["h"][g, sl], layout, tdev, 100 + i) for i, g in enumerate(gs)]
    mb = [pad(torch.stack([d["mask"][g, sl], torch.full((M,), 0.5), torch.full((M,), 0.5)], 1)).contiguous().to(tdev) for g in gs]   # mask_pitch = 3
    bh = [d["b_hh"][g].contiguous().to(tdev) for g in gs]
    ob = [_dest(out_layout, M, H, tdev) for _ in gs]
    yb = [torch.full((M + 1, H), float("nan"), device=tdev) for _ in gs]
    _, off, pitch = _slot(layout, M, H)
    _, ooff, opitch = _slot(out_layout, M, H)
    addr = lambda ts, o=0: _ptrs([t.data_ptr() + 4 * o for t in ts])
    rc = L.mms_gru_gates_group(di, len(gs), M, H, addr(gib), addr(ghb), 3 * H + 4, addr(hb, off), pitch, addr(mb) if use_mask else None, 3, addr(bh),
                               addr(ob, ooff), opitch, addr(yb) if with_y else None, stream)
    _sync(tdev)
    _lib.check(rc, None, "mms_gru_gates_group", L)
    for o, y in zip(ob, yb):
        assert _only_view_written(o, out_layout, M, H), ("h_out: something outside its [M, H] view was written", out_layout, M, H)
        assert bool(torch.isnan(y[M:]).all()) and (with_y or bool(torch.isnan(y).all())), ("y: guard row, or y although NULL", M, H)
    out = torch.stack([_view(o, out_layout, M, H) for o in ob]).cpu() if M else torch.zeros(len(gs), 0, H)
    ys = torch.stack([y[:M] for y in yb]).cpu() if with_y else None
    return out, ys


def truth_and_bound(d, use_mask=True):
    """(h' in float64, the per-element bound of the module docstring), each [G, M, H]"""
    H = d["H"]
    gi, gh, h, b = (d[k].double() for k in ("gi", "gh", "h", "b_hh"))
    m = d["mask"].double()[..., None] if use_mask else torch.ones_like(h[..., :1])
    hm, ghm = m * h, m * gh
    a = ghm + b[:, None]
    mag = gi.abs() + ghm.abs() + b.abs()[:, None]
    r = torch.sigmoid(gi[..., :H] + a[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + a[..., H:2 * H])
    a_n = a[..., 2 * H:]
    n = torch.tanh(gi[..., 2 * H:] + r * a_n)
    out = (1 - z) * n + z * hm
    da = 2 * U * mag
    dr = da[..., :H] / 4 + 4 * U
    dz = da[..., H:2 * H] / 4 + 4 * U
    dn = da[..., 2 * H:] + a_n.abs() * dr + 4 * U
    return out, dn + (n - hm).abs() * dz + 3 * U


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------
def check_against_f64(L, di, stream, tdev, H, M, G=3, layout="layers"):
    """h' of G networks with different data on M rows against float64 under the per-element bound; y equals h_out bit for bit.
    Returns (h_out, bound) for the comparison of the two builds."""
    d = make_data(G, M, H, seed=7 * H + M)
    out, y = run(L, di, stream, tdev, d, layout)
    assert _same_bits(out, y), ("y differs from h_out", H, M)
    assert bool(torch.isfinite(out).all()), ("non-finite output", H, M)
    truth, bound = truth_and_bound(d)
    err = (out.double() - truth).abs()
    worst = float((err / bound).max())
    _report(tdev, "f64_H%d_M%d_G%d" % (H, M, G), elem_over_bound=worst, rms=gk._rms(err), max_err=float(err.max()))
    assert worst <= 1.0, ("per-element bound", H, M, worst)
    return out, bound


def check_empty(L, di, stream, tdev):
    """M == 0 succeeds and touches nothing (run() asserts the poison)"""
    d = make_data(3, 4, 36, seed=5)
    out, _ = run(L, di, stream, tdev, d, "layers", rows=slice(0, 0))
    assert out.shape[1] == 0


# ---- 2. layouts ----------------------------------------------------------------------------------------------------------------------
def check_layouts(L, di, stream, tdev, H=36, M=7):
    """h read from and h_out written into every pair of the dense / layers / agents layouts give the bits of the dense call (run()
    asserts that every other element of the blocks, the guard rows and a NULL y stay poison)."""
    d = make_data(3, M, H, seed=13)
    dense, y = run(L, di, stream, tdev, d, "dense")
    assert _same_bits(dense, y)
    for src in LAYOUTS:
        for dst in LAYOUTS:
            got, y = run(L, di, stream, tdev, d, src, dst, with_y=(src != "agents"))
            assert _same_bits(got, dense), (src, dst)
            assert y is None or _same_bits(y, dense), (src, dst)


# ---- 3. masks ------------------------------------------------------------------------------------------------------------------------
def check_masks(L, di, stream, tdev, H=36, M=130):
    """The call with a random 0 / 1 mask equals, bit for bit, the call with mask = NULL on data whose masked rows of h and gh are zero;
    it differs from the unmasked call on the masked rows."""
    d = make_data(3, M, H, seed=11)
    a, _ = run(L, di, stream, tdev, d, "layers", use_mask=True)
    z = dict(d)
    z["h"], z["gh"] = d["h"] * d["mask"][..., None], d["gh"] * d["mask"][..., None]
    b, _ = run(L, di, stream, tdev, z, "layers", use_mask=False)
    off = d["mask"] == 0
    assert int(off.sum()) > 0 and int((~off).sum()) > 0
    assert _same_bits(a[off], b[off]), "rows with mask 0 differ from rows of a zero state with zero gh"
    assert _same_bits(a, b), "rows with mask 1 differ from the unmasked call"
    plain, _ = run(L, di, stream, tdev, d, "layers", use_mask=False)
    assert _same_bits(a[~off], plain[~off])
    assert not _same_bits(a[off], plain[off]), "the mask changed nothing"


# ---- 4. row independence, determinism ----------------------------------------------------------------------------------------------------
def check_rows_independent(L, di, stream, tdev, H=100):
    """Rows 5 .. 11 of network 1: alone (M = 7), inside M = 130 at rows 40 .. 46, and as network 17 of 32 -- the same bits; two runs
    of one call -- the same bits."""
    d = make_data(3, 130, H, seed=17)
    alone, _ = run(L, di, stream, tdev, d, "dense", rows=slice(5, 12), groups=[1])
    moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    for k in ("gi", "gh", "h", "mask"):
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
    """Each bad call returns non-zero, names the entry in mms_last_error and leaves the poisoned destinations as they were; the good
    call with the same arguments succeeds."""
    M, H, W = 8, 8, 1028
    t = lambda *s: torch.randn(*s).to(tdev)
    gi, gh, h, mask, bh = t(M, 3 * W), t(M, 3 * W), t(M, W), t(M), t(3 * W)
    out = torch.full((M + 1, W), float("nan"), device=tdev)
    y = torch.full((M + 1, W), float("nan"), device=tdev)
    one = lambda v, n=1: _ptrs([v.data_ptr()] * n)

    def call(groups=1, M=M, H=H, gi=gi, gh=gh, gp=3 * W, h=h, hp=W, mask=mask, mp=1, bh=bh, out=out, op=W, y=y, n=None, dev=di):
        n = max(groups, 1) if n is None else n
        arr = lambda v: None if v is None else (v if isinstance(v, ctypes.Array) else one(v, n))
        return L.mms_gru_gates_group(dev, groups, M, H, arr(gi), arr(gh), gp, arr(h), hp, arr(mask), mp, arr(bh), arr(out), op, arr(y), stream)

    bad = {
        "h_out == h": dict(out=h),
        "h_out == gi": dict(out=gi, op=3 * W),
        "h_out == gh": dict(out=gh, op=3 * W),
        "y == h": dict(y=h),
        "y == gi": dict(y=gi),
        "y == gh": dict(y=gh),
        "y == h_out": dict(y=out),
        "two groups, one destination": dict(groups=2),
        "gi NULL": dict(gi=None),
        "gh NULL": dict(gh=None),
        "h NULL": dict(h=None),
        "b_hh NULL": dict(bh=None),
        "h_out NULL": dict(out=None),
        "a NULL gi entry": dict(gi=_ptrs([None])),
        "a NULL b_hh entry": dict(bh=_ptrs([None])),
        "a NULL h_out entry": dict(out=_ptrs([None])),
        "a NULL mask entry": dict(mask=_ptrs([None])),
        "g_pitch < 3H": dict(gp=3 * H - 4),
        "odd g_pitch": dict(gp=3 * W + 1),
        "h_pitch < H": dict(hp=4),
        "odd h_pitch": dict(hp=W + 1),
        "h_out_pitch < H": dict(op=4),
        "odd h_out_pitch": dict(op=W - 1),
        "mask_pitch 0": dict(mp=0),
        "H % 4 != 0": dict(H=6),
        "H == 0": dict(H=0),
        "H > 1024": dict(H=W),
        "groups == 0": dict(groups=0),
        "groups == 33": dict(groups=33),
        "misaligned gi": dict(gi=_ptrs([gi.data_ptr() + 4])),
        "misaligned b_hh": dict(bh=_ptrs([bh.data_ptr() + 4])),
        "misaligned h_out": dict(out=_ptrs([out.data_ptr() + 8])),
        "M < 0": dict(M=-1),
        "bad device": dict(dev=-1 if di >= 0 else 0),
    }
    for name, kw in bad.items():
        rc = call(**kw)
        _sync(tdev)
        assert rc != 0, name
        if name != "bad device":                                                            # (that one is the build's own device check)
            assert "mms_gru_gates_group" in _lib.last_error(None, L), (name, _lib.last_error(None, L))
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(y).all()), ("written on error", name)
    _lib.check(call(), None, "mms_gru_gates_group", L)                                      # ... and the good call of the same arguments
    _lib.check(call(mask=None, y=None), None, "mms_gru_gates_group without mask and y", L)
    _lib.check(call(y=_ptrs([None])), None, "mms_gru_gates_group with a NULL y entry", L)
    _sync(tdev)
    assert bool(torch.isfinite(out[:M, :H]).all()) and bool(torch.isnan(out[:M, H:]).all()) and bool(torch.isnan(out[M:]).all())
    assert bool(torch.isfinite(y.view(-1)[:M * H]).all()) and bool(torch.isnan(y.view(-1)[M * H:]).all())


# ---- 6. the two builds ---------------------------------------------------------------------------------------------------------------------
builds_agree = gk.builds_agree

"""Per-entry checks of the GRU gate backward (include/mms.h: mms_gru_gates_grad_group) -- one check list for both builds:
tests/test_gru_grad.py runs it on libmms_cpu.so, tests/test_gru_grad_gpu.py on libmms.so.

Every function takes (L, device_index, stream, torch_device) and drives the C ABI through ctypes.  The data are tests/gru_gates_check.py's
(make_data) with two incoming gradients ~ N(0, 1) added, and its discipline: gi and gh sit in blocks of pitch 3H + 4 with random filler
behind every row, the mask at pitch 3, h, dh_out and dh in the state-slot layouts of tests/gru_check.py (_slot), dy at pitch H + 4, dgi
and dgh at pitch 3H + 8; every destination is filled with NaN before the launch and has a guard row (dbias: four guard floats, the
workspace: 256 guard bytes) behind it, and all of that must still be poison afterwards.  The truth is the closed form of include/mms.h in
float64 on the same fp32 inputs (closed_form), the yardstick the same closed form in fp32 torch operations.  Each check prints and
records (parity.record) its worst observed error / bound and both Frobenius errors.

Gate (a), the per-element bound (u = 2^-24; first order, evaluated in float64 from the magnitudes of the operands).  From
tests/gru_gates_check.py, for the recomputed forward values:
      da_* <= 2u (|gi_*| + |m gh_*| + |b_*|)      dr, dz <= da / 4 + 4u      dn <= da_n + |a_n| dr + 4u      |d a_n| <= u |a_n|
hm = m h is exact for a 0 / 1 mask.  G = dh_out + dy is one addition: dG <= u |G|.  A product of k factors written as k - 1 fp32
multiplications adds (k - 1) u of its own value; a difference 1 - x adds u |1 - x|.  With A = 1 - z, B = 1 - n^2, D = hm - n,
S = z (1 - z), R = r (1 - r):
      dA <= dz + u A          dB <= 2 |n| dn + u (n^2 + B) = 2 |n| dn + u          dD <= dn + u |D|
      dS <= A dz + z (dz + u A) + u S = dz + 2u S      (A + z = 1)                 dR <= dr + 2u R
  dpn = (G A) B:              e_pn <= 4u |dpn| + |G| B dz + |G| A (2 |n| dn + u)                  (u from G, u from A, two products)
  dpz = (G D) S:              e_pz <= 6u |dpz| + |G| S dn + |G D| dz                              (u G, u D, 2u S, two products)
  dpr = (dpn a_n) R:          e_pr <= |a_n| R e_pn + 5u |dpr| + |dpn a_n| dr                      (u a_n, 2u R, two products)
  r dpn:                      e_rn <= r e_pn + |dpn| dr + u |r dpn|
  dgi = [dpr | dpz | dpn]: those; dgh = m [dpr | dpz | r dpn] + 0: m times those (the product with a 0 / 1 mask and + 0 are exact)
  dh = m (G z):               e_h  <= m (2u |G z| + |G| dz)
  dbias_c = sum over rows, in double, rounded once: the sum of the rows' bounds + u |dbias_c|  (the double additions, 2^-53 each, vanish
  under the rows' own 4u or more)
Gate (b), so that a loose bound cannot hide a wrong formula: the relative Frobenius error against float64 is at most twice that of the
closed form in fp32 torch operations on the same inputs (the margin of tests/sac_grad_check.py: two fp32 evaluations that round in
different places).

Shapes (H, M) and the edge each one hits (csrc/gru_grad_lane.h: P = 256 / (H / 4) rows in flight, chunks of max(8 P, ceil(M / 256)) rows):
  (4, 1)        one item per row, one row: 255 idle threads                 (36, 7)      H / 4 = 9 does not divide 256 (four idle threads), one ragged pass
  (36, 130)     P = 28: five passes, the last with 18 rows                  (128, 128)   P = 8, chunks of 64: two full chunks
  (512, 130)    P = 2, chunks of 16: nine chunks, the last with 2 rows      (36, 300)    chunks of 224: two, the last with 76 rows = 2 passes + 20
  (1024, 2060)  one row in flight; past the cap of 256 chunks: chunks of 9 rows instead of 8, 229 of them, the last with 8 rows -- and
                the finish pass's lanes read four partials each (one network: the blocks are 25 MB each)"""
import ctypes

import torch

import gru_check as gk
import gru_gates_check as gg
import parity
from massive_marl_benchmark_amd import _lib

U = gk.U
LAYOUTS = gk.LAYOUTS
SHAPES = gg.SHAPES + ((36, 300),)
BIG = (1024, 2060)
OUTS = ("dgi", "dgh", "dh", "dbias")
_ptrs, _sync, _same_bits, _slot, _view, _source, _dest, _only_view_written = (gk._ptrs, gk._sync, gk._same_bits, gk._slot, gk._view, gk._source, gk._dest,
                                                                              gk._only_view_written)
ENTRY = "mms_gru_gates_grad_group"


def _report(tdev, name, **vals):
    print("%s/gru_grad_%s: %s" % (gk._where(tdev), name, ", ".join("%s %.3g" % kv for kv in sorted(vals.items()))))
    parity.record("%s/gru_grad_%s" % (gk._where(tdev), name), **vals)


def make_data(G, M, H, seed):
    """gru_gates_check.make_data and the two incoming gradients of h'"""
    d = gg.make_data(G, M, H, seed)
    g = torch.Generator().manual_seed(seed + 1000003)
    d["dh_out"], d["dy"] = torch.randn(G, M, H, generator=g), torch.randn(G, M, H, generator=g)
    return d


def workspace(L, di, groups, M, H, tdev):
    """(the queried size, a 256-byte aligned workspace of exactly that size with 256 guard bytes of 0xA5 behind it, its address)"""
    need = ctypes.c_int64(-1)
    _lib.check(L.mms_gru_gates_grad_group(di, groups, M, H, *([None, None, 0] + [None, 0] * 2 + [None, None, 0, None, 0, None, None, 0, None, 0, None]), None,
                                          ctypes.byref(need), None), None, ENTRY + " (size query)", L)
    assert need.value >= 0 and need.value % 256 == 0, need.value
    buf = torch.full((need.value + 512,), 0xA5, dtype=torch.uint8, device=tdev)
    base = (buf.data_ptr() + 255) // 256 * 256
    return need.value, buf, base


def _guard_intact(buf, base, need):
    off = base - buf.data_ptr() + need
    return bool((buf[off:off + 256] == 0xA5).all())


def run(L, di, stream, tdev, d, layout="layers", use_mask=True, use_dy=True, with_bias=True, rows=None, groups=None, dy_null=(), bias_null=()):
    """One mms_gru_gates_grad_group call on rows `rows` (a slice; None: all) of the networks `groups` (a list; None: all) of d.  h is read from
    a block of `layout`, dh_out from and dh into blocks of the next layout of LAYOUTS; dy_null / bias_null: positions whose dy / dbias entry
    is NULL.  Returns {dgi, dgh [G, M, 3H], dh [G, M, H], dbias [G, 4H] (None without; NaN rows where the entry was NULL)} on the CPU after
    checking that nothing but the destinations' views was written."""
    other = LAYOUTS[(LAYOUTS.index(layout) + 1) % 3]
    gs = list(range(d["G"])) if groups is None else groups
    sl = slice(0, d["M"]) if rows is None else rows
    H = d["H"]
    M = d["h"][gs[0], sl].shape[0]
    n = len(gs)
    pad = lambda v: torch.cat([v, torch.randn(1, v.shape[1])])                                        # (a row more: M = 0 still has an address)
    wide = lambda v, w=4: pad(torch.cat([v, torch.randn(M, w)], 1)).contiguous().to(tdev)             # filler behind every row
    gib, ghb = [wide(d["gi"][g, sl]) for g in gs], [wide(d["gh"][g, sl]) for g in gs]
    hb = [_source(d["h"][g, sl], layout, tdev, 100 + i) for i, g in enumerate(gs)]
    gob = [_source(d["dh_out"][g, sl], other, tdev, 200 + i) for i, g in enumerate(gs)]
    gyb = [wide(d["dy"][g, sl]) for g in gs]                                                          # dy_pitch = H + 4
    mb = [pad(torch.stack([d["mask"][g, sl], torch.full((M,), 0.5), torch.full((M,), 0.5)], 1)).contiguous().to(tdev) for g in gs]   # mask_pitch = 3
    bh = [d["b_hh"][g].contiguous().to(tdev) for g in gs]
    nan = lambda *s: torch.full(s, float("nan"), device=tdev)
    dgib, dghb = [nan(M + 1, 3 * H + 8) for _ in gs], [nan(M + 1, 3 * H + 8) for _ in gs]
    dhb = [_dest(other, M, H, tdev) for _ in gs]
    dbb = [nan(4 * H + 4) for _ in gs]
    _, off, pitch = _slot(layout, M, H)
    _, ooff, opitch = _slot(other, M, H)
    addr = lambda ts, o=0, null=(): _ptrs([None if i in null else t.data_ptr() + 4 * o for i, t in enumerate(ts)])
    need, ws, base = workspace(L, di, n, M, H, tdev)
    size = ctypes.c_int64(need)
    rc = L.mms_gru_gates_grad_group(di, n, M, H, addr(gib), addr(ghb), 3 * H + 4, addr(hb, off), pitch, addr(mb) if use_mask else None, 3, addr(bh),
                                    addr(gob, ooff), opitch, addr(gyb, 0, dy_null) if use_dy else None, H + 4, addr(dgib), addr(dghb), 3 * H + 8,
                                    addr(dhb, ooff), opitch, addr(dbb, 0, bias_null) if with_bias else None, ctypes.c_void_p(base), ctypes.byref(size), stream)
    _sync(tdev)
    _lib.check(rc, None, ENTRY, L)
    assert _guard_intact(ws, base, need), "written behind the workspace"
    for i in range(n):
        assert _only_view_written(dhb[i], other, M, H), ("dh: something outside its [M, H] view was written", other, M, H)
        for blk in (dgib[i], dghb[i]):
            assert bool(torch.isnan(blk[M:]).all()) and bool(torch.isnan(blk[:, 3 * H:]).all()), ("dgi / dgh: guard row or the columns behind a row", M, H)
        none = not with_bias or i in bias_null or M == 0
        assert bool(torch.isnan(dbb[i][0 if none else 4 * H:]).all()), ("dbias: guard, or written although NULL", M, H)
    cpu = lambda ts, w: torch.stack([t[:M, :w] for t in ts]).cpu()
    return dict(dgi=cpu(dgib, 3 * H), dgh=cpu(dghb, 3 * H), dh=torch.stack([_view(o, other, M, H) for o in dhb]).cpu() if M else torch.zeros(n, 0, H),
                dbias=torch.stack([t[:4 * H] for t in dbb]).cpu() if with_bias else None)


def closed_form(d, dtype=torch.float64, use_mask=True, use_dy=True, bounds=False):
    """include/mms.h's closed form in torch operations of `dtype`: {dgi, dgh, dh, dbias}; bounds=True (float64 only): also the bounds of
    the module docstring, as a second dict"""
    H = d["H"]
    gi, gh, h, b, go, gy = (d[k].to(dtype) for k in ("gi", "gh", "h", "b_hh", "dh_out", "dy"))
    m = d["mask"].to(dtype)[..., None] if use_mask else torch.ones_like(h[..., :1])
    G = go + gy if use_dy else go
    hm, ghm = m * h, m * gh
    a = ghm + b[:, None]
    r = torch.sigmoid(gi[..., :H] + a[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + a[..., H:2 * H])
    a_n = a[..., 2 * H:]
    n = torch.tanh(gi[..., 2 * H:] + r * a_n)
    dpn = G * (1 - z) * (1 - n * n)
    dpz = G * (hm - n) * (z * (1 - z))
    dpr = dpn * a_n * (r * (1 - r))
    rdpn = r * dpn
    out = dict(dgi=torch.cat([dpr, dpz, dpn], -1), dgh=m * torch.cat([dpr, dpz, rdpn], -1), dh=m * (G * z), dbias=torch.cat([dpr, dpz, dpn, rdpn], -1).sum(1))
    if not bounds:
        return out
    mag = gi.abs() + ghm.abs() + b.abs()[:, None]
    da = 2 * U * mag
    dr = da[..., :H] / 4 + 4 * U
    dz = da[..., H:2 * H] / 4 + 4 * U
    dn = da[..., 2 * H:] + a_n.abs() * dr + 4 * U
    A, B, D, S, R, Ga = 1 - z, 1 - n * n, (hm - n).abs(), z * (1 - z), r * (1 - r), G.abs()
    e_pn = 4 * U * dpn.abs() + Ga * B * dz + Ga * A * (2 * n.abs() * dn + U)
    e_pz = 6 * U * dpz.abs() + Ga * S * dn + Ga * D * dz
    e_pr = a_n.abs() * R * e_pn + 5 * U * dpr.abs() + (dpn * a_n).abs() * dr
    e_rn = r * e_pn + dpn.abs() * dr + U * rdpn.abs()
    e_h = m * (2 * U * (G * z).abs() + Ga * dz)
    bnd = dict(dgi=torch.cat([e_pr, e_pz, e_pn], -1), dgh=m * torch.cat([e_pr, e_pz, e_rn], -1), dh=e_h,
               dbias=torch.cat([e_pr, e_pz, e_pn, e_rn], -1).sum(1) + U * out["dbias"].abs())
    return out, bnd


def _fro(err, truth):
    return float(err.norm() / truth.norm())


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------
def check_against_f64(L, di, stream, tdev, H, M, G=3, layout="layers"):
    """The four outputs of G networks with different data on M rows against float64: gate (a) per element, gate (b) in the Frobenius norm.
    Returns (outputs, bounds) for the comparison of the two builds."""
    d = make_data(G, M, H, seed=7 * H + M)
    got = run(L, di, stream, tdev, d, layout)
    truth, bound = closed_form(d, bounds=True)
    yard = closed_form(d, torch.float32)
    vals = {}
    for k in OUTS:
        assert bool(torch.isfinite(got[k]).all()), ("non-finite output", k, H, M)
        err = (got[k].double() - truth[k]).abs()
        free = bound[k] == 0                                                        # masked rows of dgh and dh: exactly +0
        assert bool((err[free] == 0).all()), ("an error where the bound is zero", k, H, M)
        vals[k + "_elem_over_bound"] = float((err[~free] / bound[k][~free]).max())
        vals[k + "_fro"], vals[k + "_fro_torch32"] = _fro(err, truth[k]), _fro(yard[k].double() - truth[k], truth[k])
    _report(tdev, "f64_H%d_M%d_G%d" % (H, M, G), **vals)
    for k in OUTS:
        assert vals[k + "_elem_over_bound"] <= 1.0, ("gate (a): per-element bound", k, H, M, vals[k + "_elem_over_bound"])
        assert vals[k + "_fro"] <= 2.0 * vals[k + "_fro_torch32"], ("gate (b): Frobenius error against fp32 torch", k, H, M, vals[k + "_fro"], vals[k + "_fro_torch32"])
    return got, bound


def check_empty(L, di, stream, tdev):
    """M == 0 succeeds and touches nothing (run() asserts the poison), with and without a workspace to speak of"""
    d = make_data(3, 4, 36, seed=5)
    got = run(L, di, stream, tdev, d, "layers", rows=slice(0, 0))
    assert got["dh"].shape[1] == 0


# ---- 2. masks, NULL operands ---------------------------------------------------------------------------------------------------------
def check_masks(L, di, stream, tdev, H=36, M=130):
    """Rows with mask 0: dgh and dh are +0 bit for bit while dgi and the rows' share of dbias are not zero; mask NULL is a mask of ones
    bit for bit; dy NULL has the values of a dy of zeros; per-group NULL dy and dbias entries."""
    d = make_data(3, M, H, seed=11)
    a = run(L, di, stream, tdev, d)
    off = d["mask"] == 0
    assert int(off.sum()) > 0 and int((~off).sum()) > 0
    assert _same_bits(a["dgh"][off], torch.zeros_like(a["dgh"][off])) and _same_bits(a["dh"][off], torch.zeros_like(a["dh"][off])), "a masked row is not +0"
    assert bool((a["dgi"][off] != 0).all()), "dgi of a masked row is zero"
    assert bool((a["dgh"][~off] != 0).any()) and bool((a["dh"][~off] != 0).all())
    only_off = dict(d)
    only_off["dh_out"], only_off["dy"] = d["dh_out"] * off[..., None], d["dy"] * off[..., None]       # G = 0 on the rows with mask 1
    share = run(L, di, stream, tdev, only_off)["dbias"]
    assert bool((share != 0).all()), "the masked rows add nothing to dbias"
    ones = dict(d)
    ones["mask"] = torch.ones_like(d["mask"])
    b, c = run(L, di, stream, tdev, ones), run(L, di, stream, tdev, ones, use_mask=False)
    assert all(_same_bits(b[k], c[k]) for k in OUTS), "mask NULL differs from a mask of ones"
    assert not _same_bits(a["dgh"], b["dgh"]), "the mask changed nothing"
    zero = dict(d)
    zero["dy"] = torch.zeros_like(d["dy"])
    e, f = run(L, di, stream, tdev, zero), run(L, di, stream, tdev, d, use_dy=False)
    assert all(bool(torch.equal(e[k], f[k])) for k in OUTS), "dy NULL differs in value from a dy of zeros"
    assert not bool(torch.equal(e["dgi"], a["dgi"])), "dy changed nothing"
    g = run(L, di, stream, tdev, zero, dy_null=(1,), bias_null=(0, 2))                                 # run() asserts that dbias 0 and 2 stay poison
    h = run(L, di, stream, tdev, d, dy_null=(1,))
    assert all(_same_bits(g[k], e[k]) for k in OUTS[:3]) and _same_bits(g["dbias"][1], e["dbias"][1])
    assert _same_bits(h["dgi"][1], f["dgi"][1]) and _same_bits(h["dgi"][0], a["dgi"][0]) and _same_bits(h["dbias"][2], a["dbias"][2])


# ---- 3. row independence, determinism ------------------------------------------------------------------------------------------------
def check_rows_independent(L, di, stream, tdev, H=100):
    """Rows 5 .. 11 of network 1: alone (M = 7), inside M = 300 at rows 240 .. 246 (the last of four chunks), and as network 17 of 32 -- the same
    bits of dgi, dgh and dh.  dbias: two runs of one call, and network 1 alone against network 1 among three -- the same bits."""
    d = make_data(3, 300, H, seed=17)
    alone = run(L, di, stream, tdev, d, "dense", rows=slice(5, 12), groups=[1])
    moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    for k in ("gi", "gh", "h", "mask", "dh_out", "dy"):
        moved[k][1, 240:247] = d[k][1, 5:12]
    inside = run(L, di, stream, tdev, moved, "layers")
    many = [g % 3 for g in range(32)]
    many[17] = 1
    wide = run(L, di, stream, tdev, d, "agents", rows=slice(0, 33), groups=many)
    for k in OUTS[:3]:
        assert _same_bits(inside[k][1, 240:247], alone[k][0]), ("a row's result depends on M or on where the row sits", k)
        assert _same_bits(wide[k][17, 5:12], alone[k][0]), ("a row's result depends on the number of groups", k)
    again = run(L, di, stream, tdev, moved, "layers")
    assert all(_same_bits(again[k], inside[k]) for k in OUTS), "two runs of one call differ"
    single = run(L, di, stream, tdev, moved, "layers", groups=[1])
    assert _same_bits(single["dbias"][0], inside["dbias"][1]), "dbias depends on the number of groups"
    assert _same_bits(wide["dbias"][17], wide["dbias"][1]) and _same_bits(wide["dbias"][31], wide["dbias"][1])


# ---- 4. layouts and writes -----------------------------------------------------------------------------------------------------------
def check_layouts(L, di, stream, tdev, H=36, M=7):
    """h from every layout (dh_out and dh then take the next one; no pitch of run() is the dense one) gives the same bits; without dbias
    the three row outputs are the same bits and nothing else is written -- the workspace of the queried size with its guard included
    (run() asserts the poison everywhere)."""
    d = make_data(3, M, H, seed=13)
    first = run(L, di, stream, tdev, d, LAYOUTS[0])
    for layout in LAYOUTS[1:]:
        got = run(L, di, stream, tdev, d, layout)
        assert all(_same_bits(got[k], first[k]) for k in OUTS), layout
    bare = run(L, di, stream, tdev, d, LAYOUTS[1], with_bias=False)
    assert bare["dbias"] is None and all(_same_bits(bare[k], first[k]) for k in OUTS[:3])


# ---- 5. contract -------------------------------------------------------------------------------------------------------------------------
def check_contract(L, di, stream, tdev):
    """The size query; each bad call returns non-zero, names the entry in mms_last_error and leaves the poisoned destinations as they were;
    the good call with the same arguments succeeds."""
    M, H, W = 8, 8, 1028
    t = lambda *s: torch.randn(*s).to(tdev)
    src = dict(gi=t(M, 3 * W), gh=t(M, 3 * W), h=t(M, W), mask=t(M), bh=t(3 * W), go=t(M, W), gy=t(M, W))
    nan = lambda *s: torch.full(s, float("nan"), device=tdev)
    dst = dict(dgi=nan(M + 1, 3 * W), dgh=nan(M + 1, 3 * W), dh=nan(M + 1, W), db=nan(4 * W))
    need, ws, base = workspace(L, di, 1, M, H, tdev)
    if torch.device(tdev).type == "cpu":
        assert need == 0, "the CPU build needs no workspace"
    else:
        assert 0 < need <= workspace(L, di, 2, M, H, tdev)[0]
    one = lambda v, n=1: _ptrs([v.data_ptr()] * n)
    pitches = dict(gp=3 * W, hp=W, mp=1, gop=W, gyp=W, dgp=3 * W, dhp=W)

    def call(groups=1, M=M, H=H, n=None, dev=di, wsp=base, size=need, no_size=False, **kw):
        n = max(groups, 1) if n is None else n
        v = dict(src, **dst)
        v.update(pitches)
        v.update(kw)
        arr = lambda x: None if x is None else (x if isinstance(x, ctypes.Array) else one(x, n))
        sz = ctypes.c_int64(size)
        return L.mms_gru_gates_grad_group(dev, groups, M, H, arr(v["gi"]), arr(v["gh"]), v["gp"], arr(v["h"]), v["hp"], arr(v["mask"]), v["mp"], arr(v["bh"]),
                                          arr(v["go"]), v["gop"], arr(v["gy"]), v["gyp"], arr(v["dgi"]), arr(v["dgh"]), v["dgp"], arr(v["dh"]), v["dhp"],
                                          arr(v["db"]), None if wsp is None else ctypes.c_void_p(wsp), None if no_size else ctypes.byref(sz), stream)

    bad = {}
    for k in dst:                                                                           # every aliasing pair of include/mms.h
        for s in src:
            bad["%s == %s" % (k, s)] = {k: src[s]}
        for k2 in dst:
            if k2 > k:
                bad["%s == %s" % (k, k2)] = {k: dst[k2]}
    bad.update({
        "two groups, one destination": dict(groups=2),
        "workspace too small": dict(size=need - 256),
        "misaligned workspace": dict(wsp=base + 64, size=need + 256),
        "ws_bytes NULL": dict(no_size=True),
        "ws_bytes NULL in the size query": dict(no_size=True, wsp=None),
        "H % 4 != 0": dict(H=6),
        "H == 0": dict(H=0),
        "H > 1024": dict(H=W),
        "H > 1024 in the size query": dict(H=W, wsp=None),
        "groups == 0": dict(groups=0),
        "groups == 33": dict(groups=33),
        "M < 0": dict(M=-1),
        "g_pitch < 3H": dict(gp=3 * H - 4),
        "odd g_pitch": dict(gp=3 * W + 1),
        "dg_pitch < 3H": dict(dgp=3 * H - 4),
        "odd dg_pitch": dict(dgp=3 * W + 2),
        "h_pitch < H": dict(hp=4),
        "dh_out_pitch < H": dict(gop=4),
        "odd dh_out_pitch": dict(gop=W + 1),
        "dy_pitch < H": dict(gyp=4),
        "dh_pitch < H": dict(dhp=4),
        "odd dh_pitch": dict(dhp=W - 1),
        "mask_pitch 0": dict(mp=0),
        "gi NULL": dict(gi=None),
        "b_hh NULL": dict(bh=None),
        "dh_out NULL": dict(go=None),
        "dgi NULL": dict(dgi=None),
        "dgh NULL": dict(dgh=None),
        "dh NULL": dict(dh=None),
        "a NULL gh entry": dict(gh=_ptrs([None])),
        "a NULL dh_out entry": dict(go=_ptrs([None])),
        "a NULL dh entry": dict(dh=_ptrs([None])),
        "a NULL mask entry": dict(mask=_ptrs([None])),
        "misaligned gi": dict(gi=_ptrs([src["gi"].data_ptr() + 4])),
        "misaligned dh_out": dict(go=_ptrs([src["go"].data_ptr() + 8])),
        "misaligned dy": dict(gy=_ptrs([src["gy"].data_ptr() + 4])),
        "misaligned dgh": dict(dgh=_ptrs([dst["dgh"].data_ptr() + 4])),
        "misaligned dh": dict(dh=_ptrs([dst["dh"].data_ptr() + 8])),
        "misaligned dbias": dict(db=_ptrs([dst["db"].data_ptr() + 2])),
        "bad device": dict(dev=-1 if di >= 0 else 0),
    })
    if need == 0:
        del bad["workspace too small"]                                                      # (the CPU build: nothing is too small)
    assert len([k for k in bad if " == " in k and "groups" not in k and "H ==" not in k]) == 4 * 7 + 6
    for name, kw in bad.items():
        rc = call(**kw)
        _sync(tdev)
        assert rc != 0, name
        if name != "bad device":                                                            # (that one is the build's own device check)
            assert ENTRY in _lib.last_error(None, L), (name, _lib.last_error(None, L))
        assert all(bool(torch.isnan(v).all()) for v in dst.values()), ("written on error", name)
    assert _guard_intact(ws, base, need)
    _lib.check(call(M=0), None, ENTRY + " with M == 0", L)
    _sync(tdev)
    assert all(bool(torch.isnan(v).all()) for v in dst.values()), "M == 0 wrote something"
    _lib.check(call(), None, ENTRY, L)                                                      # ... and the good call of the same arguments
    _lib.check(call(mask=None, gy=None, db=None), None, ENTRY + " without mask, dy and dbias", L)
    _lib.check(call(gy=_ptrs([None]), db=_ptrs([None])), None, ENTRY + " with NULL dy and dbias entries", L)
    _sync(tdev)
    for k, w in (("dgi", 3 * H), ("dgh", 3 * H), ("dh", H)):
        v = dst[k]
        assert bool(torch.isfinite(v[:M, :w]).all()) and bool(torch.isnan(v[:M, w:]).all()) and bool(torch.isnan(v[M:]).all()), k
    assert bool(torch.isfinite(dst["db"][:4 * H]).all()) and bool(torch.isnan(dst["db"][4 * H:]).all())


# ---- 6. the two builds ---------------------------------------------------------------------------------------------------------------------
def builds_agree(gpu, cpu):
    """(outputs, bounds) of check_against_f64 from both builds on the same data: each output lies within its bound of the truth, so the
    builds differ by at most the sum of the two bounds.  Returns the worst difference / that sum over the four outputs."""
    (a, ba), (b, bb) = gpu, cpu
    worst = 0.0
    for k in OUTS:
        diff, room = (a[k].double() - b[k].double()).abs(), ba[k] + bb[k]
        assert bool((diff[room == 0] == 0).all()), k
        worst = max(worst, float((diff[room > 0] / room[room > 0]).max()))
    assert worst <= 1.0, worst
    return worst

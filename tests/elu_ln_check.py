"""Per-entry checks of the ELU + LayerNorm block entries (include/mms.h: mms_elu_ln_group, mms_elu_ln_grad_group) -- one check list for
both builds: tests/test_elu_ln.py runs it on libmms_cpu.so, tests/test_elu_ln_gpu.py on libmms.so.

Every function takes (L, device_index, stream, torch_device) and drives the C ABI through ctypes, with tests/gru_grad_check.py's
discipline: z sits in a block of pitch H + 4 and dy in one of pitch H + 8 with random filler behind every row; y (pitch H + 8), stat,
dz (pitch H + 12) and dparams are filled with NaN before the launch and have a guard row (dparams: four guard floats) behind them; the
workspace has exactly the queried size, is filled with 0x00 or with 0xFF (both must give the same bits) and stands between guard bytes;
all of that must still be poison afterwards.  In every row of the data columns 0 and 1 are made to have u > 0 and u < 0 (the rest falls
as it falls), so both branches of the ELU are present in every row; closed_form asserts it.

The truth is include/mms.h's closed form in float64 on the same fp32 inputs (closed_form), the yardstick F.elu + F.layer_norm (its
statistics: torch.native_layer_norm's) + autograd in fp32 torch on the same inputs (yardstick), both computed once per data set on the
CPU.  The gate, per network and per output (y, stat, dz, dbias, dgamma, dbeta): the relative Frobenius error against float64 is at
most twice the yardstick's (the project's margin for two fp32 evaluations that round in different places: tests/sac_grad_check.py,
tests/gru_grad_check.py), or, where the yardstick's error happens to be below one rounding of the output itself, u = 2^-24.  Each check
prints and records (parity.record) both errors and the worst per-element error over the largest magnitude of the output.

Shapes (H, M) and the edge each one hits (csrc/elu_ln_lane.h: q = H / 4 threads per row, P = 256 / q rows in flight, chunks of
max(8 P, ceil(M / 512)) rows; csrc/elu_ln_kernels.hip: row_sum's three forms):
  (4, 1)        one thread per row (no reduction step at all), one row: 255 threads without a row
  (36, 7)       q = 9 does not divide 256: rows straddle wavefronts, four idle threads, the LDS form of the row sums; one ragged pass
  (36, 130)     P = 28: five passes, the last with 18 rows
  (128, 128)    q = 32: the butterfly inside half a wave; P = 8, chunks of 64: two full chunks
  (512, 130)    q = 128: a row over two waves (butterfly + LDS); P = 2, chunks of 16: nine chunks, the last with 2 rows
  (36, 300)     chunks of 224: two, the last with 76 rows = 2 passes + 20
  (1024, 4100)  q = 256: one row per workgroup over four waves; past the cap of 512 chunks: chunks of 9 rows instead of 8, 456 of them,
                the last with 5 rows -- and the finish pass's lanes read up to eight partials each (one network: the blocks are 17 MB
                each; with the issue's (1024, 2060) there would be 258 chunks of 8 rows, under this partition's cap)
  (36, 7) x 32  the full group count, every network with its own data"""
import ctypes
import functools

import torch
import torch.nn.functional as F

import gru_check as gk
import parity
from massive_marl_benchmark_amd import _lib

U = gk.U
EPS = 1e-5
SHAPES = ((4, 1), (36, 7), (36, 130), (128, 128), (512, 130), (36, 300))
BIG = (1024, 4100)
OUTS = ("y", "stat", "dz", "dbias", "dgamma", "dbeta")
_ptrs, _sync, _same_bits, _where = gk._ptrs, gk._sync, gk._same_bits, gk._where
FWD, BWD = "mms_elu_ln_group", "mms_elu_ln_grad_group"


def _report(tdev, name, **vals):
    print("%s/elu_ln_%s: %s" % (_where(tdev), name, ", ".join("%s %.3g" % kv for kv in sorted(vals.items()))))
    parity.record("%s/elu_ln_%s" % (_where(tdev), name), **vals)


@functools.lru_cache(maxsize=None)
def make_data(G, M, H, seed):
    """{z, dy [G, M, H], bias, gamma, beta [G, H]}: pre-activations ~ 1.5 N(0, 1), so both branches of the ELU carry weight; in every row
    u[0] >= 0.1 and u[1] <= -0.1"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(G=G, M=M, H=H, z=1.5 * rn(G, M, H), dy=rn(G, M, H), bias=0.3 * rn(G, H), gamma=1.0 + 0.3 * rn(G, H), beta=0.3 * rn(G, H))
    if H >= 2:
        d["z"][..., 0] = d["z"][..., 0].abs() + 0.25 - d["bias"][:, None, 0]
        d["z"][..., 1] = -d["z"][..., 1].abs() - 0.25 - d["bias"][:, None, 1]
    return d


def _key(d):
    return id(d["z"])


_FORMS = {}


def closed_form(d):
    """include/mms.h's closed form in float64 on d's fp32 values: {y, stat, dz, dbias, dgamma, dbeta}, computed once per data set"""
    if ("truth", _key(d)) in _FORMS:
        return _FORMS["truth", _key(d)]
    H = d["H"]
    z, dy, b, ga, be = (d[k].double() for k in ("z", "dy", "bias", "gamma", "beta"))
    u = z + b[:, None]
    assert d["M"] == 0 or (bool((u > 0).any(-1).all()) and bool((u < 0).any(-1).all())), "a row without both branches of the ELU"
    a = torch.where(u > 0, u, torch.expm1(u))
    mean = a.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((a - mean) ** 2).mean(-1, keepdim=True) + EPS)
    xhat = (a - mean) * rstd
    q = dy * ga[:, None]
    c1, c2 = q.mean(-1, keepdim=True), (q * xhat).mean(-1, keepdim=True)
    dz = rstd * (q - c1 - xhat * c2) * torch.where(u > 0, torch.ones_like(u), a + 1.0)
    out = dict(y=xhat * ga[:, None] + be[:, None], stat=torch.cat([mean, rstd], -1), dz=dz, dbias=dz.sum(1), dgamma=(dy * xhat).sum(1), dbeta=dy.sum(1))
    _FORMS["truth", _key(d)] = out
    return out


def yardstick(d):
    """The same six tensors from F.elu + F.layer_norm (+ native_layer_norm's statistics) + autograd in fp32 torch on the CPU, once per data set"""
    if ("yard", _key(d)) in _FORMS:
        return _FORMS["yard", _key(d)]
    H = d["H"]
    out = {k: [] for k in OUTS}
    for g in range(d["G"]):
        z, b, ga, be = (d[k][g].clone().requires_grad_(True) for k in ("z", "bias", "gamma", "beta"))
        a = F.elu(z + b)
        y = F.layer_norm(a, (H,), ga, be, EPS)
        with torch.no_grad():
            _, mean, rstd = torch.native_layer_norm(a, (H,), ga, be, EPS)
        y.backward(d["dy"][g])
        for k, v in zip(OUTS, (y.detach(), torch.cat([mean.reshape(-1, 1), rstd.reshape(-1, 1)], -1), z.grad, b.grad, ga.grad, be.grad)):
            out[k].append(v)
    out = {k: torch.stack(v) for k, v in out.items()}
    _FORMS["yard", _key(d)] = out
    return out


def _pick(d, rows, groups):
    gs = list(range(d["G"])) if groups is None else groups
    sl = slice(0, d["M"]) if rows is None else rows
    return gs, sl, d["z"][gs[0], sl].shape[0]


def _wide(v, w, tdev):
    """v [M, H] with w columns of filler behind every row and a row of filler below (M = 0 still has an address)"""
    M = v.shape[0]
    return torch.cat([torch.cat([v, torch.randn(M, w)], 1), torch.randn(1, v.shape[1] + w)]).contiguous().to(tdev)


def _nan(tdev, *s):
    return torch.full(s, float("nan"), device=tdev)


def forward(L, di, stream, tdev, d, rows=None, groups=None):
    """One mms_elu_ln_group call on rows `rows` (a slice; None: all) of the networks `groups` (a list; None: all) of d.  Returns {y [G, M, H],
    stat [G, M, 2]} on the CPU after checking that nothing but the destinations' views was written."""
    gs, sl, M = _pick(d, rows, groups)
    H, n = d["H"], len(gs)
    zb = [_wide(d["z"][g, sl], 4, tdev) for g in gs]
    par = [[d[k][g].contiguous().to(tdev) for g in gs] for k in ("bias", "gamma", "beta")]
    yb, sb = [_nan(tdev, M + 1, H + 8) for _ in gs], [_nan(tdev, M + 1, 2) for _ in gs]
    addr = lambda ts: _ptrs([t.data_ptr() for t in ts])
    rc = L.mms_elu_ln_group(di, n, M, H, EPS, addr(zb), H + 4, addr(par[0]), addr(par[1]), addr(par[2]), addr(yb), H + 8, addr(sb), stream)
    _sync(tdev)
    _lib.check(rc, None, FWD, L)
    for i in range(n):
        assert bool(torch.isnan(yb[i][M:]).all()) and bool(torch.isnan(yb[i][:, H:]).all()), ("y: guard row or the columns behind a row", M, H)
        assert bool(torch.isnan(sb[i][M:]).all()), ("stat: guard row", M, H)
    return dict(y=torch.stack([t[:M, :H] for t in yb]).cpu(), stat=torch.stack([t[:M] for t in sb]).cpu())


def workspace(L, di, groups, M, H, tdev, fill=0x00):
    """(the queried size, a buffer holding a 256-byte aligned workspace of exactly that size filled with `fill` between guard bytes of 0xA5,
    its address)"""
    need = ctypes.c_int64(-1)
    _lib.check(L.mms_elu_ln_grad_group(di, groups, M, H, None, 0, None, None, None, None, 0, None, 0, None, None, ctypes.byref(need), None), None,
               BWD + " (size query)", L)
    assert need.value >= 0 and need.value % 256 == 0, need.value
    buf = torch.full((need.value + 768,), 0xA5, dtype=torch.uint8, device=tdev)
    base = (buf.data_ptr() + 256 + 255) // 256 * 256
    off = base - buf.data_ptr()
    buf[off:off + need.value] = fill
    return need.value, buf, base


def _guard_intact(buf, base, need):
    off = base - buf.data_ptr()
    return bool((buf[:off] == 0xA5).all()) and bool((buf[off + need:] == 0xA5).all())


def backward(L, di, stream, tdev, d, stat, rows=None, groups=None, with_params=True, null=(), fill=0x00):
    """One mms_elu_ln_grad_group call like forward(); stat [G, M, 2]: the forward's statistics of all of d; null: positions whose dparams
    entry is NULL.  Returns {dz [G, M, H], dparams [G, 3H] (None without; NaN rows where the entry was NULL)} on the CPU."""
    gs, sl, M = _pick(d, rows, groups)
    H, n = d["H"], len(gs)
    zb, dyb = [_wide(d["z"][g, sl], 4, tdev) for g in gs], [_wide(d["dy"][g, sl], 8, tdev) for g in gs]
    stb = [torch.cat([stat[g, sl], torch.randn(1, 2)]).contiguous().to(tdev) for g in gs]
    par = [[d[k][g].contiguous().to(tdev) for g in gs] for k in ("bias", "gamma")]
    dzb, dpb = [_nan(tdev, M + 1, H + 12) for _ in gs], [_nan(tdev, 3 * H + 4) for _ in gs]
    addr = lambda ts, skip=(): _ptrs([None if i in skip else t.data_ptr() for i, t in enumerate(ts)])
    need, ws, base = workspace(L, di, n, M, H, tdev, fill)
    size = ctypes.c_int64(need)
    rc = L.mms_elu_ln_grad_group(di, n, M, H, addr(zb), H + 4, addr(par[0]), addr(par[1]), addr(stb), addr(dyb), H + 8, addr(dzb), H + 12,
                                 addr(dpb, null) if with_params else None, ctypes.c_void_p(base), ctypes.byref(size), stream)
    _sync(tdev)
    _lib.check(rc, None, BWD, L)
    assert _guard_intact(ws, base, need), "written outside the workspace"
    for i in range(n):
        assert bool(torch.isnan(dzb[i][M:]).all()) and bool(torch.isnan(dzb[i][:, H:]).all()), ("dz: guard row or the columns behind a row", M, H)
        none = not with_params or i in null
        assert bool(torch.isnan(dpb[i][0 if none else 3 * H:]).all()), ("dparams: guard, or written although NULL", M, H)
    return dict(dz=torch.stack([t[:M, :H] for t in dzb]).cpu(), dparams=torch.stack([t[:3 * H] for t in dpb]).cpu() if with_params else None)


def run(L, di, stream, tdev, d, **kw):
    """forward, then backward on the forward's own statistics: the six outputs"""
    f = forward(L, di, stream, tdev, d, rows=kw.get("rows"), groups=kw.get("groups"))
    gs, sl, M = _pick(d, kw.get("rows"), kw.get("groups"))
    stat = torch.zeros(d["G"], d["M"], 2)
    for i, g in enumerate(gs):
        stat[g, sl] = f["stat"][i]
    b = backward(L, di, stream, tdev, d, stat, **kw)
    H = d["H"]
    p = b["dparams"]
    return dict(f, dz=b["dz"], dbias=None if p is None else p[:, :H], dgamma=None if p is None else p[:, H:2 * H], dbeta=None if p is None else p[:, 2 * H:])


def _fro(err, truth):
    return float(err.norm() / truth.norm())


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------
def check_against_f64(L, di, stream, tdev, H, M, G=3):
    """The six outputs of G networks with different data on M rows against float64, per network, with the module docstring's gate; the
    backward once on a workspace of zeros and once on one of 0xFF bytes: the same bits.  Returns (outputs, their per-network errors)."""
    d = make_data(G, M, H, 7 * H + M)
    got = run(L, di, stream, tdev, d)
    again = run(L, di, stream, tdev, d, fill=0xFF)
    assert all(_same_bits(got[k], again[k]) for k in OUTS), "the result depends on what the workspace held"
    truth, yard = closed_form(d), yardstick(d)
    vals, errs, bad = {}, {}, []
    for k in OUTS:
        assert bool(torch.isfinite(got[k]).all()), ("non-finite output", k, H, M)
        errs[k] = []
        for g in range(G):
            t = truth[k][g]
            e, ey = _fro(got[k][g].double() - t, t), _fro(yard[k][g].double() - t, t)
            elem = float((got[k][g].double() - t).abs().max() / t.abs().max())
            errs[k].append(e)
            for name, v in ((k + "_fro", e), (k + "_fro_torch32", ey), (k + "_elem", elem), (k + "_ratio", e / max(2.0 * ey, U))):
                vals[name] = max(vals.get(name, 0.0), v)
            if not e <= max(2.0 * ey, U):
                bad.append((k, g, e, ey))
    _report(tdev, "f64_H%d_M%d_G%d" % (H, M, G), **vals)
    assert not bad, ("relative Frobenius error above max(2 x fp32 torch's, 2^-24): (output, network, error, torch's)", H, M, bad)
    return got, errs


def check_empty(L, di, stream, tdev):
    """M == 0: the forward touches nothing; the backward writes zeros into dparams and nothing else (forward() / backward() assert the poison)"""
    d = make_data(3, 4, 36, 5)
    f = forward(L, di, stream, tdev, d, rows=slice(0, 0))
    assert f["y"].shape[1] == 0
    b = backward(L, di, stream, tdev, d, torch.zeros(3, 4, 2), rows=slice(0, 0), null=(1,))
    assert _same_bits(b["dparams"][0], torch.zeros(3 * 36)) and _same_bits(b["dparams"][2], torch.zeros(3 * 36)) and bool(torch.isnan(b["dparams"][1]).all())
    backward(L, di, stream, tdev, d, torch.zeros(3, 4, 2), rows=slice(0, 0), with_params=False)


# ---- 2. NULL dparams -------------------------------------------------------------------------------------------------------------------
def check_null_params(L, di, stream, tdev, H=36, M=130):
    """NULL dparams entries and a NULL dparams array: dz is the same bits, the entries that are given too, nothing else is written
    (backward() asserts that a NULL entry's buffer stays poison and that the exactly sized workspace's guards hold)"""
    d = make_data(3, M, H, 11)
    full = run(L, di, stream, tdev, d)
    part = run(L, di, stream, tdev, d, null=(0, 2))
    bare = run(L, di, stream, tdev, d, with_params=False)
    assert _same_bits(part["dz"], full["dz"]) and _same_bits(bare["dz"], full["dz"]) and bare["dbias"] is None
    for k in OUTS[3:]:
        assert _same_bits(part[k][1], full[k][1]), k


# ---- 3. row independence, determinism ------------------------------------------------------------------------------------------------
def check_rows_independent(L, di, stream, tdev, H=100):
    """Rows 5 .. 11 of network 1: alone (M = 7), inside M = 300 at rows 240 .. 246 (another chunk, another slot of the workgroup), and as
    network 17 of 32 -- the same bits of y, stat and dz.  dparams: two runs of one call, and network 1 alone against network 1 among
    three -- the same bits."""
    d = make_data(3, 300, H, 17)
    alone = run(L, di, stream, tdev, d, rows=slice(5, 12), groups=[1])
    moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    for k in ("z", "dy"):
        moved[k][1, 240:247] = d[k][1, 5:12]
    inside = run(L, di, stream, tdev, moved)
    many = [g % 3 for g in range(32)]
    many[17] = 1
    wide = run(L, di, stream, tdev, d, rows=slice(0, 33), groups=many)
    for k in OUTS[:3]:
        assert _same_bits(inside[k][1, 240:247], alone[k][0]), ("a row's result depends on M or on where the row sits", k, H)
        assert _same_bits(wide[k][17, 5:12], alone[k][0]), ("a row's result depends on the number of groups", k, H)
    again = run(L, di, stream, tdev, moved)
    assert all(_same_bits(again[k], inside[k]) for k in OUTS), "two runs of one call differ"
    single = run(L, di, stream, tdev, moved, groups=[1])
    for k in OUTS[3:]:
        assert _same_bits(single[k][0], inside[k][1]), ("dparams depends on the number of groups", k, H)
        assert _same_bits(wide[k][17], wide[k][1]) and _same_bits(wide[k][31], wide[k][1]), k


# ---- 4. contract -----------------------------------------------------------------------------------------------------------------------
def check_contract(L, di, stream, tdev):
    """The size query; each bad call of either entry returns non-zero, names the entry in mms_last_error and leaves the poisoned
    destinations as they were; the good calls with the same arguments succeed."""
    M, H, W = 8, 8, 1028
    t = lambda *s: torch.randn(*s).to(tdev)
    src = dict(z=t(M, W), bias=t(W), gamma=t(W), beta=t(W), stat=t(M, 2).abs() + 0.5, dy=t(M, W))
    dst = dict(y=_nan(tdev, M + 1, W), st=_nan(tdev, M + 1, 2), dz=_nan(tdev, M + 1, W), dp=_nan(tdev, 3 * W))
    need, ws, base = workspace(L, di, 1, M, H, tdev)
    if torch.device(tdev).type == "cpu":
        assert need == 0, "the CPU build needs no workspace"
    else:
        assert 0 < need <= workspace(L, di, 2, M, H, tdev)[0]
    one = lambda v, n=1: _ptrs([v.data_ptr()] * n)

    def values(groups, n, kw):
        n = max(groups, 1) if n is None else n
        v = dict(src, **dst)
        v.update(zp=W, yp=W, dyp=W, dzp=W)
        v.update(kw)
        return v, (lambda x: None if x is None else (x if isinstance(x, ctypes.Array) else one(x, n)))

    def fwd(groups=1, M=M, H=H, n=None, dev=di, eps=EPS, **kw):
        v, arr = values(groups, n, kw)
        return L.mms_elu_ln_group(dev, groups, M, H, eps, arr(v["z"]), v["zp"], arr(v["bias"]), arr(v["gamma"]), arr(v["beta"]), arr(v["y"]), v["yp"], arr(v["st"]), stream)

    def bwd(groups=1, M=M, H=H, n=None, dev=di, wsp=base, size=need, no_size=False, **kw):
        v, arr = values(groups, n, kw)
        sz = ctypes.c_int64(size)
        return L.mms_elu_ln_grad_group(dev, groups, M, H, arr(v["z"]), v["zp"], arr(v["bias"]), arr(v["gamma"]), arr(v["stat"]), arr(v["dy"]), v["dyp"], arr(v["dz"]),
                                       v["dzp"], arr(v["dp"]), None if wsp is None else ctypes.c_void_p(wsp), None if no_size else ctypes.byref(sz), stream)

    shapes = {
        "H % 4 != 0": dict(H=6), "H == 0": dict(H=0), "H > 1024": dict(H=W), "groups == 0": dict(groups=0), "groups == 33": dict(groups=33), "M < 0": dict(M=-1),
        "two groups, one destination": dict(groups=2), "z_pitch < H": dict(zp=4), "odd z_pitch": dict(zp=W + 2), "z NULL": dict(z=None), "bias NULL": dict(bias=None),
        "gamma NULL": dict(gamma=None), "a NULL z entry": dict(z=_ptrs([None])), "a NULL gamma entry": dict(gamma=_ptrs([None])),
        "misaligned z": dict(z=_ptrs([src["z"].data_ptr() + 4])), "misaligned bias": dict(bias=_ptrs([src["bias"].data_ptr() + 8])),
        "misaligned gamma": dict(gamma=_ptrs([src["gamma"].data_ptr() + 4])), "bad device": dict(dev=-1 if di >= 0 else 0),
    }
    bad_fwd = dict(shapes, **{
        "y_pitch < H": dict(yp=4), "odd y_pitch": dict(yp=W + 1), "beta NULL": dict(beta=None), "y NULL": dict(y=None), "stat NULL": dict(st=None),
        "a NULL y entry": dict(y=_ptrs([None])), "a NULL stat entry": dict(st=_ptrs([None])), "misaligned beta": dict(beta=_ptrs([src["beta"].data_ptr() + 4])),
        "misaligned y": dict(y=_ptrs([dst["y"].data_ptr() + 8])), "misaligned stat": dict(st=_ptrs([dst["st"].data_ptr() + 4])), "negative eps": dict(eps=-1.0),
        "y == z": dict(y=src["z"]), "y == gamma": dict(y=src["gamma"]), "stat == bias": dict(st=src["bias"]), "y == stat": dict(y=dst["st"]),
    })
    bad_bwd = dict(shapes, **{
        "dy_pitch < H": dict(dyp=4), "odd dy_pitch": dict(dyp=W + 3), "dz_pitch < H": dict(dzp=4), "odd dz_pitch": dict(dzp=W + 1), "stat NULL": dict(stat=None),
        "dy NULL": dict(dy=None), "dz NULL": dict(dz=None), "a NULL stat entry": dict(stat=_ptrs([None])), "a NULL dy entry": dict(dy=_ptrs([None])),
        "a NULL dz entry": dict(dz=_ptrs([None])), "misaligned stat": dict(stat=_ptrs([src["stat"].data_ptr() + 4])),
        "misaligned dy": dict(dy=_ptrs([src["dy"].data_ptr() + 4])), "misaligned dz": dict(dz=_ptrs([dst["dz"].data_ptr() + 8])),
        "misaligned dparams": dict(dp=_ptrs([dst["dp"].data_ptr() + 2])), "dz == z": dict(dz=src["z"]), "dz == dy": dict(dz=src["dy"]), "dparams == gamma": dict(dp=src["gamma"]),
        "dparams == stat": dict(dp=src["stat"]), "dz == dparams": dict(dz=dst["dp"]), "workspace too small": dict(size=need - 256),
        "misaligned workspace": dict(wsp=base + 64, size=need + 256), "ws_bytes NULL": dict(no_size=True), "ws_bytes NULL in the size query": dict(no_size=True, wsp=None),
        "H > 1024 in the size query": dict(H=W, wsp=None), "groups == 33 in the size query": dict(groups=33, wsp=None),
    })
    if need == 0:
        del bad_bwd["workspace too small"]                                                  # (the CPU build: nothing is too small)
    for entry, call, bad in ((FWD, fwd, bad_fwd), (BWD, bwd, bad_bwd)):
        for name, kw in bad.items():
            rc = call(**kw)
            _sync(tdev)
            assert rc != 0, (entry, name)
            if name != "bad device":                                                        # (that one is the build's own device check)
                assert entry in _lib.last_error(None, L), (entry, name, _lib.last_error(None, L))
            assert all(bool(torch.isnan(v).all()) for v in dst.values()), ("written on error", entry, name)
    assert _guard_intact(ws, base, need)
    _lib.check(fwd(M=0), None, FWD + " with M == 0", L)
    _sync(tdev)
    assert all(bool(torch.isnan(v).all()) for v in dst.values()), "M == 0 wrote something"
    _lib.check(fwd(), None, FWD, L)                                                         # ... and the good calls of the same arguments
    _lib.check(bwd(dp=None), None, BWD + " without dparams", L)
    _sync(tdev)
    assert bool(torch.isnan(dst["dp"]).all())
    _lib.check(bwd(), None, BWD, L)
    _sync(tdev)
    for k in ("y", "dz"):
        v = dst[k]
        assert bool(torch.isfinite(v[:M, :H]).all()) and bool(torch.isnan(v[:M, H:]).all()) and bool(torch.isnan(v[M:]).all()), k
    assert bool(torch.isfinite(dst["st"][:M]).all()) and bool(torch.isnan(dst["st"][M:]).all())
    assert bool(torch.isfinite(dst["dp"][:3 * H]).all()) and bool(torch.isnan(dst["dp"][3 * H:]).all())
    assert _guard_intact(ws, base, need)


# ---- 5. the two builds, graph replay (GPU driver only) ---------------------------------------------------------------------------------------
def builds_agree(gpu, cpu, truth_norms):
    """(outputs, errors) of check_against_f64 from both builds on the same data: per network and output the builds differ, relative to
    the truth's norm, by at most the sum of their two errors against float64.  By the triangle inequality that holds for any two results;
    what is worth having is the figure, the worst difference over that sum: near 0 the builds round alike, near 1 their errors are
    unrelated.  Each build's own gate is check_against_f64's."""
    (a, ea), (b, eb) = gpu, cpu
    worst = 0.0
    for k in OUTS:
        for g in range(a[k].shape[0]):
            diff, room = float((a[k][g].double() - b[k][g].double()).norm()) / truth_norms[k][g], ea[k][g] + eb[k][g]
            assert diff <= room * (1 + 1e-9) + 1e-300, (k, g, diff, room)
            worst = max(worst, diff / room if room > 0 else 0.0)
    return worst


def check_graph_replay(tdev="cuda", H=512, M=130, G=2):
    """Both entries captured into one graph on a side stream: two replays give the bits of the eager calls on the same buffers"""
    L = _lib.lib()
    d = make_data(G, M, H, 23)
    dev = lambda k: [d[k][g].contiguous().to(tdev) for g in range(G)]
    z, dy, bias, gamma, beta = (dev(k) for k in ("z", "dy", "bias", "gamma", "beta"))
    new = lambda *s: [_nan(tdev, *s) for _ in range(G)]
    addr = lambda ts: _ptrs([t.data_ptr() for t in ts])
    need, ws, base = workspace(L, 0, G, M, H, tdev)

    def step(y, st, dz, dp):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.mms_elu_ln_group(0, G, M, H, EPS, addr(z), H, addr(bias), addr(gamma), addr(beta), addr(y), H, addr(st), stream), None, FWD, L)
        size = ctypes.c_int64(need)
        _lib.check(L.mms_elu_ln_grad_group(0, G, M, H, addr(z), H, addr(bias), addr(gamma), addr(st), addr(dy), H, addr(dz), H, addr(dp), ctypes.c_void_p(base),
                                           ctypes.byref(size), stream), None, BWD, L)

    eager, held = [new(M, H), new(M, 2), new(M, H), new(3 * H)], [new(M, H), new(M, 2), new(M, H), new(3 * H)]
    step(*eager)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(*held)                                                                         # warm-up
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step(*held)
        for _ in range(2):
            for ts in held:
                for t in ts:
                    t.fill_(float("nan"))
            graph.replay()
            s.synchronize()
            for a, b in zip(eager, held):
                assert all(_same_bits(x, y) for x, y in zip(a, b)), "a graph replay differs from the eager call"
    assert _guard_intact(ws, base, need)

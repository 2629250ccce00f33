"""Checks of mms_split_planes16_cat (include/mms.h, csrc/split16_kernels.hip, csrc/cpu/mms_cpu.cpp) through the C ABI, shared by the
CPU-build tests (test_split16_cat.py) and the GPU tests (test_split16_cat_gpu.py).

The oracle is the project's own entry on the same build: mms_split_planes16_group (groups = 1, stat = NULL) on
torch.cat([x0, x1], 1).contiguous().  Planes, scale, inv, chain_scale and chain_inv must be byte-equal to it.  Every output of the
entry under test is an exactly sized slice of a larger buffer pre-filled with NaN (0xFF bytes for the planes); the bytes around the
slice must stay what they were."""
import ctypes

import torch

from massive_marl_benchmark_amd import _lib

# (rows, K0, K1): one element each; the seam inside a 32-chunk and inside an 8-piece; the seam on a chunk edge; an odd seam; several rows
# per wave with a ragged last block; the tasks' own widths (52 + 24, 60 + 8); more than one block of 8-lane rows
CASES = [(1, 1, 1), (3, 30, 5), (5, 32, 32), (7, 33, 31), (130, 13, 3), (129, 52, 24), (64, 60, 8), (257, 96, 8)]
LAYOUTS = ["dense", "pitched", "offset0", "offset1"]
CHAINS = [(0, 0), (1, 1), (1, 3), (2, 1), (2, 3)]
KINDS = ["zero", "big1", "big0"]
PAD = 64                                   # guard elements (bytes for the planes: keeps the slice 16-byte aligned) on either side


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def arr(t):
    return (ctypes.c_void_p * 1)(t.data_ptr())


def h32_bytes(rows, K):
    return rows * ((K + 31) // 32) * 128


def values(rows, K0, K1, seed, kinds):
    """x0 [rows, K0], x1 [rows, K1] ~ N(0, 1) on the CPU, with the first len(kinds) rows made special: all zero; the only large
    magnitude (1e4) in x1; the only large magnitude in x0."""
    g = torch.Generator().manual_seed(seed)
    x0, x1 = torch.randn(rows, K0, generator=g), torch.randn(rows, K1, generator=g)
    for r, kind in enumerate(kinds[:rows]):
        if kind == "zero":
            x0[r], x1[r] = 0.0, 0.0
        elif kind == "big1":
            x1[r, K1 // 2] = -1e4
        elif kind == "big0":
            x0[r, K0 - 1] = 1e4
    return x0, x1


def place(x, layout, which, dev):
    """`x` on `dev` in the given layout; returns (tensor whose data_ptr / stride(0) the entry gets, pitch argument).  pitched: slice
    [:, j, :] of a [rows, 3, K] block whose other slices hold 1e6 (a read across the row's end would show in the bound); offset<i>:
    source i starts one float past a 16-byte boundary (the scalar path)."""
    rows, K = x.shape
    if layout == "pitched":
        block = torch.full((rows, 3, K), 1e6, device=dev)
        j = 1 if which == 0 else 2
        block[:, j, :] = x.to(dev)
        return block[:, j, :], 3 * K
    if layout == "offset%d" % which:
        flat = torch.zeros(rows * K + 1, device=dev)
        assert flat.data_ptr() % 16 == 0
        v = flat[1:].view(rows, K)
        v.copy_(x)
        return v, 0
    return x.to(dev).contiguous(), 0


def guarded(n, dtype, dev):
    """(buffer, slice): `n` elements inside a buffer of n + 2 PAD elements pre-filled with 0xFF bytes (as f32: a NaN)."""
    buf = torch.full(((n + 2 * PAD) * (1 if dtype == torch.uint8 else 4),), 0xFF, dtype=torch.uint8, device=dev).view(dtype)
    return buf, buf[PAD:PAD + n]


def raw(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def untouched(buf, n):
    b = raw(buf)
    e = buf.element_size()
    return bool((b[:PAD * e] == 0xFF).all()) and bool((b[(PAD + n) * e:] == 0xFF).all())


def oracle(L, device, stream, x0, x1, nch, Lc, chain):
    """mms_split_planes16_group on the materialised concatenation (same build, same device)."""
    cat = torch.cat([x0, x1], 1).contiguous()
    rows, K = cat.shape
    dev = cat.device
    planes = torch.full((max(h32_bytes(rows, K), 1),), 0xFF, dtype=torch.uint8, device=dev)
    scale, inv = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    cs, ci = torch.empty(max(nch * Lc * rows, 1), device=dev), torch.empty(max(nch * Lc * rows, 1), device=dev)
    rc = L.mms_split_planes16_group(device, 1, rows, K, 0, arr(cat), arr(planes), arr(scale), arr(inv), nch, Lc, arr(chain) if nch else None,
                                    arr(cs) if nch else None, arr(ci) if nch else None, None, 0.0, stream)
    _lib.check(rc, None, "mms_split_planes16_group", L)
    return planes[:h32_bytes(rows, K)], scale, inv, cs[:nch * Lc * rows], ci[:nch * Lc * rows]


def one_call(L, device, stream, dev, rows, K0, K1, layout, nch, Lc, null, seed, kinds):
    """One call of the entry against the oracle; `null`: 0 = scale and inv given, 1 = scale NULL, 2 = inv NULL."""
    what = "rows %d K %d + %d %s chains %d x %d null %d %s" % (rows, K0, K1, layout, nch, Lc, null, kinds)
    v0, v1 = values(rows, K0, K1, seed, kinds)
    x0, pitch0 = place(v0, layout, 0, dev)
    x1, pitch1 = place(v1, layout, 1, dev)
    g = torch.Generator().manual_seed(seed + 1)
    chain = torch.stack([torch.rand(max(nch, 1), max(Lc, 1), generator=g) * 20 + 0.5, torch.rand(max(nch, 1), max(Lc, 1), generator=g)], -1).contiguous().to(dev)
    K = K0 + K1
    want = oracle(L, device, stream, x0, x1, nch, Lc, chain)
    nb, nc = h32_bytes(rows, K), nch * Lc * rows
    pb, planes = guarded(nb, torch.uint8, dev)
    sb, scale = guarded(rows, torch.float32, dev)
    ib, inv = guarded(rows, torch.float32, dev)
    cb, cs = guarded(nc, torch.float32, dev)
    db, ci = guarded(nc, torch.float32, dev)
    assert planes.data_ptr() % 16 == 0
    rc = L.mms_split_planes16_cat(device, rows, K0, pitch0, p(x0), K1, pitch1, p(x1), p(planes), None if null == 1 else p(scale), None if null == 2 else p(inv),
                                  nch, Lc, p(chain) if nch else None, p(cs) if nch else None, p(ci) if nch else None, stream)
    _lib.check(rc, None, "mms_split_planes16_cat", L)
    if dev != "cpu":
        torch.cuda.synchronize()
    for name, buf, n in (("planes", pb, nb), ("scale", sb, rows), ("inv", ib, rows), ("chain_scale", cb, nc), ("chain_inv", db, nc)):
        assert untouched(buf, n), (what, name, "bytes outside the output were written")
    assert torch.equal(planes, want[0]), (what, "planes")
    for name, got, ref, given in (("scale", scale, want[1], null != 1), ("inv", inv, want[2], null != 2), ("chain_scale", cs, want[3], True), ("chain_inv", ci, want[4], True)):
        if given:
            assert torch.equal(raw(got), raw(ref)), (what, name)
        else:
            assert bool((raw(got) == 0xFF).all()), (what, name, "a NULL output's neighbour was written")
    if "zero" in kinds[:rows]:
        r = kinds.index("zero")
        if null != 1:
            assert float(scale[r]) == 1.0, what                          # an all-zero row keeps scale 1
        assert not bool(planes.view(rows, -1)[r].any()), what
    return want


def check_case(L, device, stream, dev, rows, K0, K1):
    """Every layout x chain shape of one (rows, K0, K1), the NULL-output forms cycling through them."""
    i = 0
    kind_sets = [KINDS] if rows >= 3 else [KINDS[j:j + rows] for j in range(0, len(KINDS), rows)]
    for layout in LAYOUTS:
        for nch, Lc in CHAINS:
            for kinds in kind_sets:
                one_call(L, device, stream, dev, rows, K0, K1, layout, nch, Lc, i % 3, 100 * rows + K0 + i, kinds)
                i += 1
    # the bound is the largest magnitude over BOTH sources: 1e4 sits in [2^13, 2^14), scale 2^14 / 2^14 = 1
    want = one_call(L, device, stream, dev, rows, K0, K1, "dense", 0, 0, 0, 5, ["big1"])
    assert float(want[1][0]) == 1.0
    want = one_call(L, device, stream, dev, rows, K0, K1, "dense", 0, 0, 0, 6, ["big0"])
    assert float(want[1][0]) == 1.0


def check_rows_zero(L, device, stream, dev):
    x0, x1 = torch.randn(4, 6).to(dev), torch.randn(4, 3).to(dev)
    chain = torch.ones(2, device=dev)
    bufs = [guarded(n, dt, dev) for n, dt in ((512, torch.uint8), (4, torch.float32), (4, torch.float32), (4, torch.float32), (4, torch.float32))]
    rc = L.mms_split_planes16_cat(device, 0, 6, 0, p(x0), 3, 0, p(x1), p(bufs[0][1]), p(bufs[1][1]), p(bufs[2][1]), 1, 1, p(chain), p(bufs[3][1]), p(bufs[4][1]), stream)
    assert rc == 0, _lib.last_error(None, L)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert all(bool((raw(b) == 0xFF).all()) for b, _ in bufs)


def error_paths(L, device, stream, dev):
    """Every refused call returns non-zero with a message and writes nothing.  Returns [(label, message)]."""
    rows, K0, K1 = 4, 6, 3
    x0, x1 = torch.randn(rows, K0).to(dev), torch.randn(rows, K1).to(dev)
    chain = torch.ones(2, device=dev)
    bufs = [guarded(n, dt, dev) for n, dt in ((h32_bytes(rows, K0 + K1) + 16, torch.uint8), (rows, torch.float32), (rows, torch.float32), (rows, torch.float32),
                                              (rows, torch.float32))]
    planes, scale, inv, cs, ci = (s for _, s in bufs)

    def go(rows=rows, K0=K0, pitch0=0, x0=x0, K1=K1, pitch1=0, x1=x1, planes=planes, nch=1, Lc=1, chain=chain, cs=cs, ci=ci):
        return L.mms_split_planes16_cat(device, rows, K0, pitch0, p(x0), K1, pitch1, p(x1), p(planes), p(scale), p(inv), nch, Lc, p(chain), p(cs), p(ci), stream)

    N = None
    bad = [("null x0", dict(x0=N), "null"), ("null x1", dict(x1=N), "null"), ("null planes", dict(planes=N), "null"), ("K0 = 0", dict(K0=0), "K0, K1 >= 1"),
           ("K1 = 0", dict(K1=0), "K0, K1 >= 1"), ("K1 = -1", dict(K1=-1), "K0, K1 >= 1"), ("pitch0 below K0", dict(pitch0=K0 - 1), "pitch0 >= K0"),
           ("pitch1 below K1", dict(pitch1=K1 - 1), "pitch1 >= K1"), ("misaligned planes", dict(planes=planes[4:]), "16-byte aligned"),
           ("chains without chain", dict(chain=N), "chain"), ("chains without chain_scale", dict(cs=N), "chain"), ("chains with L = 0", dict(Lc=0), "L >= 1"),
           ("rows = -1", dict(rows=-1), "rows >= 0")]
    out = []
    for label, kw, contains in bad:
        rc = go(**kw)
        msg = _lib.last_error(None, L)
        assert rc != 0 and msg, (label, rc, msg)
        assert msg.startswith("mms_split_planes16_cat:") and contains in msg, (label, msg)
        if dev != "cpu":
            torch.cuda.synchronize()
        assert all(bool((raw(b) == 0xFF).all()) for b, _ in bufs), (label, "a refused call wrote")
        out.append((label, msg))
    assert go() == 0, _lib.last_error(None, L)
    assert go(pitch0=K0, pitch1=K1) == 0                       # a pitch equal to K is the dense form
    return out

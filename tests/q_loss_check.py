"""Checks of mms_q_heads_loss (include/mms.h) shared by the CPU-build tests (test_q_loss.py) and the GPU tests (test_q_loss_gpu.py):
seeded problems, the launch through ctypes, the float64 statement from the call's own q_out, and the gates.

Gates.  q_out equals mms_q_heads_backup's q on the same library bit for bit.  Everything else is recomputed in float64 FROM THE
CALL'S OWN q_out, so the dot product's error is out of it:

  dq   is no output of the entry; it shows in dh.  Mode 0: dq64 = scale 2 e / M, which the entry evaluates by the same three double
       operations and rounds to fp32 for dh: |dq - dq64| <= 2^-24 |dq64| (1 + 2^-20).  Mode 1: dq is -scale / M, half of it or 0.
  dh   dq w with one more rounding: |dh - dq64 w| <= (2 x 2^-24 + 2^-40) |dq64 w|, and the dq a row of dh implies (dh / w at the
       largest |w|) is within the same of dq64; in mode 1, where dq is a constant, dh == fp32(dq64 w) bit for bit (the double
       product, rounded to fp32).
  dw, db, loss   a sum of n = M (loss: G M) terms in double in SOME order, rounded to fp32 once; the terms are the double dq64 h,
       dq64 and the loss terms, each within 2^-52 relative of this check's own (three double operations in dq, one product).  A sum
       of n terms in any order is within (n - 1) 2^-53 sum|terms| of the exact sum (to first order), and this check's own float64
       sum (numpy, another order) is within the same.  So |x - x64| <= 2^-24 |x64| + M 2^-50 sum|terms|: 2^-50 = 8 x 2^-53 covers
       both orders and the terms' own roundings.

The HIP build and the CPU build share the partition and the order of every double sum (q_loss_lane.h), so on inputs whose dot
product is exact in fp32 (small dyadic rationals: `exact_problem`) q is equal on both builds and dq, dh, dw, db and the loss agree
BIT FOR BIT; on general inputs q itself differs between the builds (one fmaf chain against sixteen and a butterfly, as for
mms_q_heads_backup), so that comparison is made on the exact problem.

The launcher's rule, restated (csrc/q_loss_kernels.hip: launch_main): `expected_kernel`.  REACHABLE is every q_heads_loss_kernel<G, NJ>,
G in {1, 2} and NJ in {1, 2, 4, 8, 16} the power of two that holds nj = H / 64 chunks (H a positive multiple of 64 up to
MMS_Q_LOSS_MAX_H = 1024, mms_host.h: check_q_heads_loss), each with every chunk live (nj = NJ) and, where some H gives it (NJ >= 4),
with chunks guarded out by `j < nj`: ten kernels, sixteen entries.  NEW_SHAPES reaches all of them (test_q_loss.py:
test_shape_table_reaches_every_kernel).  Operands live inside NaN-filled allocations (q_check.poisoned)."""
import ctypes
import itertools

import numpy as np
import torch

import q_check as qc
from massive_marl_benchmark_amd import _lib

SENTINEL = 7.0
PAD = 8                      # canary floats on each side of a destination (32 bytes: dh stays 16-byte aligned)
SHAPES = [(1, 64, 1), (15, 64, 2), (17, 192, 2), (389, 1024, 2), (2100, 128, 2)]
Q_LOSS_MAX_H = 1024          # mms_host.h: check_q_heads_loss (MMS_Q_LOSS_MAX_H)


def expected_kernel(G, H):
    """launch_main<G>'s choice (G, NJ, nj) of q_heads_loss_kernel<G, NJ>: NJ the least of 1, 2, 4, 8, 16 that is >= nj = H / 64."""
    assert G in (1, 2) and H > 0 and H % 64 == 0 and H <= Q_LOSS_MAX_H
    nj = H // 64
    return G, next(n for n in (1, 2, 4, 8, 16) if nj <= n), nj


def _entry(G, H):
    G, NJ, nj = expected_kernel(G, H)
    return G, NJ, "full" if nj == NJ else "guarded"


REACHABLE = {_entry(G, H) for G in (1, 2) for H in range(64, Q_LOSS_MAX_H + 1, 64)}
# (M, H, G): nj = 1 <1>, 2 <2>, 3 and 4 <4>, 5 and 8 <8>, 9 and 16 <16> for either G at M in {17, 33} (two or three 16-row slots, the
# last one partial), and a single row
NEW_SHAPES = [(17 if (i + G) % 2 else 33, H, G) for i, H in enumerate((64, 128, 192, 256, 320, 512, 576, 1024)) for G in (1, 2)] + [(1, 320, 2)]


def coverage(shapes=None):
    return {_entry(G, H) for _, H, G in (NEW_SHAPES if shapes is None else shapes)}
MULTI = (16 * 512 * 2 + 5, 64, 2)       # more than 512 row groups: a workgroup walks several, the finish pass adds hundreds of partials


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def problem(M, H, G, seed=0, device="cpu", tie=False):
    """h_g [M,H] (ELU outputs of N(0,1)), w_g [1,H] ~ N(0, 1/H), b_g [1], target [M] ~ N(0,1), logp [M] ~ N(-3, 2).  tie: network 1 is a
    copy of network 0."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + M + G)
    hs = [torch.nn.functional.elu(torch.randn(M, H, generator=g)) for _ in range(G)]
    ws = [torch.randn(1, H, generator=g) * H ** -0.5 for _ in range(G)]
    bs = [torch.randn(1, generator=g) * 0.1 for _ in range(G)]
    if tie and G == 2:
        hs[1], ws[1], bs[1] = hs[0].clone(), ws[0].clone(), bs[0].clone()
    target = torch.randn(M, generator=g)
    logp = torch.randn(M, generator=g) * 2 - 3
    to = lambda t: qc.poisoned(t.to(device).contiguous())
    return dict(h=[to(t) for t in hs], w=[to(t) for t in ws], b=[to(t) for t in bs], target=to(target), logp=to(logp))


def exact_problem(M, H, G, seed=0, device="cpu"):
    """Multiples of 1/8 in [-2, 2] (h) and [-1, 1] (w, b): every partial sum of the dot product is a multiple of 1/64 below 2^12, exact in
    fp32 in any order, so q is the same on every build."""
    g = torch.Generator().manual_seed(77 * seed + H + M)
    r = lambda shape, k: torch.randint(-k, k + 1, shape, generator=g).float() / 8
    to = lambda t: t.to(device).contiguous()
    return dict(h=[to(r((M, H), 16)) for _ in range(G)], w=[to(r((1, H), 8)) for _ in range(G)], b=[to(r((1,), 8)) for _ in range(G)],
                target=to(r((M,), 64)), logp=to(r((M,), 64)))


def workspace(L, device, stream, M, H, G, dev):
    n = ctypes.c_int64(-1)
    two = lambda: ctypes.c_void_p(16) if G == 2 else None
    rc = L.mms_q_heads_loss(device, M, H, None, None, None, two(), two(), two(), 0, None, None, 0.0, 1.0, *([None] * 9), None, ctypes.byref(n), stream)
    _lib.check(rc, None, "mms_q_heads_loss size query", L)
    assert n.value >= 0
    buf = torch.empty(n.value + 512, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + (-buf.data_ptr()) % 256, n


class Out:
    """Destinations with PAD canaries on each side and `extra` rows behind M, pre-filled with SENTINEL."""
    NAMES = ("loss", "q0", "q1", "dh0", "dh1", "dw0", "db0", "dw1", "db1")

    def __init__(self, M, H, G, dev, want=None, extra=3):
        sizes = dict(loss=1, q0=M + extra, q1=M + extra, dh0=(M + extra) * H, dh1=(M + extra) * H, dw0=H, db0=1, dw1=H, db1=1)
        self.M, self.H, self.G = M, H, G
        self.full, self.view = {}, {}
        for k in self.NAMES:
            on = (want is None or k in want or k == "loss") and (G == 2 or not k.endswith("1"))
            if not on:
                self.view[k] = None
                continue
            self.full[k] = torch.full((sizes[k] + 2 * PAD,), SENTINEL, device=dev)
            self.view[k] = self.full[k][PAD:PAD + sizes[k]]

    def ptrs(self):
        return [p(self.view[k]) for k in self.NAMES]

    def get(self, k):
        """The written part of destination k (None where it was NULL), on the host."""
        v = self.view[k]
        if v is None:
            return None
        n = dict(loss=1, q0=self.M, q1=self.M, dh0=self.M * self.H, dh1=self.M * self.H).get(k, v.numel())
        out = v[:n].cpu()
        return out.view(self.M, self.H) if k.startswith("dh") else out

    def untouched(self):
        """Canaries round every destination and everything past M."""
        for k, f in self.full.items():
            n = dict(loss=1, q0=self.M, q1=self.M, dh0=self.M * self.H, dh1=self.M * self.H).get(k, self.view[k].numel())
            f = f.cpu()
            if not ((f[:PAD] == SENTINEL).all() and (f[PAD + n:] == SENTINEL).all()):
                return False
        return True

    def all_sentinel(self):
        return all((f.cpu() == SENTINEL).all() for f in self.full.values())


def run(L, device, stream, pr, mode, *, G=None, rows=None, row0=0, with_logp=True, alpha=0.2, scale=1.0, want=None, expect_ok=True):
    """One call on rows [row0, row0 + rows) of problem `pr`.  Returns the Out."""
    G = len(pr["h"]) if G is None else G
    Mfull, H = pr["h"][0].shape
    M = Mfull - row0 if rows is None else rows
    dev = pr["h"][0].device
    out = Out(M, H, G, dev, want)
    keep, ws, n = workspace(L, device, stream, M, H, G, dev)
    hs = [pr["h"][g][row0:] for g in range(G)]
    g1 = lambda xs: p(xs[1]) if G == 2 else None
    target = pr["target"][row0:] if mode == 0 else None
    logp = pr["logp"][row0:] if (mode == 1 and with_logp) else None
    rc = L.mms_q_heads_loss(device, M, H, p(hs[0]), p(pr["w"][0]), p(pr["b"][0]), g1(hs), g1(pr["w"]), g1(pr["b"]), mode, p(target), p(logp),
                            float(alpha), float(scale), *out.ptrs(), ctypes.c_void_p(ws), ctypes.byref(n), stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    if expect_ok:
        _lib.check(rc, None, "mms_q_heads_loss", L)
        assert out.untouched(), "a canary or a row past M was written"
    del keep
    return out


def backup_q(L, device, stream, pr, G, rows=None):
    """mms_q_heads_backup's q on the same library."""
    M, H = pr["h"][0].shape
    M = M if rows is None else rows
    dev = pr["h"][0].device
    q = [torch.empty(M, device=dev) for _ in range(G)]
    g1 = lambda xs: p(xs[1]) if G == 2 else None
    rc = L.mms_q_heads_backup(device, M, H, p(pr["h"][0]), p(pr["w"][0]), p(pr["b"][0]), p(q[0]), g1(pr["h"]), g1(pr["w"]), g1(pr["b"]), g1(q),
                              None, None, None, 0.99, 0.2, None, stream)
    _lib.check(rc, None, "mms_q_heads_backup", L)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return [t.cpu() for t in q]


def f64_statement(out, pr, mode, with_logp, alpha, scale):
    """dq, the loss and the sums' terms in float64 from the call's own q_out."""
    G, M = out.G, out.M
    q = [out.get("q%d" % g).double().numpy() for g in range(G)]
    alpha, scale = float(np.float32(alpha)), float(np.float32(scale))
    if mode == 0:
        t = pr["target"].cpu().double().numpy()[:M]
        e = [q[g] - t for g in range(G)]
        dq = [scale * 2.0 * e[g] / M for g in range(G)]
        loss_terms = np.concatenate([x * x for x in e]) / M
    else:
        full = -scale / M
        if G == 2:
            dq = [np.where(q[0] < q[1], full, np.where(q[1] < q[0], 0.0, 0.5 * full)), np.where(q[1] < q[0], full, np.where(q[0] < q[1], 0.0, 0.5 * full))]
            m = np.minimum(q[0], q[1])
        else:
            dq, m = [np.full(M, full)], q[0]
        lp = pr["logp"].cpu().double().numpy()[:M] if with_logp else np.zeros(M)
        loss_terms = np.concatenate([alpha * lp, -m]) / M
    return dq, loss_terms


def check_against_float64(out, pr, mode, with_logp=True, alpha=0.2, scale=1.0, what="", mutation=None):
    """Every output but q against the float64 statement (module docstring); returns each one's worst error / gate.  `mutation` corrupts
    the statement's h and w -- "chunk": the last 64 k are zero, "last": the last k alone, what a kernel that drops its last chunk or
    element would leave in dh and dw -- and nothing is asserted: the caller judges the ratios."""
    if mutation is not None:
        return _ratios_against_mutated(out, pr, mode, with_logp, alpha, scale, mutation)
    G, M, H = out.G, out.M, out.H
    dq64, loss_terms = f64_statement(out, pr, mode, with_logp, alpha, scale)
    u = 2.0 ** -24
    worst = {}
    loss = float(out.get("loss")[0])
    ref = float(loss_terms.sum())
    gate = u * abs(ref) + M * 2.0 ** -50 * float(np.abs(loss_terms).sum())
    worst["loss"] = abs(loss - ref) / (gate + 1e-300)
    assert abs(loss - ref) <= gate, (what, "loss", loss, ref, gate)
    for g in range(G):
        w = pr["w"][g].cpu().double().numpy()[0]
        h = pr["h"][g].cpu().double().numpy()[:M]
        dh = out.get("dh%d" % g)
        if dh is not None:
            dh = dh.double().numpy()
            ref = dq64[g][:, None] * w[None, :]
            if mode == 1:
                assert np.array_equal(dh.astype(np.float32), (dq64[g][:, None] * w[None, :]).astype(np.float32)), (what, "dh", g)
            gate = (2 * u + 2.0 ** -40) * np.abs(ref)
            worst["dh%d" % g] = float((np.abs(dh - ref) / (gate + 1e-300)).max())
            assert (np.abs(dh - ref) <= gate).all(), (what, "dh", g, worst)
            # each row of dh is ONE fp32 dq times w: the dq it implies meets the one-rounding gate
            k = int(np.abs(w).argmax())
            dq_implied = dh[:, k] / w[k]
            assert (np.abs(dq_implied - dq64[g]) <= (2 * u + 2.0 ** -40) * np.abs(dq64[g])).all(), (what, "dq", g)
        dw, db = out.get("dw%d" % g), out.get("db%d" % g)
        if dw is not None:
            terms = dq64[g][:, None] * h
            ref = terms.sum(0)
            gate = u * np.abs(ref) + M * 2.0 ** -50 * np.abs(terms).sum(0)
            err = np.abs(dw.double().numpy() - ref)
            worst["dw%d" % g] = float((err / (gate + 1e-300)).max())
            assert (err <= gate).all(), (what, "dw", g, worst)
            ref = dq64[g].sum()
            gate = u * abs(ref) + M * 2.0 ** -50 * np.abs(dq64[g]).sum()
            worst["db%d" % g] = abs(float(db[0]) - ref) / (gate + 1e-300)
            assert abs(float(db[0]) - ref) <= gate, (what, "db", g, worst)
    print("%s M %d H %d G %d mode %d: worst error / gate %s" % (what, M, H, G, mode, {k: round(v, 3) for k, v in worst.items()}))
    return worst


def _ratios_against_mutated(out, pr, mode, with_logp, alpha, scale, mutation):
    """check_against_float64's dh and dw gates, unasserted, against h and w without their last chunk or element."""
    G, M, H = out.G, out.M, out.H
    dq64, _ = f64_statement(out, pr, mode, with_logp, alpha, scale)
    cut = {"chunk": H - 64, "last": H - 1}[mutation]
    u = 2.0 ** -24
    worst = {}
    for g in range(G):
        w = pr["w"][g].cpu().double().numpy()[0].copy()
        h = pr["h"][g].cpu().double().numpy()[:M].copy()
        w[cut:], h[:, cut:] = 0.0, 0.0
        ref = dq64[g][:, None] * w[None, :]
        worst["dh%d" % g] = float((np.abs(out.get("dh%d" % g).double().numpy() - ref) / ((2 * u + 2.0 ** -40) * np.abs(ref) + 1e-300)).max())
        terms = dq64[g][:, None] * h
        ref = terms.sum(0)
        gate = u * np.abs(ref) + M * 2.0 ** -50 * np.abs(terms).sum(0)
        worst["dw%d" % g] = float((np.abs(out.get("dw%d" % g).double().numpy() - ref) / (gate + 1e-300)).max())
    return worst


def same_bits(a, b, keys=Out.NAMES):
    for k in keys:
        x, y = a.get(k), b.get(k)
        if x is None or y is None:
            continue
        if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
            return k
    return None


def check_shape(L, device, stream, dev, M, H, G, what="", mutation=None):
    """Both modes at one shape: q against mms_q_heads_backup, everything else against float64, a second run bit for bit.  With
    `mutation` (check_against_float64) only mode 0's ratios against the corrupted statement are returned."""
    pr = problem(M, H, G, seed=3, device=dev)
    if mutation is not None:
        return check_against_float64(run(L, device, stream, pr, 0, scale=0.75), pr, 0, True, 0.2, 0.75, what, mutation=mutation)
    qb = backup_q(L, device, stream, pr, G)
    worst = 0.0
    for mode, with_logp in ((0, True), (1, True), (1, False)):
        out = run(L, device, stream, pr, mode, with_logp=with_logp, scale=0.75)
        for g in range(G):
            assert torch.equal(out.get("q%d" % g), qb[g]), (what, "q differs from mms_q_heads_backup", g)
        worst = max(worst, max(check_against_float64(out, pr, mode, with_logp, 0.2, 0.75, what).values()))
        again = run(L, device, stream, pr, mode, with_logp=with_logp, scale=0.75)
        assert same_bits(out, again) is None, (what, "second run differs", same_bits(out, again))
    qc.note("cpu" if device < 0 else "gpu", "q_heads_loss", "new" if (M, H, G) in NEW_SHAPES else "old", worst)


def check_ties_and_strict(L, device, stream, dev):
    """Mode 1: a copied network ties on every row and both get exactly half; strict rows get exactly -scale/M and 0."""
    M, H, scale = 77, 128, 3.0
    full = -np.float64(np.float32(scale)) / M
    dh_of = lambda dq, w: torch.from_numpy((np.asarray(dq, np.float64)[:, None] * w.double().numpy()).astype(np.float32))     # one rounding
    pr = problem(M, H, 2, seed=4, device=dev, tie=True)
    out = run(L, device, stream, pr, 1, scale=scale)
    for g in range(2):
        assert torch.equal(out.get("dh%d" % g), dh_of(np.full(M, 0.5 * full), pr["w"][0].cpu())), g
        assert torch.equal(out.get("dh%d" % g) * 2, dh_of(np.full(M, full), pr["w"][0].cpu())), g            # exactly half
    assert torch.equal(out.get("dw0"), out.get("dw1")) and torch.equal(out.get("db0"), out.get("db1"))
    assert float(out.get("db0")[0]) == float(np.float32(M * 0.5 * full))
    pr = problem(M, H, 2, seed=5, device=dev)
    out = run(L, device, stream, pr, 1, scale=scale)
    q0, q1 = out.get("q0"), out.get("q1")
    assert (q0 != q1).all() and (q0 < q1).any() and (q1 < q0).any()
    for g, mine, other in ((0, q0, q1), (1, q1, q0)):
        assert torch.equal(out.get("dh%d" % g), dh_of(np.where((mine < other).numpy(), full, 0.0), pr["w"][g].cpu())), g
    one = run(L, device, stream, dict(pr, h=pr["h"][:1], w=pr["w"][:1], b=pr["b"][:1]), 1, G=1, scale=scale)
    assert torch.equal(one.get("dh0"), dh_of(np.full(M, full), pr["w"][0].cpu()))


def check_row_independence(L, device, stream, dev):
    """A row's q, dq and dh on a slice, with scale adjusted for the slice's 1/M (powers of two, so the adjustment is exact)."""
    M, H = 256, 192
    pr = problem(M, H, 2, seed=6, device=dev)
    for mode in (0, 1):
        full = run(L, device, stream, pr, mode, scale=1.0)
        part = run(L, device, stream, pr, mode, rows=64, row0=52, scale=0.25)          # 64 / 256: scale / M is unchanged
        for k in ("q0", "q1", "dh0", "dh1"):
            assert torch.equal(part.get(k), full.get(k)[52:52 + 64]), (mode, k)


def check_null_outputs(L, device, stream, dev, M=17, H=192, G=2):
    """Every combination of NULL outputs leaves the others' bits unchanged."""
    pr = problem(M, H, G, seed=7, device=dev)
    groups = [("q0",), ("q1",), ("dh0",), ("dh1",), ("dw0", "db0"), ("dw1", "db1")]
    groups = [grp for grp in groups if G == 2 or not grp[0].endswith("1")]
    for mode in (0, 1):
        full = run(L, device, stream, pr, mode)
        for mask in itertools.product((0, 1), repeat=len(groups)):
            want = set(k for on, grp in zip(mask, groups) if on for k in grp)
            out = run(L, device, stream, pr, mode, want=want)
            assert all((out.get(k) is None) == (k not in want and k != "loss") for k in Out.NAMES if G == 2 or not k.endswith("1"))
            assert same_bits(out, full) is None, (mode, sorted(want), same_bits(out, full))


def check_contract(L, device, stream, other_device):
    """Bad arguments return non-zero with a message and write nothing."""
    M, H = 8, 64
    dev = torch.device("cpu" if device < 0 else "cuda:%d" % device)
    pr = problem(M, H, 2, seed=8, device=dev)
    out = Out(M, H, 2, dev)
    keep, ws, n = workspace(L, device, stream, M, H, 2, dev)
    pad = torch.zeros(M * H + 1, device=dev)[1:].view(M, H)        # 4 bytes past a 16-byte boundary
    N = None

    def go(M=M, H=H, h=pr["h"], w=pr["w"], b=pr["b"], mode=0, target=pr["target"], dst=None, ws=ws, nbytes=None, device=device):
        d = dict(out.view)
        d.update(dst or {})
        nb = ctypes.c_int64(n.value if nbytes is None else nbytes)
        return L.mms_q_heads_loss(device, M, H, p(h[0]), p(w[0]), p(b[0]), p(h[1]), p(w[1]), p(b[1]), mode, p(target), p(pr["logp"]), 0.2, 1.0,
                                  *[p(d[k]) for k in Out.NAMES], ctypes.c_void_p(ws), ctypes.byref(nb), stream)

    bad = [("M = 0", dict(M=0), "1..2147483647"), ("M = -1", dict(M=-1), "1..2147483647"), ("M = 2^31", dict(M=2 ** 31), "1..2147483647"),
           ("H = 96", dict(H=96), "multiple of 64"), ("H = 0", dict(H=0), "multiple of 64"), ("H = 1088", dict(H=1088), "up to 1024"),
           ("mode 2", dict(mode=2), "mode"), ("mode 0 without target", dict(target=N), "target"), ("mode 1 with target", dict(mode=1), "no target"),
           ("NULL w0", dict(w=[N, pr["w"][1]]), "required"), ("NULL loss", dict(dst=dict(loss=N)), "required"),
           ("h1 without w1", dict(w=[pr["w"][0], N]), "second network"), ("q1_out without network 1", dict(h=[pr["h"][0], N], w=[pr["w"][0], N], b=[pr["b"][0], N]), "second network"),
           ("dw0 without db0", dict(dst=dict(db0=N)), "together"), ("misaligned h0", dict(h=[pad, pr["h"][1]]), "aligned"),
           ("misaligned dh1", dict(dst=dict(dh1=out.view["dh1"][1:])), "aligned"), ("misaligned workspace", dict(ws=ws + 64), "256-byte"),
           ("wrong device", dict(device=other_device), None)]
    if device >= 0:
        bad.append(("small workspace", dict(nbytes=n.value - 1), "too small"))
    for label, kw, contains in bad:
        rc = go(**kw)
        msg = _lib.last_error(None, L)
        assert rc != 0 and msg, (label, rc, msg)
        assert contains is None or contains in msg, (label, msg)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert out.all_sentinel(), label
    assert go() == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert out.untouched() and not any((out.get(k) == SENTINEL).any() for k in Out.NAMES)
    del keep


def run_exact(L, device, stream, dev, M, H, mode):
    return run(L, device, stream, exact_problem(M, H, 2, seed=9, device=dev), mode, scale=0.5)

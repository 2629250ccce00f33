"""Checks of mms_sac_heads_act (include/mms.h) shared by the CPU-build tests (test_sac_actor.py) and the GPU tests
(test_sac_actor_gpu.py): the launch through ctypes, the float64 evaluation of SAC's head formulae (agents/algorithms/rl/sac/
module.py:31-61) and the error gates.

Gates.  The epilogue (clamp, exp, rsample, tanh, log-probability) is checked against float64 evaluated from the call's own mu and
log_std, so that the GEMM's rounding is judged separately.  The log-probability's tanh correction log(1 - t^2 + eps) amplifies an
error dt of t = tanh(u) by 2|t| / (1 - t^2 + eps) -- large near |t| = 1, where the reference's fp32 evaluation has the same
cancellation -- so a row's logp gate is sum_j (1e-4 + 2|t_j| dt_j / (1 - t_j^2 + eps)) with dt = 8 ulp(1) + (1 - t^2) |du| (a few
ulp of tanh plus the propagated difference of u): 1e-4 A plus little on rows with max|u| < 3.

The launcher's rule, restated (csrc/sac_kernels.hip: launch_sac_head_act): `expected_kernel`.  REACHABLE is every
(NCT, WAVES, demoted) over the entry's accepted arguments (A in 1..128, H any positive multiple of 64: mms_host.h,
check_sac_heads_act): NCT = 2 ceil(A / 16) in {2, 4, .., 16}, WAVES in {1, 2, 4, 8} for NCT <= 8 and in {1, 2, 4} above, where
H % 512 == 0 asks for 8 waves and the 64 KB clamp halves them (demoted) -- 28 kernels, the four of NCT >= 10 with 4 waves reached
both ways, 32 entries.  CASES reaches all of them (test_sac_actor.py: test_case_table_reaches_every_kernel).

In `check_kernel` operands live inside NaN-filled allocations and destinations between guard floats (q_check.poisoned, Guarded)."""
import ctypes

import numpy as np
import torch

import q_check as qc
from massive_marl_benchmark_amd import _lib

LOG_2PI_HALF = 0.5 * np.log(2.0 * np.pi)
ULP1 = 2.0 ** -24


def run(L, device, stream, hidden, mu_w, mu_b, ls_w, ls_b, *, act_limit=1.0, epsilon=1e-6, deterministic=False, seed=1, counters=None,
        row_offset=0, with_logp=True):
    """One mms_sac_heads_act call with every destination; returns a dict of the outputs (tensors on hidden's device).  Every
    destination is NaN-filled between guard floats, which the call must leave alone."""
    N, H = hidden.shape
    A = mu_w.shape[0]
    dev = hidden.device
    guards = {k: qc.Guarded((N, A), dev, fill=float("nan")) for k in ("action", "act_slot", "u", "mu", "log_std")}
    if with_logp:
        guards["logp"] = qc.Guarded((N,), dev, fill=float("nan"))
    out = {k: g.view for k, g in guards.items()}
    out.setdefault("logp", None)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(L.mms_sac_heads_act(device, p(hidden), H, p(mu_w), p(mu_b), p(ls_w), p(ls_b), float(act_limit), float(epsilon), int(deterministic),
                                   seed, p(counters), row_offset, p(out["action"]), p(out["act_slot"]), p(out["logp"]), p(out["u"]), p(out["mu"]),
                                   p(out["log_std"]), N, A, stream), None, "mms_sac_heads_act", L)
    assert all(g.intact() for g in guards.values()), "a float outside a destination was written"
    return out


def draws(L, device, stream, seed, counters, row_offset, N, A):
    """The standard normals a sample call with these counters uses: the same call on mu = 0, log_std = 0, where u = 0 + 1 * z = z
    exactly.  `counters` is not advanced (a copy is)."""
    dev = counters.device
    z64 = torch.zeros(N, 64, device=dev)
    w, b = torch.zeros(A, 64, device=dev), torch.zeros(A, device=dev)
    return run(L, device, stream, z64, w, b, w, b, seed=seed, counters=counters[:N].clone(), row_offset=row_offset, with_logp=False)["u"]


def f64_head(hidden, mu_w, mu_b, ls_w, ls_b, mutation=None):
    """mu and the unclamped log_std in float64, with the row scale sum_k |h_k w_jk| + |b_j| of each product.  `mutation` corrupts mu and
    log_std (not the scales): "tile" leaves the weight rows of each head's last 16-column tile out, "last" the last live column's
    alone -- what a kernel that loses those tiles, or that column, would store."""
    h, mw, mb, lw, lb = (np.asarray(t.detach().cpu(), np.float64) for t in (hidden, mu_w, mu_b, ls_w, ls_b))
    s_mu, s_ls = np.abs(h) @ np.abs(mw).T + np.abs(mb), np.abs(h) @ np.abs(lw).T + np.abs(lb)
    if mutation is not None:
        A = mw.shape[0]
        mw, lw = mw.copy(), lw.copy()
        mw[{"tile": 16 * ((A - 1) // 16), "last": A - 1}[mutation]:] = 0.0
        lw[{"tile": 16 * ((A - 1) // 16), "last": A - 1}[mutation]:] = 0.0
    mu, ls = h @ mw.T + mb, h @ lw.T + lb
    return mu, ls, s_mu, s_ls


def f64_epilogue(mu, log_std, z, act_limit, epsilon, deterministic):
    """The sampling epilogue in float64 from (fp32) mu, clamped log_std and the draws z."""
    mu, ls, z = (np.asarray(t, np.float64) for t in (mu, log_std, z))
    if deterministic:
        z = np.zeros_like(mu)
    u = mu + np.exp(ls) * z
    t = np.tanh(u)
    logp = (-0.5 * z * z - ls - LOG_2PI_HALF - np.log(1.0 - t * t + epsilon)).sum(-1)
    return u, t, act_limit * t, logp


def logp_gate(t, du, epsilon):
    t = np.asarray(t, np.float64)
    dt = 8 * ULP1 + (1.0 - t * t) * np.abs(du)
    return (1e-4 + 2.0 * np.abs(t) * dt / (1.0 - t * t + epsilon)).sum(-1)


def check_epilogue(out, z, act_limit, epsilon, deterministic, what=""):
    """The call's u / action / logp against the float64 epilogue of its own mu and log_std; returns the worst logp error over its gate."""
    np_ = lambda k: out[k].detach().cpu().numpy().astype(np.float64)
    mu, ls, u_k, act, logp = np_("mu"), np_("log_std"), np_("u"), np_("action"), np_("logp")
    u, t, act64, logp64 = f64_epilogue(mu, ls, z.cpu().numpy(), act_limit, epsilon, deterministic)
    du = np.abs(u_k - u)
    # fma rounding of u, and expf: the device's fast exp2(x log2 e) is off by up to ~|x| 2^-24 relative (x = log_std >= -20)
    assert (du <= 2.4e-7 * np.abs(u) + 2e-6 * np.exp(ls) * np.abs(z.cpu().numpy()) + 1e-30).all(), (what, du.max())
    assert (np.abs(act) <= act_limit).all(), what
    assert (np.abs(act - act64) <= act_limit * (8 * ULP1 + (1 - t * t) * du)).all(), (what, np.abs(act - act64).max())
    assert np.array_equal(np_("act_slot"), act), what
    gate = logp_gate(t, du, epsilon)
    ratio = np.abs(logp - logp64) / gate
    assert (ratio <= 1.0).all(), (what, ratio.max(), np.argmax(ratio))
    return float(ratio.max())


def problem(N, H, A, seed=0, device="cpu", scaled=True):
    """hidden [N,H] (ELU outputs; with `scaled`, every 8th row x 30 and every 8th + 4 x 300: log_std past both clamp bounds, tanh
    saturated) and the two heads' parameters at nn.Linear's scale."""
    g = torch.Generator().manual_seed(seed)
    h = torch.nn.functional.elu(torch.randn(N, H, generator=g))
    if scaled:
        h[0::8] *= 30.0
        h[4::8] *= 300.0
    k = H ** -0.5
    mk = lambda *s: qc.poisoned(((torch.rand(*s, generator=g) * 2 - 1) * k).to(device))
    return qc.poisoned(h.to(device)), mk(A, H), mk(A), mk(A, H), mk(A)


# ---- the kernel against float64 on either build, and the table of every instantiation ---------------------------------------------------

MAX_A = 128                  # mms_host.h: check_sac_heads_act (A in 1..128; H a positive multiple of 64, no maximum)
REACHABLE = ({(nct, waves, False) for nct in range(2, 2 * (MAX_A // 16) + 1, 2) for waves in (1, 2, 4, 8) if waves * 16 * nct * 16 * 4 <= 64 * 1024}
             | {(nct, 4, True) for nct in (10, 12, 14, 16)})
# the shapes test_sac_actor_gpu.py ran before CASES
OLD_SHAPES = [(4096, 1024, 80), (8192, 1024, 24), (1000, 256, 8), (7, 64, 3), (333, 128, 17), (256, 64, 128)]


def expected_kernel(H, A):
    """launch_sac_head_act's choice (nct, waves, demoted) of sac_head_act_kernel<NCT, WAVES>: a 16-column tile per 16 actions and head,
    the most waves that leave every wave a multiple of 64 k, halved while the partial sums (waves x 16 rows x 16 nct floats) exceed
    64 KB of LDS -- only 8 waves at nct >= 10 do; (8, 8) and (16, 4) ask for exactly 65536 bytes."""
    assert 1 <= A <= MAX_A and H > 0 and H % 64 == 0
    nct = 2 * ((A + 15) // 16)
    asked = waves = 8 if H % 512 == 0 else 4 if H % 256 == 0 else 2 if H % 128 == 0 else 1
    while waves > 1 and waves * 16 * nct * 16 * 4 > 64 * 1024:
        waves //= 2
    return nct, waves, waves != asked


def _cases():
    """(N, H, A): one case per entry of REACHABLE at N in {17, 33} (two or three 16-row blocks, the last one partial).  Per t = NCT / 2 the
    H alternate between A = 16 t (a full last column tile per head) and A = 16 (t - 1) + 1 (one live column in it).  Then H = 192, 384,
    768 (multiples of 64 that are no power of two: 1, 2, 4 waves) and a single row."""
    cases, n = [], 0
    for t in range(1, 9):
        for wi, H in enumerate((64, 128, 256, 512)):
            cases.append((17 if n % 2 == 0 else 33, H, 16 * t if (t + wi) % 2 == 0 else 16 * (t - 1) + 1))
            n += 1
    return cases + [(33, 192, 40), (17, 384, 97), (33, 768, 113), (1, 512, 128)]


CASES = _cases()


def coverage(cases=None):
    return {expected_kernel(H, A) for _, H, A in (CASES if cases is None else cases)}


def check_kernel(L, device, stream, dev, N, H, A, mutation=None, kind="new"):
    """A sample call and a deterministic call at one shape on either build: mu and the unclamped part of log_std against float64 over
    the row scale, e <= 2 e_torch + 1e-6 with e_torch the same measure of torch's fp32 nn.Linear on the same device; the clamp exact at
    both bounds; the counters advanced by one; the epilogue of either call (check_epilogue).  Returns the worst ratio to a gate.  With
    `mutation` the float64 side is corrupted (f64_head; torch's fp32 is still measured against the true one) and nothing but the
    ratio of the products is computed."""
    h, mw, mb, lw, lb = problem(N, H, A, seed=N + H + A, device=dev)
    c0 = ((torch.arange(N, dtype=torch.int64) * 3) % 7).to(dev)
    counters = c0.clone()
    sync = torch.cuda.synchronize if device >= 0 else (lambda: None)
    z = draws(L, device, stream, 11, counters, 5, N, A)
    out = run(L, device, stream, h, mw, mb, lw, lb, act_limit=1.0, seed=11, counters=counters, row_offset=5)
    det = run(L, device, stream, h, mw, mb, lw, lb, deterministic=True, seed=11)
    sync()
    mu64, ls64, s_mu, s_ls = f64_head(h, mw, mb, lw, lb)
    mu_m, ls_m, _, _ = f64_head(h, mw, mb, lw, lb, mutation)
    # the GEMMs: error against float64 (over the row scale) <= 2 x torch fp32 nn.Linear's on the same data + 1e-6
    t_mu = torch.nn.functional.linear(h, mw, mb).double().cpu().numpy()
    t_ls = torch.nn.functional.linear(h, lw, lb).double().cpu().numpy()
    worst = 0.0
    for name, got, ref, cmp, tref, s in (("mu", out["mu"], mu64, mu_m, t_mu, s_mu), ("mu det", det["mu"], mu64, mu_m, t_mu, s_mu)):
        e = (np.abs(got.double().cpu().numpy() - cmp) / s).max()
        et = (np.abs(tref - ref) / s).max()
        worst = max(worst, e / (2 * et + 1e-6))
        assert mutation is not None or e <= 2 * et + 1e-6, (name, e, et)
    ls = out["log_std"].double().cpu().numpy()
    inside = (ls64 > -19.99) & (ls64 < 1.99)
    e = (np.abs(ls - ls_m) / s_ls)[inside].max()
    et = (np.abs(t_ls - ls64) / s_ls)[inside].max()
    worst = max(worst, e / (2 * et + 1e-6))
    if mutation is not None:
        return float(worst)
    assert e <= 2 * et + 1e-6, ("log_std", e, et)
    assert (ls[ls64 < -20.001] == -20.0).all() and (ls[ls64 > 2.001] == 2.0).all()
    assert torch.equal(counters, c0 + 1)
    where = "cpu" if device < 0 else "gpu"
    r1 = check_epilogue(out, z, 1.0, 1e-6, False, where + " sample")
    r2 = check_epilogue(det, torch.zeros_like(z), 1.0, 1e-6, True, where + " deterministic")
    assert torch.equal(det["u"], det["mu"])
    print("%s N %d H %d A %d, kernel <%d, %d>%s: worst product error / gate %.3g, logp %.3g" %
          ((where, N, H, A) + expected_kernel(H, A)[:2] + (" (demoted)" if expected_kernel(H, A)[2] else "", worst, max(r1, r2))))
    qc.note(where, "sac_heads_act_products", kind, worst)
    qc.note(where, "sac_heads_act_logp", kind, max(r1, r2))
    return float(worst)


def check_case(L, device, stream, dev, N, H, A):
    """check_kernel, then the same two calls without logp_slot: every other output keeps its bits."""
    check_kernel(L, device, stream, dev, N, H, A)
    h, mw, mb, lw, lb = problem(N, H, A, seed=N + H + A, device=dev)
    c0 = ((torch.arange(N, dtype=torch.int64) * 3) % 7).to(dev)
    for det in (False, True):
        a = run(L, device, stream, h, mw, mb, lw, lb, deterministic=det, seed=11, counters=c0.clone(), row_offset=5)
        b = run(L, device, stream, h, mw, mb, lw, lb, deterministic=det, seed=11, counters=c0.clone(), row_offset=5, with_logp=False)
        assert b["logp"] is None and not torch.isnan(a["logp"]).any()
        for k in ("action", "act_slot", "u", "mu", "log_std"):
            assert torch.equal(a[k], b[k]) and not torch.isnan(a[k]).any(), (det, k)

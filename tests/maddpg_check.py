"""Checks of MADDPG's two entries (include/mms.h: mms_det_heads_act_group, mms_q_heads_backup_group) shared by the CPU-build tests
(test_maddpg.py) and the GPU tests (test_maddpg_gpu.py): seeded problems, the launches through ctypes, the float64 statements and
the gates.

Gates.  Deterministic actions against float64: e <= 2 e_ref + 1e-6 with e = max |a - a64| / (act_limit (1 + s)), s the row scale
sum_k |h_k w_jk| + |b_j| (q_check.f64_q's) and e_ref the same measure for torch's fp32 `act_limit * tanh(linear)` on the same device.
The drawn normal is recovered as z' = (a_noisy - a_det) / sigma in float64: a_noisy is a + sigma z rounded once (fused) or twice, so
|z' - z| <= 2^-23 (|a| + sigma |z|) / sigma <= 2^-23 (act_limit / sigma + |z|); the gate is twice that.

The launcher's rule, restated (csrc/maddpg_kernels.hip: launch_det_heads_act): `expected_kernel`.  REACHABLE is every
det_heads_act_kernel<NCT, WAVES> with NCT = ceil(A / 16) in 1..8 (A in 1..128, mms_host.h: check_det_heads_act_group) and WAVES in
{1, 2, 4, 8} (H any positive multiple of 64: the check sets no maximum), 32 kernels: the launcher's `switch` instantiates exactly
these and no A demotes WAVES.  HEAD_CASES + NEW_HEAD_CASES reaches all of them (test_maddpg.py: test_head_table_reaches_every_kernel).
Q_REACHABLE is the grouped Q kernel with each part of its k-loop (q_check.expected_path); Q_CASES + NEW_Q_CASES reaches it.

Operands live inside NaN-filled allocations and destinations between guard floats (q_check.poisoned, q_check.Guarded)."""
import ctypes

import numpy as np
import torch

import q_check as qc
from massive_marl_benchmark_amd import _lib

SENTINEL = 7.0
HEAD_CASES = [(1, 64, 1, 1, 0), (7, 64, 3, 2, 0), (16, 128, 8, 3, 0), (17, 512, 8, 10, 0), (333, 512, 16, 3, 2), (333, 256, 17, 2, 0),
              (100, 1024, 24, 32, 0), (1000, 512, 8, 10, 5)]                  # (M, H, A, groups, agent0)
Q_CASES = [(1, 64, 1), (7, 256, 3), (17, 512, 10), (1000, 256, 32), (37, 4096, 2)]    # (M, H, groups)
MAX_A = 128                  # mms_host.h: check_det_heads_act_group (A in 1..128; H a positive multiple of 64, no maximum)
REACHABLE = {(nct, waves) for nct in range(1, MAX_A // 16 + 1) for waves in (1, 2, 4, 8)}
Q_REACHABLE = {("grouped", path) for path in qc.PATHS}


def expected_kernel(H, A):
    """launch_det_heads_act's choice (nct, waves) of det_heads_act_kernel<NCT, WAVES>: one 16-column tile per 16 actions, the most waves
    that leave every wave a multiple of 64 k.  The launcher then halves waves while the partial sums (waves x 16 rows x 16 nct floats)
    exceed 64 KB of LDS: for nct <= 8 they never do -- the largest, (8, 8), is 8 x 16 x 128 x 4 = 65536 bytes, exactly 64 KB, and the
    comparison is `>` -- so that loop is unreachable through the entry and no (H, A) is demoted."""
    assert 1 <= A <= MAX_A and H > 0 and H % 64 == 0
    nct = (A + 15) // 16
    waves = 8 if H % 512 == 0 else 4 if H % 256 == 0 else 2 if H % 128 == 0 else 1
    assert waves * 16 * nct * 16 * 4 <= 64 * 1024
    return nct, waves


def _new_head_cases():
    """One case per kernel at M in {17, 33} (two or three 16-row blocks, the last one partial).  Per NCT = t the four WAVES alternate
    between A = 16 t (a full last column tile) and A = 16 (t - 1) + 1 (one live column in it); groups go round 1, 3, 10 and agent0
    alternates between 0 and 2 (the joint row's column offset).  Then H = 192, 384, 768 (multiples of 64 that are no power of two: 1, 2,
    4 waves) and a single row."""
    cases, n = [], 0
    for t in range(1, 9):
        for wi, H in enumerate((64, 128, 256, 512)):
            A = 16 * t if (t + wi) % 2 == 0 else 16 * (t - 1) + 1
            cases.append((17 if n % 2 == 0 else 33, H, A, (1, 3, 10)[n % 3], (0, 2)[(n // 2) % 2]))
            n += 1
    return cases + [(33, 192, 40, 3, 2), (17, 384, 97, 1, 0), (33, 768, 113, 3, 0), (1, 512, 128, 3, 2)]


NEW_HEAD_CASES = _new_head_cases()
# nj = 1, 3 (remainder), 4 (unrolled), 5, 7, 9 (both), each with one group and with three, and a single row
NEW_Q_CASES = [(17 if (i + G) % 2 else 33, H, G) for i, H in enumerate((64, 192, 256, 320, 448, 576)) for G in (1, 3)] + [(1, 448, 3)]


def head_coverage(cases=None):
    return {expected_kernel(H, A) for _, H, A, _, _ in (HEAD_CASES + NEW_HEAD_CASES if cases is None else cases)}


def q_coverage(cases=None):
    return {("grouped", qc.expected_path(H)) for _, H, _ in (Q_CASES + NEW_Q_CASES if cases is None else cases)}


def noise_case(case):
    """`case` with agent0, then groups, cut down until the joint row has at most 128 columns (mms_ppo_act, the source of the expected
    normals, draws for columns 0..127): the kernel is the same, it follows from H and A."""
    M, H, A, G, agent0 = case
    agent0 = min(agent0, max(0, 128 // A - 1))
    return M, H, A, min(G, 128 // A - agent0), agent0


vp = ctypes.c_void_p


def p(t):
    return None if t is None else vp(t.data_ptr())


def table(ts):
    """A host array of device pointers (None entries: NULL); None: no table."""
    return None if ts is None else (vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def head_problem(M, H, A, groups, seed=0, device="cpu"):
    """h_g [M,H] (ELU outputs of N(0,1)), w_g [A,H] ~ N(0, 1/H), b_g [A] ~ N(0, 0.01), act_limit[g] = 1 + g / 4."""
    g = torch.Generator().manual_seed(100003 * seed + 131 * H + 7 * M + 3 * A + groups)
    hs = [torch.nn.functional.elu(torch.randn(max(M, 1), H, generator=g))[:M].contiguous() for _ in range(groups)]
    ws = [torch.randn(A, H, generator=g) * H ** -0.5 for _ in range(groups)]
    bs = [torch.randn(A, generator=g) * 0.1 for _ in range(groups)]
    to = lambda t: qc.poisoned(t.to(device))
    return dict(h=[to(t) for t in hs], w=[to(t) for t in ws], b=[to(t) for t in bs], limit=[1.0 + 0.25 * i for i in range(groups)])


def head_raw(L, device, stream, groups, M, H, A, agent0, h, w, b, limit, sigma, seed, counters, row_offset, act_out, act_pitch, joint_out,
             joint_pitch):
    """The raw entry; returns the return code."""
    lim = None if limit is None else (ctypes.c_float * len(limit))(*limit)
    return L.mms_det_heads_act_group(device, groups, M, H, A, agent0, table(h), table(w), table(b), lim, float(sigma), seed, p(counters), row_offset,
                                     table(act_out), act_pitch, p(joint_out), joint_pitch, stream)


def head_run(L, device, stream, pr, *, agent0=0, sigma=0.0, seed=0, counters=None, row_offset=0, with_act=True, with_joint=True, act_pad=0,
             joint_pad=0, rows=None, tail=3):
    """One call on the first `rows` rows of `pr` into SENTINEL-filled destinations of M + tail rows with padded pitches.  Returns
    (act buffers [M + tail, A + act_pad] or None, joint buffer [M + tail, (agent0 + groups) A + joint_pad] or None).  Every destination
    sits between guard floats, which the call must leave alone."""
    G = len(pr["h"])
    M, H = pr["h"][0].shape
    A = pr["w"][0].shape[0]
    M = M if rows is None else rows
    dev = pr["h"][0].device
    ap, jp = A + act_pad, (agent0 + G) * A + joint_pad
    guards = ([qc.Guarded((M + tail, ap), dev) for _ in range(G)] if with_act else []) + ([qc.Guarded((M + tail, jp), dev)] if with_joint else [])
    acts = [x.view for x in guards[:G]] if with_act else None
    joint = guards[-1].view if with_joint else None
    rc = head_raw(L, device, stream, G, M, H, A, agent0, pr["h"], pr["w"], pr["b"], pr["limit"], sigma, seed, counters, row_offset, acts, ap, joint, jp)
    _lib.check(rc, None, "mms_det_heads_act_group", L)
    sync(pr["h"][0])
    assert all(x.intact() for x in guards), "a float outside a destination was written"
    return acts, joint


def head_f64(pr, g, mutation=None):
    """a_g in float64 and the row scale s of the pre-activation.  `mutation` corrupts a_g (not s): "tile" leaves the weight rows of the
    last 16-column tile out, "last" the last live column's alone -- what a kernel that loses that tile, or that column, would store."""
    h, w, b = (t.detach().double() for t in (pr["h"][g], pr["w"][g], pr["b"][g]))
    s = h.abs() @ w.abs().T + b.abs()
    if mutation is not None:
        w = w.clone()
        w[{"tile": 16 * ((w.shape[0] - 1) // 16), "last": w.shape[0] - 1}[mutation]:] = 0.0
    pre = h @ w.T + b
    return (pr["limit"][g] * torch.tanh(pre)).cpu().numpy(), s.cpu().numpy()


def check_head_case(L, device, stream, case, dev, mutation=None):
    """Deterministic actions against float64 (module docstring), every destination layout: padded pitches and each destination NULL in
    turn give the same bits; nothing is written past M, past A or between pitched rows.  With `mutation` the float64 actions are
    corrupted (head_f64; torch's fp32 is still measured against the true ones), the gate is not asserted and the worst
    e / (2 e_ref + 1e-6) is returned."""
    M, H, A, G, agent0 = case
    pr = head_problem(M, H, A, G, seed=1, device=dev)
    acts, joint = head_run(L, device, stream, pr, agent0=agent0, act_pad=3, joint_pad=5)
    worst = 0.0
    for g in range(G):
        a64, s = head_f64(pr, g)
        got = acts[g][:M, :A]
        e = float((np.abs(got.double().cpu().numpy() - head_f64(pr, g, mutation)[0]) / (pr["limit"][g] * (1 + s))).max())
        ref = pr["limit"][g] * torch.tanh(torch.nn.functional.linear(pr["h"][g], pr["w"][g], pr["b"][g]))
        et = float((np.abs(ref.double().cpu().numpy() - a64) / (pr["limit"][g] * (1 + s))).max())
        worst = max(worst, e / (2 * et + 1e-6))
        if mutation is not None:
            continue
        assert e <= 2 * et + 1e-6, (case, g, e, et)
        assert torch.equal(joint[:M, (agent0 + g) * A:(agent0 + g + 1) * A], got), (case, g)
        assert (acts[g][:M, A:] == SENTINEL).all() and (acts[g][M:] == SENTINEL).all(), (case, g)
    print("head case %s, kernel <%d, %d>: worst e / (2 e_ref + 1e-6) = %.3g" % ((case,) + expected_kernel(H, A) + (worst,)))
    if mutation is not None:
        return worst
    qc.note("cpu" if device < 0 else "gpu", "det_heads_act", "old" if case in HEAD_CASES else "new", worst)
    assert (joint[:, :agent0 * A] == SENTINEL).all() and (joint[:, (agent0 + G) * A:] == SENTINEL).all() and (joint[M:] == SENTINEL).all(), case
    only_act, none = head_run(L, device, stream, pr, agent0=agent0, with_joint=False)
    assert none is None and all(torch.equal(only_act[g][:M], acts[g][:M, :A]) for g in range(G)), case
    none, only_joint = head_run(L, device, stream, pr, agent0=agent0, with_act=False)
    assert none is None and torch.equal(only_joint[:M], joint[:M, :(agent0 + G) * A]), case
    return pr, acts, joint


def check_head_exactness(L, device, stream, dev):
    """A row's sigma = 0 result is the same bits for another M, groups, agent0, other pitches and another row position."""
    for case in [(333, 512, 16, 3, 2), (100, 1024, 24, 4, 0), (333, 256, 17, 2, 0)]:
        M, H, A, G, agent0 = case
        pr = head_problem(M, H, A, G, seed=2, device=dev)
        acts, _ = head_run(L, device, stream, pr, agent0=agent0)
        for g, (lo, n) in zip(range(G), [(0, 1), (37, 50), (16, 17), (5, M - 5)]):
            one = dict(h=[pr["h"][g][lo:lo + n]], w=[pr["w"][g]], b=[pr["b"][g]], limit=[pr["limit"][g]])
            assert one["h"][0].data_ptr() % 16 == 0
            a1, j1 = head_run(L, device, stream, one, agent0=7, act_pad=1, joint_pad=2)
            assert torch.equal(a1[0][:n, :A], acts[g][lo:lo + n]), (case, g)
            assert torch.equal(j1[:n, 7 * A:8 * A], acts[g][lo:lo + n]), (case, g)
    # M = 0 touches nothing
    pr = head_problem(4, 64, 3, 2, seed=3, device=dev)
    acts, joint = head_run(L, device, stream, pr, rows=0)
    assert all((a == SENTINEL).all() for a in acts) and (joint == SENTINEL).all()


def ppo_draws(L, device, stream, seed, counters, row_offset, N, A):
    """z[N, A] of mms_ppo_act for (seed, row_offset + i, counters[i], j): mean 0, log_std 0, reference_scale 0 gives action = z.
    `counters` is not advanced (a copy is)."""
    dev = counters.device
    mean, log_std, out = torch.zeros(N, A, device=dev), torch.zeros(A, device=dev), torch.empty(N, A, device=dev)
    c = counters[:N].clone()
    _lib.check(L.mms_ppo_act(device, p(mean), None, p(log_std), seed, p(c), row_offset, 0, p(out), None, None, None, None, None, N, A, stream), None,
               "mms_ppo_act", L)
    sync(out)
    return out


def check_head_noise(L, device, stream, case, dev, sigma=0.5):
    """z' against mms_ppo_act's stream, the counters, the clamp."""
    M, H, A, G, agent0 = case
    assert (agent0 + G) * A <= 128
    pr = head_problem(M, H, A, G, seed=4, device=dev)
    counters = (torch.arange(M, dtype=torch.int64) % 5).to(dev)
    c0 = counters.clone()
    det, _ = head_run(L, device, stream, pr, agent0=agent0, counters=counters)                 # sigma = 0: counters untouched
    assert torch.equal(counters, c0)
    z = ppo_draws(L, device, stream, 77, counters, 9, M, (agent0 + G) * A).double()
    noisy, joint = head_run(L, device, stream, pr, agent0=agent0, sigma=sigma, seed=77, counters=counters, row_offset=9)
    assert torch.equal(counters, c0 + 1)
    free = 0
    for g in range(G):
        lim = pr["limit"][g]
        a, n = det[g][:M].double(), noisy[g][:M].double()
        zg = z[:, (agent0 + g) * A:(agent0 + g + 1) * A]
        assert (n.abs() <= lim).all()
        inside = (a + sigma * zg).abs() < lim * (1 - 1e-6)
        outside = (a + sigma * zg).abs() > lim * (1 + 1e-6)
        assert torch.equal(n[outside], lim * torch.sign(a + sigma * zg)[outside]), (case, g)     # clamped: +-act_limit exactly
        err = ((n - a) / sigma - zg).abs()
        gate = 2.0 ** -22 * (lim / sigma + zg.abs())
        assert (err[inside] <= gate[inside]).all(), (case, g, float((err / gate)[inside].max()))
        free += int(inside.sum())
    assert free > 0.5 * M * A * G
    # a second noisy call draws with the advanced counters: other normals
    again, _ = head_run(L, device, stream, pr, agent0=agent0, sigma=sigma, seed=77, counters=counters, row_offset=9)
    assert torch.equal(counters, c0 + 2) and not any(torch.equal(again[g], noisy[g]) for g in range(G))
    # sigma > 0 with NULL act_out still draws the same joint row
    counters.copy_(c0)
    _, j2 = head_run(L, device, stream, pr, agent0=agent0, sigma=sigma, seed=77, counters=counters, row_offset=9, with_act=False)
    assert torch.equal(j2[:M], joint[:M])


def zero_head_draws(L, device, stream, dev, M=1000, A=8, G=10, agent0=5, calls=2, seed=1234, sigma=0.5):
    """The normals of `calls` consecutive noisy calls on zero weights and biases (a_det = 0, so a_noisy = sigma z exactly for the
    power of two sigma; act_limit 16 never clamps |z| < 32): [calls, M, G * A] float64."""
    pr = dict(h=[torch.zeros(M, 64, device=dev)] * G, w=[torch.zeros(A, 64, device=dev)] * G, b=[torch.zeros(A, device=dev)] * G, limit=[16.0] * G)
    counters = torch.zeros(M, dtype=torch.int64, device=dev)
    out = []
    for _ in range(calls):
        _, joint = head_run(L, device, stream, pr, agent0=agent0, sigma=sigma, seed=seed, counters=counters, with_act=False, tail=0)
        out.append(joint[:, agent0 * A:].double() / sigma)
    assert torch.equal(counters, torch.full_like(counters, calls))
    return torch.stack(out)


def check_head_statistics(L, device, stream, dev):
    """Over n = 160 000 draws |mean| and |var - 1| stay within 5 standard errors (1 / sqrt(n) and sqrt(2 / n))."""
    z = zero_head_draws(L, device, stream, dev)
    n = z.numel()
    assert n >= 100000
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print("n %d mean %.4g var %.5g" % (n, mean, var))
    assert abs(mean) <= 5 / n ** 0.5 and abs(var - 1) <= 5 * (2 / n) ** 0.5
    return z


def check_head_error_paths(L, device, stream, other_device):
    """Every refused call returns non-zero with a message and writes nothing; M = 0 succeeds and writes nothing."""
    M, H, A, G = 8, 64, 3, 2
    dev = "cpu" if device < 0 else "cuda:%d" % device
    pr = head_problem(M, H, A, G, seed=5, device=dev)
    acts = [torch.full((M, A), SENTINEL, device=dev) for _ in range(G)]
    joint = torch.full((M, G * A), SENTINEL, device=dev)
    counters = torch.zeros(M, dtype=torch.int64, device=dev)
    pad_h = torch.zeros(M * H + 1, device=dev)[1:].view(M, H)
    pad_w = torch.zeros(A * H + 1, device=dev)[1:].view(A, H)
    many = lambda xs, n: [xs[0]] * n
    N = None

    def go(groups=G, M=M, H=H, A=A, agent0=0, h=pr["h"], w=pr["w"], b=pr["b"], limit=pr["limit"], sigma=0.0, counters=N, act_out=acts, act_pitch=A,
           joint_out=joint, joint_pitch=G * A, device=device):
        return head_raw(L, device, stream, groups, M, H, A, agent0, h, w, b, limit, sigma, 3, counters, 0, act_out, act_pitch, joint_out, joint_pitch)

    bad = [("H = 96", dict(H=96), "multiple of 64"), ("H = 0", dict(H=0), "multiple of 64"), ("A = 0", dict(A=0), "1..128"), ("A = 129", dict(A=129), "1..128"),
           ("misaligned h", dict(h=[pr["h"][0], pad_h]), "aligned"), ("misaligned w", dict(w=[pad_w, pr["w"][1]]), "aligned"),
           ("groups = 0", dict(groups=0), "groups"),
           ("groups = 33", dict(groups=33, h=many(pr["h"], 33), w=many(pr["w"], 33), b=many(pr["b"], 33), limit=[1.0] * 33, act_out=many(acts, 33),
                                joint_pitch=33 * A), "groups"),
           ("act_pitch too small", dict(act_pitch=A - 1), "act_pitch"), ("joint_pitch too small", dict(joint_pitch=G * A - 1), "joint_pitch"),
           ("joint_pitch too small for agent0", dict(agent0=1), "joint_pitch"), ("no destination", dict(act_out=N, joint_out=N), "destination"),
           ("no destination in one group", dict(act_out=[acts[0], N], joint_out=N), "destination"), ("NULL h in a group", dict(h=[pr["h"][0], N]), "null pointer"),
           ("NULL b in a group", dict(b=[N, pr["b"][1]]), "null pointer"), ("sigma > 0 without counters", dict(sigma=0.5), "counters"),
           ("M = -1", dict(M=-1), "M >= 0"), ("agent0 = -1", dict(agent0=-1), "agent0"), ("wrong device", dict(device=other_device), None)]
    for label, kw, contains in bad:
        rc = go(**kw)
        msg = _lib.last_error(None, L)
        assert rc != 0 and msg, (label, rc, msg)
        assert contains is None or contains in msg, (label, msg)
        sync(joint)
        assert all((t == SENTINEL).all() for t in acts + [joint]) and (counters == 0).all(), label
    assert go(M=0, sigma=0.5, counters=counters) == 0
    sync(joint)
    assert all((t == SENTINEL).all() for t in acts + [joint]) and (counters == 0).all()
    assert go(sigma=0.5, counters=counters) == 0
    sync(joint)
    assert not any((t == SENTINEL).any() for t in acts + [joint]) and (counters == 1).all()


# ---- the grouped Q tail -------------------------------------------------------------------------------------------------------------

def q_problem(M, H, G, seed=0, device="cpu"):
    """q_check.problem with G networks and a reward / done pair per group."""
    pr = qc.problem(M, H, G, seed=seed, device=device)
    pr["r"] = [qc.poisoned(pr["r"] * (1 + g)) for g in range(G)]
    pr["d"] = [qc.poisoned(torch.roll(pr["d"], g)) for g in range(G)]
    return pr


def q_raw(L, device, stream, groups, M, H, h, w, b, q_out, reward, done, gamma, backup):
    return L.mms_q_heads_backup_group(device, groups, M, H, table(h), table(w), table(b), table(q_out), table(reward), table(done), float(gamma),
                                      table(backup), stream)


def check_q_case(L, device, stream, case, dev, gamma=0.99):
    """Each group is bit-identical to mms_q_heads_backup for that network alone; done rows give reward exactly; NULL q_out[g] /
    backup[g] per group are honoured and rows past M stay untouched."""
    M, H, G = case
    pr = q_problem(M, H, G, seed=3, device=dev)
    tail = 5
    guards = [qc.Guarded((M + tail,), dev) for _ in range(2 * G)]
    q = [x.view for x in guards[:G]]
    bk = [x.view for x in guards[G:]]
    _lib.check(q_raw(L, device, stream, G, M, H, pr["h"], pr["w"], pr["b"], q, pr["r"], pr["d"], gamma, bk), None, "mms_q_heads_backup_group", L)
    sync(q[0])
    assert all(x.intact() for x in guards), (case, "a float outside a destination was written")
    for g in range(G):
        q1, b1 = torch.full((M,), SENTINEL, device=dev), torch.full((M,), SENTINEL, device=dev)
        _lib.check(qc.call(L, device, stream, M, H, [pr["h"][g]], [pr["w"][g]], [pr["b"][g]], [q1], pr["r"][g], pr["d"][g], None, gamma, 0.0, b1), None,
                   "mms_q_heads_backup", L)
        sync(q1)
        assert torch.equal(q[g][:M], q1) and torch.equal(bk[g][:M], b1), (case, g)
        assert (q[g][M:] == SENTINEL).all() and (bk[g][M:] == SENTINEL).all(), (case, g)
        done = pr["d"][g] != 0
        assert torch.equal(bk[g][:M][done], pr["r"][g][done]), (case, g)
    # per-group NULLs: even groups without q_out, odd groups without backup (and without their reward / done)
    q2 = [None if g % 2 == 0 else torch.full((M,), SENTINEL, device=dev) for g in range(G)]
    b2 = [torch.full((M,), SENTINEL, device=dev) if g % 2 == 0 else None for g in range(G)]
    r2 = [pr["r"][g] if g % 2 == 0 else None for g in range(G)]
    d2 = [pr["d"][g] if g % 2 == 0 else None for g in range(G)]
    _lib.check(q_raw(L, device, stream, G, M, H, pr["h"], pr["w"], pr["b"], q2, r2, d2, gamma, b2), None, "mms_q_heads_backup_group", L)
    sync(q[0])
    for g in range(G):
        assert torch.equal(b2[g], bk[g][:M]) if g % 2 == 0 else torch.equal(q2[g], q[g][:M]), (case, g)
    # the forward alone: no backup table, no reward, no done
    q3 = [torch.full((M,), SENTINEL, device=dev) for _ in range(G)]
    _lib.check(q_raw(L, device, stream, G, M, H, pr["h"], pr["w"], pr["b"], q3, None, None, gamma, None), None, "mms_q_heads_backup_group", L)
    sync(q[0])
    assert all(torch.equal(q3[g], q[g][:M]) for g in range(G)), case


def check_q_error_paths(L, device, stream, other_device):
    M, H, G = 8, 64, 2
    dev = "cpu" if device < 0 else "cuda:%d" % device
    pr = q_problem(M, H, G, seed=5, device=dev)
    q = [torch.full((M,), SENTINEL, device=dev) for _ in range(G)]
    bk = [torch.full((M,), SENTINEL, device=dev) for _ in range(G)]
    pad = torch.zeros(M * H + 1, device=dev)[1:].view(M, H)
    padw = torch.zeros(H + 1, device=dev)[1:].view(1, H)
    many = lambda xs, n: [xs[0]] * n
    N = None

    def go(groups=G, M=M, H=H, h=pr["h"], w=pr["w"], b=pr["b"], q_out=q, reward=pr["r"], done=pr["d"], backup=bk, device=device):
        return q_raw(L, device, stream, groups, M, H, h, w, b, q_out, reward, done, 0.99, backup)

    bad = [("H = 96", dict(H=96), "multiple of 64"), ("H = 0", dict(H=0), "multiple of 64"), ("H above MMS_Q_MAX_H", dict(H=4160), "up to 4096"),
           ("M = -1", dict(M=-1), "M >= 0"), ("misaligned h", dict(h=[pad, pr["h"][1]]), "aligned"), ("misaligned w", dict(w=[pr["w"][0], padw]), "aligned"),
           ("groups = 0", dict(groups=0), "groups"),
           ("groups = 33", dict(groups=33, h=many(pr["h"], 33), w=many(pr["w"], 33), b=many(pr["b"], 33), q_out=many(q, 33), reward=many(pr["r"], 33),
                                done=many(pr["d"], 33), backup=many(bk, 33)), "groups"),
           ("NULL w in a group", dict(w=[pr["w"][0], N]), "null pointer"), ("NULL h table", dict(h=N), "required"),
           ("no destination", dict(q_out=N, backup=N), "destination"), ("no destination, tables of NULLs", dict(q_out=[N, N], backup=[N, N]), "destination"),
           ("backup without reward", dict(reward=[pr["r"][0], N]), "reward and done"), ("backup without done table", dict(done=N), "reward and done"),
           ("wrong device", dict(device=other_device), None)]
    for label, kw, contains in bad:
        rc = go(**kw)
        msg = _lib.last_error(None, L)
        assert rc != 0 and msg, (label, rc, msg)
        assert contains is None or contains in msg, (label, msg)
        sync(q[0])
        assert all((t == SENTINEL).all() for t in q + bk), label
    assert go(M=0) == 0
    sync(q[0])
    assert all((t == SENTINEL).all() for t in q + bk)
    assert go() == 0
    sync(q[0])
    assert not any((t == SENTINEL).any() for t in q + bk)


# ---- the modules of algorithms/marl/maddpg against the reference's recorded update (tests/golden/maddpg_update.npz) -----------------
# Gate of the losses: 1e-5 (1 + |stored|), the q_target fixture's; post-update parameters: 1e-5 absolute.

import ast
import copy
import os
import random
import types

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maddpg_update.npz")
NETS = ("actor", "critic", "actor_targ", "critic_targ")
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(GOLDEN))
    return _fixture


def spaces_of(obs, sobs, act, n):
    o, s = types.SimpleNamespace(shape=(obs,)), types.SimpleNamespace(shape=(sobs,))
    a = types.SimpleNamespace(shape=(act,), high=np.ones(act, np.float32))
    return o, s, a, [a] * n


def fixture_trainer(device, **kw):
    """The fixture's policies (parameters from the stored 16-bit words) and a MADDPG over them."""
    from massive_marl_benchmark_amd.algorithms.marl.maddpg import MADDPG, MADDPG_policy
    g = fixture()
    n, obs, sobs, act = (int(v) for v in g["shape"][:4])
    config = ast.literal_eval(str(g["config"]))
    o, s, a, joint = spaces_of(obs, sobs, act, n)
    policies = [MADDPG_policy(config, o, s, a, joint, device=device) for _ in range(n)]
    assert list(policies[0].actor.state_dict().keys()) == list(g["actor_keys"]) and list(policies[0].critic.state_dict().keys()) == list(g["critic_keys"])
    with torch.no_grad():
        for i, po in enumerate(policies):
            for name in NETS:
                flat = torch.from_numpy((g["agent%d_%s_bf16" % (i, name)].astype(np.uint32) << 16).view(np.float32)).to(device)
                at = 0
                for v in getattr(po, name).state_dict().values():
                    v.copy_(flat[at:at + v.numel()].view(v.shape))
                    at += v.numel()
                assert at == flat.numel()
    return config, policies, MADDPG(config, policies, n, device=device, **kw)


def fixture_buffers(config, device, shared_joint=False):
    """Our ReplayBuffers fed the recorded transitions through add_transitions."""
    from massive_marl_benchmark_amd.algorithms.marl.maddpg import ReplayBuffer
    g = fixture()
    n, obs, sobs, act = (int(v) for v in g["shape"][:4])
    a = types.SimpleNamespace(shape=(act,))
    buffers = []
    for i in range(n):
        buffers.append(ReplayBuffer(config, (obs,), (sobs,), (act,), [a] * n, device=device, joint_actions=buffers[0].joint_actions if shared_joint and i else None))
    fed = {k[4:]: torch.from_numpy(v).to(device) for k, v in g.items() if k.startswith("fed_")}
    for t in range(fed["obs"].shape[0]):
        for i, b in enumerate(buffers):
            b.add_transitions(fed["obs"][t, i], fed["share_obs"][t, i], fed["actions"][t, i], fed["joint_actions"][t, i], fed["rewards"][t, i],
                              fed["next_observations"][t, i], fed["next_share_obs"][t, i], fed["dones"][t, i])
    return buffers


def samples_of(buffers, indices):
    """What MADDPG.train hands to ddpg_update, gathered at the buffers' padded pitch."""
    out = []
    for b in buffers:
        K = b.obs.shape[-1]
        out.append({"obs": b.obs_padded[indices][..., :K], "sobs": b.share_obs[indices], "act": b.actions[indices], "jact": b.joint_actions[indices],
                    "r": b.rewards[indices], "obs2": b.next_observations_padded[indices][..., :K], "sobs2": b.next_share_obs[indices], "done": b.dones[indices]})
    return out


class Calls:
    """Counts the calls of the two new entries (and of the grouped layer) on library L."""
    NAMES = ("mms_det_heads_act_group", "mms_q_heads_backup_group", "mms_linear_group_act")

    def __init__(self, L, monkeypatch):
        self.n = {k: 0 for k in self.NAMES}
        for name in self.NAMES:
            real = getattr(L, name)

            def wrapped(*a, _real=real, _name=name):
                self.n[_name] += 1
                return _real(*a)
            monkeypatch.setattr(L, name, wrapped)

    def snapshot(self):
        return dict(self.n)


def close(got, stored):
    got = got.item() if torch.is_tensor(got) else got
    return abs(float(got) - float(stored)) <= 1e-5 * (1 + abs(float(stored)))


def check_storage(device):
    """The ring against the reference's recorded ring (an overflow included), the zero padding, slot() and the aliased joint ring."""
    g = fixture()
    config = ast.literal_eval(str(g["config"]))
    buffers = fixture_buffers(config, device)
    for i, b in enumerate(buffers):
        for k in ("obs", "share_obs", "actions", "joint_actions", "rewards", "next_observations", "next_share_obs", "dones"):
            assert np.array_equal(getattr(b, k).cpu().numpy(), g["ring_" + k][i]), (i, k)
        assert b.step == int(g["ring_step"][i]) and b.fullfill == bool(g["ring_fullfill"][i])
        K = b.obs.shape[-1]
        assert b.obs_padded.shape[-1] == 12 and K == 10 and b.obs.data_ptr() == b.obs_padded.data_ptr()
        assert (b.obs_padded[..., K:] == 0).all() and (b.next_observations_padded[..., K:] == 0).all()
    # slot(): rows 0 .. R-1, then (R + 1) % R = 1 and on; rows written in place are recognised by address
    b = fixture_buffers(config, device)[0].__class__(config, (10,), (18,), (2,), [types.SimpleNamespace(shape=(2,))] * 3, device=device)
    seen = []
    for t in range(9):
        k = b.slot()
        seen.append(k)
        b.actions[k].fill_(float(t + 1))
        z = lambda *s: torch.zeros(*s, device=device)
        b.add_transitions(z(5, 10), z(5, 18), b.actions[k], z(5, 6), z(5), z(5, 10), z(5, 18), z(5))
        assert b.step - 1 == k and (b.actions[k] == t + 1).all()
    assert seen == [0, 1, 2, 3, 4, 5, 1, 2, 3]
    shared = fixture_buffers(config, device, shared_joint=True)
    assert all(s.joint_actions.data_ptr() == shared[0].joint_actions.data_ptr() for s in shared)
    assert np.array_equal(shared[0].joint_actions.cpu().numpy(), g["ring_joint_actions"][0])     # (the recorded joint rows are the same for every agent)


def check_losses(device, L, monkeypatch):
    """cal_value_loss / cal_pi_loss per agent at the initial parameters; the fused entries ran; fused=False never runs them."""
    g = fixture()
    calls = Calls(L, monkeypatch)
    for fused in (True, False):
        config, policies, trainer = fixture_trainer(device, fused=fused)
        samples = samples_of(fixture_buffers(config, device), list(g["indices"]))
        before = calls.snapshot()
        for i in range(trainer.num_agents):
            v, p = trainer.cal_value_loss(samples, i), trainer.cal_pi_loss(samples, i)
            print("fused %d agent %d: value %.9g (stored %.9g) pi %.9g (stored %.9g)" % (fused, i, v.item(), g["value_loss_init"][i], p.item(), g["pi_loss_init"][i]))
            assert v.requires_grad and p.requires_grad
            assert close(v, g["value_loss_init"][i]) and close(p, g["pi_loss_init"][i]), (fused, i)
        after = calls.snapshot()
        ran = {k: after[k] - before[k] for k in after}
        if fused:
            # per agent: cal_value_loss = a target pass of all actors (1 head launch) + 1 Q tail; cal_pi_loss = 1 or 2 head launches
            assert ran["mms_q_heads_backup_group"] == 3 and ran["mms_det_heads_act_group"] == 3 + (1 + 2 + 1) and ran["mms_linear_group_act"] > 0, ran
        else:
            assert not any(ran.values()), ran
    # the other actors' gradients stay untouched on the fused path
    config, policies, trainer = fixture_trainer(device)
    samples = samples_of(fixture_buffers(config, device), list(g["indices"]))
    trainer.cal_pi_loss(samples, 1).backward()
    assert all(p.grad is None for a in (0, 2) for p in policies[a].actor.parameters()) and all(p.grad is not None for p in policies[1].actor.parameters())


def check_update(device, L, monkeypatch):
    """ddpg_update: the two loss lists, the post-update parameters, and the in-loop ordering of the target actors."""
    g = fixture()
    gate = lambda x: 1e-5 * (1 + abs(float(x)))
    for i in (1, 2):            # the fixture resolves the ordering: in-loop and all-targets-before-the-loop differ by >= 100 gates
        assert abs(g["value_loss_update"][i] - g["value_loss_pre"][i]) >= 100 * gate(g["value_loss_update"][i]), i
    calls = Calls(L, monkeypatch)
    for fused in (True, False):
        config, policies, trainer = fixture_trainer(device, fused=fused)
        samples = samples_of(fixture_buffers(config, device), list(g["indices"]))
        before = calls.snapshot()
        value_loss, policy_loss = trainer.ddpg_update(samples)
        ran = {k: calls.n[k] - before[k] for k in before}
        for i in range(3):
            print("fused %d agent %d: value %.9g (stored %.9g, pre %.9g) pi %.9g (stored %.9g)"
                  % (fused, i, value_loss[i].item(), g["value_loss_update"][i], g["value_loss_pre"][i], policy_loss[i].item(), g["pi_loss_update"][i]))
            assert close(value_loss[i], g["value_loss_update"][i]) and close(policy_loss[i], g["pi_loss_update"][i]), (fused, i)
        for name in ("actor_targ", "critic"):
            for i, po in enumerate(policies):
                sd = list(getattr(po, name).state_dict().values())
                assert np.abs(sd[0][0].cpu().numpy() - g["post_%s_w0_row0" % name][i]).max() <= 1e-5, (fused, name, i)
                assert np.abs(sd[-1].cpu().numpy() - g["post_%s_last_bias" % name][i]).max() <= 1e-5, (fused, name, i)
        if fused:
            # target actors: one grouped pass + a refresh behind agents 0 and 1 = N + (N - 1) actor passes in 3 head launches;
            # cal_pi_loss: 1 + 2 + 1 head launches; one Q tail per agent
            assert ran["mms_det_heads_act_group"] == 3 + 4 and ran["mms_q_heads_backup_group"] == 3, ran
        else:
            assert not any(ran.values()), ran


def check_train(device):
    g = fixture()
    config, policies, trainer = fixture_trainer(device)
    buffers = fixture_buffers(config, device, shared_joint=True)
    random.seed(5)
    infos = trainer.train(buffers)
    assert len(infos) == 3 and infos[0] is infos[1] is infos[2]
    for i, d in enumerate(infos):
        print("train agent %d: %r (stored %.9g %.9g)" % (i, d, g["train_value_loss"][i], g["train_policy_loss"][i]))
        assert sorted(d) == ["policy_loss", "value_loss"]
        assert close(d["value_loss"], g["train_value_loss"][i]) and close(d["policy_loss"], g["train_policy_loss"][i])


def check_target_critic(device, L, monkeypatch):
    """use_target_critic=True: the value loss with critic_targ.q in the backup, against the same expression through float64 copies of
    the modules, within the fixture's gate."""
    g = fixture()
    calls = Calls(L, monkeypatch)
    config, policies, trainer = fixture_trainer(device, use_target_critic=True)
    samples = samples_of(fixture_buffers(config, device), list(g["indices"]))
    p64 = [types.SimpleNamespace(critic=copy.deepcopy(po.critic).double(), critic_targ=copy.deepcopy(po.critic_targ).double(),
                                 actor_targ=copy.deepcopy(po.actor_targ).double()) for po in policies]
    for i in range(3):
        got = trainer.cal_value_loss(samples, i).item()
        with torch.no_grad():
            d = samples[i]
            q = p64[i].critic.q(d["sobs"].double(), d["jact"].double())
            jact2 = torch.cat([p64[v].actor_targ.pi(samples[v]["obs2"].double()) for v in range(3)], dim=-1)
            ref = float(((q - (d["r"].double() + config["gamma"] * (1 - d["done"].double()) * p64[i].critic_targ.q(d["sobs2"].double(), jact2))) ** 2).mean())
        print("use_target_critic agent %d: %.9g (float64 %.9g, online-critic fixture %.9g)" % (i, got, ref, g["value_loss_init"][i]))
        assert close(got, ref), i
        assert not close(got, g["value_loss_init"][i]), i             # (the perturbed target critic is another network)
    assert calls.n["mms_q_heads_backup_group"] == 3


def _err(x, x64):
    return float((x.double() - x64).abs().max() / (1 + x64.abs().max()))


def make_trainer(n, obs, sobs, act, hidden, device, seed=0, **kw):
    from massive_marl_benchmark_amd.algorithms.marl.maddpg import MADDPG, MADDPG_policy
    torch.manual_seed(seed)
    config = {"learning_rate": 1e-3, "hidden_size": list(hidden), "activation": "elu", "act_noise": 0.25, "num_learning_epochs": 2, "num_mini_batch": 1,
              "gamma": 0.99, "polyak": 0.5, "max_grad_norm": 1.0, "n_rollout_threads": 16, "replay_size": 6, "batch_size": 4, "sampler": "random"}
    o, s, a, joint = spaces_of(obs, sobs, act, n)
    policies = [MADDPG_policy(config, o, s, a, joint, device=device) for _ in range(n)]
    return config, policies, MADDPG(config, policies, n, device=device, **kw)


def check_act_all(device, L, monkeypatch, n=33, obs=10, act=3, hidden=(64,), M=16):
    """33 agents (two chunks of the 32-group limit), observation width 10 (padded rows): deterministic actions against the plain
    modules -- no worse than torch's fp32 against float64, err <= 2 err_torch + 1e-6 with err = max |x - x64| / (1 + max |x64|) --
    the slots hold what is returned, the joint row is the concatenation; exploration stays within the limit and advances the counters."""
    from massive_marl_benchmark_amd.algorithms.marl.maddpg import ReplayBuffer
    calls = Calls(L, monkeypatch)
    config, policies, trainer = make_trainer(n, obs, 12, act, hidden, device, seed=3)
    a = types.SimpleNamespace(shape=(act,))
    buffers = []
    for i in range(n):
        buffers.append(ReplayBuffer(config, (obs,), (12,), (act,), [a] * n, device=device, joint_actions=buffers[0].joint_actions if i else None))
    gen = torch.Generator().manual_seed(8)
    k = buffers[0].slot()
    for b in buffers:
        b.obs[k].copy_(torch.randn(M, obs, generator=gen).to(device))
    obs_list = [b.obs[k] for b in buffers]
    acts, joint = trainer.act_all(obs_list, deterministic=True, act_slots=[b.actions[k] for b in buffers], joint_slot=buffers[0].joint_actions[k])
    sync(joint)
    assert calls.n["mms_det_heads_act_group"] == 2 and calls.n["mms_linear_group_act"] == 2, calls.n          # 32 + 1 agents
    assert all(acts[i].data_ptr() == buffers[i].actions[k].data_ptr() for i in range(n)) and joint.data_ptr() == buffers[0].joint_actions[k].data_ptr()
    assert torch.equal(joint, torch.cat(acts, dim=-1))
    assert all(torch.equal(b.joint_actions[k], joint) for b in buffers)
    worst = 0.0
    for i, po in enumerate(policies):
        with torch.no_grad():
            plain = po.act(obs_list[i], deterministic=True)
            x64 = copy.deepcopy(po.actor).double().act(obs_list[i].double())
        ef, et = _err(acts[i], x64), _err(plain, x64)
        worst = max(worst, ef / (2 * et + 1e-6))
        assert ef <= 2 * et + 1e-6, (i, ef, et)
    print("act_all: worst err / (2 err_torch + 1e-6) = %.3g" % worst)
    # fresh tensors when no slots are given: the same bits
    acts2, joint2 = trainer.act_all(obs_list, deterministic=True)
    assert torch.equal(joint2, joint) and all(torch.equal(x, y) for x, y in zip(acts, acts2))
    # exploration
    noisy, jn = trainer.act_all(obs_list, deterministic=False)
    sync(jn)
    c = trainer._counters[(str(jn.device), M)]
    assert (c == 1).all() and not torch.equal(jn, joint) and float(jn.abs().max()) <= 1.0
    assert float((jn - joint).abs().max()) <= 0.25 * 6          # |z| < 6 for every one of 1584 draws
    trainer.act_all(obs_list, deterministic=False)
    assert (c == 2).all()
    # fused=False: the plain modules, never the entries, the same slots contract
    before = calls.snapshot()
    config, policies_off, off = make_trainer(n, obs, 12, act, hidden, device, seed=3, fused=False)
    acts3, joint3 = off.act_all(obs_list, deterministic=True, act_slots=[b.actions[k] for b in buffers], joint_slot=buffers[0].joint_actions[k])
    assert calls.snapshot() == before and torch.equal(joint3, torch.cat(acts3, dim=-1)) and _err(joint3, joint.double()) <= 1e-5


RUNNER_CONFIG = {"algorithm_name": "maddpg", "experiment_name": "check", "num_env_steps": 2 * 8 * 64, "episode_length": 8, "n_rollout_threads": 64,
                 "n_eval_rollout_threads": 64, "hidden_size": [64, 64], "use_render": False, "save_interval": 100, "use_eval": False, "eval_interval": 100,
                 "eval_episodes": 1, "log_interval": 1, "batch_size": 4, "replay_size": 6, "learning_rate": 1e-3, "activation": "elu", "act_noise": 0.1,
                 "num_learning_epochs": 2, "num_mini_batch": 1, "gamma": 0.99, "polyak": 0.995, "max_grad_norm": 1.0, "sampler": "random"}


def check_runner(device_type, L, monkeypatch, tmp_path):
    """TenAnt at 64 envs, two episodes of 8 steps into a ring of 6 rows: updates happen after the warm-up, losses are finite, the rows
    the head kernel wrote are found in place, one joint ring serves all agents, and no per-env host loop remains."""
    import inspect
    from massive_marl_benchmark_amd.algorithms.marl.maddpg import Runner
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.multi_vec_task import MultiVecTaskPython
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = 64
    cfg["clip_observations"] = 7.0
    cfg["seed"] = 3
    rl_device = "cpu" if device_type == "cpu" else "cuda:0"
    env = MultiVecTaskPython(TenAnt(cfg, None, "physx", device_type, 0, True, is_multi_agent=True), rl_device)
    calls = Calls(L, monkeypatch)
    random.seed(1)
    torch.manual_seed(1)
    runner = Runner(env, dict(RUNNER_CONFIG, run_dir=str(tmp_path)))
    in_place = []
    real_collect = runner.collect

    def collect(step):
        slots = [b.slot() for b in runner.buffer]
        acts, joint = real_collect(step)
        in_place.append(all(acts[a].data_ptr() == runner.buffer[a].actions[slots[a]].data_ptr() for a in range(runner.num_agents))
                        and joint.data_ptr() == runner.buffer[0].joint_actions[slots[0]].data_ptr())
        return acts, joint
    runner.collect = collect
    runner.run()
    assert runner.updates > 0 and not runner.warm_up and len(in_place) == 16 and all(in_place)
    assert all(np.isfinite(v) for d in runner.last_train_infos for v in d.values()), runner.last_train_infos
    assert all(b.joint_actions.data_ptr() == runner.buffer[0].joint_actions.data_ptr() for b in runner.buffer)
    b = runner.buffer[3]
    assert b.fullfill and b.obs.shape[-1] == 46 and b.obs_padded.shape[-1] == 48 and (b.obs_padded[..., 46:] == 0).all() and (b.next_observations_padded[..., 46:] == 0).all()
    assert torch.isfinite(b.obs).all() and torch.isfinite(b.rewards).all() and float(b.actions.abs().max()) <= 1.0 and float(b.actions.abs().max()) > 0
    assert torch.equal(b.joint_actions[..., 24:32], b.actions)
    assert calls.n["mms_det_heads_act_group"] >= 16 and calls.n["mms_q_heads_backup_group"] >= 10 * runner.updates      # TenAnt ran the fused paths
    assert os.path.exists(os.path.join(runner.save_dir, "actor_agent9.pt"))
    src = inspect.getsource(Runner.run)
    assert "for t in range" not in src and "n_rollout_threads):" not in src

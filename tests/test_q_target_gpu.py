"""The off-policy Q target (mms_q_heads_backup, csrc/q_kernels.hip; fused_q_forward / fused_q_backup / q_backup of
algorithms/rl/{ddpg,td3,sac}/module.py) on the MI355X: the kernel against float64 and against the CPU build, its exact properties
and error paths, the modules' fused chain against the same modules in float64 next to torch's fp32, the reference's compute_loss_q
fixture, graph replay, and the paths that must stay on torch."""
import copy

import numpy as np
import pytest

import q_check as qc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu():
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device("cuda:0")


def _make(algo, W, A, hidden, activation, **kw):
    from test_q_target import boxes
    from massive_marl_benchmark_amd.algorithms.rl.ddpg import module as ddpg_module
    from massive_marl_benchmark_amd.algorithms.rl.sac import module as sac_module
    from massive_marl_benchmark_amd.algorithms.rl.td3 import module as td3_module
    ob, ac = boxes(W, A)
    if algo == "sac":
        return sac_module.MLPActorCritic(ob, ac, hidden_sizes=hidden, activation=activation, **kw).cuda()
    mod = td3_module if algo == "td3" else ddpg_module
    return mod.MLPActorCritic(ob, ac, 0.1, "cuda:0", hidden_sizes=hidden, activation=activation, **kw).cuda()


def _critics(ac):
    return [ac.q] if hasattr(ac, "q") else [ac.q1, ac.q2]


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("M,H", [(65536, 1024), (8192, 256), (1000, 256), (7, 64), (333, 128), (37, 4096)])     # the last: H = MMS_Q_MAX_H
def test_kernel_against_float64(torch_cuda, M, H, G):
    torch = torch_cuda
    L, dev, stream = _gpu()
    pr = qc.problem(M, H, G, seed=1, device="cuda")
    for with_logp in (True, False):
        q, backup = qc.run(L, dev, stream, pr, with_logp=with_logp)
        torch.cuda.synchronize()
        for g in range(G):
            q64, s = qc.f64_q(pr, g)
            e = (np.abs(q[g].double().cpu().numpy() - q64) / s).max()
            t = torch.nn.functional.linear(pr["h"][g], pr["w"][g], pr["b"][g])[:, 0].double().cpu().numpy()
            et = (np.abs(t - q64) / s).max()
            print("M %d H %d G %d g %d: e = %.3g, e_torch = %.3g" % (M, H, G, g, e, et))
            assert e <= 2 * et + 1e-6, (e, et)
            qc.note("gpu", "q_heads_backup", "old", e / (2 * et + 1e-6))
        qc.check_backup(q, backup, pr, with_logp, 0.99, 0.2, "gpu M %d H %d G %d logp %d" % (M, H, G, with_logp))


@pytest.fixture
def no_dispatch_override():
    import os
    found = [v for v in qc.DISPATCH_ENV if v in os.environ]
    if found:
        pytest.fail("%s set in the environment: not the shipped dispatch; unset to run these tests" % ", ".join(found))


@pytest.mark.parametrize("M,H,G", qc.CASES)
def test_path_table(torch_cuda, no_dispatch_override, M, H, G):
    """q_heads_backup_kernel<G> with each part of its k-loop (qc.expected_path): the unrolled loop, the remainder loop, and both in one
    call."""
    L, dev, stream = _gpu()
    qc.check_case(L, dev, stream, "cuda", M, H, G)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("mutation", ["chunk", "last"])
def test_gate_sees_a_dropped_chunk_or_element(torch_cuda, no_dispatch_override, mutation, G):
    """test_q_target.py's, with the device's gate."""
    L, dev, stream = _gpu()
    assert qc.check_case(L, dev, stream, "cuda", 33, 576, G, mutation=mutation) >= 10


def test_exact_properties(torch_cuda):
    L, dev, stream = _gpu()
    qc.exact_properties(L, dev, stream, qc.problem(1000, 256, 2, seed=9, device="cuda"))
    qc.exact_properties(L, dev, stream, qc.problem(1000, 1024, 2, seed=10, device="cuda"))
    qc.exact_properties(L, dev, stream, qc.problem(1000, 4096, 2, seed=11, device="cuda"))      # the widest layer the entry takes


def test_abi_errors(torch_cuda):
    L, dev, stream = _gpu()
    qc.check_error_paths(L, dev, stream, other_device=-1)


@pytest.mark.parametrize("M,H", [(1000, 256), (333, 128), (4096, 1024)])
def test_kernel_against_cpu_build(torch_cuda, M, H):
    """|q_gpu - q_cpu| <= 1e-5 s: the two builds sum in different orders (16 interleaved fmaf chains and a butterfly on the device,
    one chain over k on the host), the bound and its reasoning are test_sac_actor_gpu.py::test_kernel_against_cpu_build's.  The
    backups then differ by at most the backup's gate (q_check) plus gamma times the q difference."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu()
    pr = qc.problem(M, H, 2, seed=4)
    prg = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in pr.items()}
    qc_, bc = qc.run(_lib.lib_cpu(), -1, None, pr)
    qg, bg = qc.run(L, dev, stream, prg)
    torch.cuda.synchronize()
    dq = np.zeros(M)
    for g in range(2):
        _, s = qc.f64_q(pr, g)
        diff = np.abs(qg[g].double().cpu().numpy() - qc_[g].double().numpy())
        print("M %d H %d g %d: max |q_gpu - q_cpu| / s = %.3g" % (M, H, g, (diff / s).max()))
        assert (diff <= 1e-5 * s).all()
        dq = np.maximum(dq, diff)
    _, gate = qc.f64_backup(qc_, pr, True, 0.99, 0.2)
    db = np.abs(bg.double().cpu().numpy() - bc.double().numpy())
    print("M %d H %d: max |backup_gpu - backup_cpu| / (gate + gamma dq) = %.3g" % (M, H, (db / (gate + 0.99 * dq + 1e-30)).max()))
    assert (db <= gate + 0.99 * dq).all()


def _err(x, x64):
    return float((x.double() - x64).abs().max() / (1 + x64.abs().max()))


CASES = [("sac", 1024, "ELU"), ("sac", 256, "ELU"), ("sac", 1024, "ReLU"), ("sac", 256, "ReLU"), ("td3", 256, "ReLU"), ("ddpg", 1024, "ELU")]


@pytest.mark.parametrize("algo,width,act", CASES)
def test_module_on_device(torch_cuda, algo, width, act):
    """A fused path is no worse than torch's fp32 modules: err(fused) <= 2 err(torch fp32) + 1e-6 against the same module in float64,
    err(x) = max |x - x64| / (1 + max |x64|), for the separate q(o2, a2) calls and for the one-chain q_backup; again after an Adam step
    on the online critics and a polyak .data write into the target (nothing is cached)."""
    torch = torch_cuda
    nn = torch.nn
    torch.manual_seed(3)
    W, A, N = 52, 24, 1024
    activation = getattr(nn, act)
    online = _make(algo, W, A, (width,) * 3, activation, fused_q=True)
    targ = copy.deepcopy(online)
    g = torch.Generator(device="cuda").manual_seed(5)
    o2 = torch.randn(8, N, W, device="cuda", generator=g)
    a2 = torch.rand(8, N, A, device="cuda", generator=g) * 2 - 1
    r = torch.randn(8, N, 1, device="cuda", generator=g)
    d8 = (torch.rand(8, N, 1, device="cuda", generator=g) < 0.3).to(torch.uint8)
    logp = torch.randn(8, N, 1, device="cuda", generator=g) * 2 - 3
    extra = (0.2, logp) if algo == "sac" else ()
    extra64 = (0.2, logp.double()) if algo == "sac" else ()

    def compare(what):
        plain = copy.deepcopy(targ)
        for m in (plain, *_critics(plain)):
            m.fused_q = False
        t64 = copy.deepcopy(plain).double()
        with torch.no_grad():
            q_f = [q(o2, a2) for q in _critics(targ)]
            q_t = [q(o2, a2) for q in _critics(plain)]
            q_64 = [q(o2.double(), a2.double()) for q in _critics(t64)]
            b_f = targ.q_backup(o2, a2, r, d8, 0.99, *extra)
            b_t = plain.q_backup(o2, a2, r, d8, 0.99, *extra)
            b_64 = t64.q_backup(o2.double(), a2.double(), r.double(), d8, 0.99, *extra64)
        assert b_f.shape == r.shape and all(q.shape == (8, N, 1) for q in q_f)
        for name, f, t, x64 in [("q%d" % i, q_f[i], q_t[i], q_64[i]) for i in range(len(q_f))] + [("backup", b_f, b_t, b_64)]:
            ef, et = _err(f, x64), _err(t, x64)
            print("%s %s %d %s %s: err fused %.3g, err torch %.3g" % (what, algo, width, act, name, ef, et))
            assert ef <= 2 * et + 1e-6, (what, name, ef, et)
        done = d8 != 0
        assert torch.equal(b_f[done], r[done])
        return b_f

    first = compare("initial")
    # d as uint8, bool and float: the same backup
    for d in (d8.bool(), d8.float()):
        assert torch.equal(targ.q_backup(o2, a2, r, d, 0.99, *extra), first)
    # an Adam step on the online critics, then the polyak write into the target (sac.py:354-359)
    params = [p for q in _critics(online) for p in q.parameters()]
    opt = torch.optim.Adam(params, lr=1e-2)
    loss = sum(((q(o2[0], a2[0]) - r[0]) ** 2).mean() for q in _critics(online))
    assert loss.requires_grad                                       # grad enabled, parameters requiring grad: the torch path
    loss.backward()
    opt.step()
    with torch.no_grad():
        for p, p_targ in zip(online.parameters(), targ.parameters()):
            p_targ.data.mul_(0.5)
            p_targ.data.add_(0.5 * p.data)
    second = compare("after update")
    assert not torch.equal(first, second)


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_reference_fixture_through_fused_path(torch_cuda, algo, monkeypatch):
    from conftest import load_golden
    from test_q_target import fixture_loss, fixture_target
    L, _, _ = _gpu()
    calls = []
    real = L.mms_q_heads_backup
    monkeypatch.setattr(L, "mms_q_heads_backup", lambda *a: (calls.append(1), real(*a))[1])
    g = load_golden("q_target")
    loss, stored = fixture_loss(g, algo, fixture_target(g, algo, device="cuda", fused_q=True), device="cuda")
    print("loss_q %.9g stored %.9g" % (loss, stored))
    assert len(calls) == 1                                          # the fused chain ran
    assert abs(loss - stored) <= 1e-5 * (1 + stored)


def test_graph_replay_follows_the_parameters(torch_cuda):
    torch = torch_cuda
    torch.manual_seed(2)
    W, A, N = 52, 24, 512
    targ = _make("sac", W, A, (256, 256, 256), torch.nn.ELU, fused_q=True)
    other = _make("sac", W, A, (256, 256, 256), torch.nn.ELU, fused_q=True)
    o2, a2 = torch.randn(8, N, W, device="cuda"), torch.rand(8, N, A, device="cuda") * 2 - 1
    r, d = torch.randn(8, N, 1, device="cuda"), (torch.rand(8, N, 1, device="cuda") < 0.3).to(torch.uint8)
    logp = torch.randn(8, N, 1, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        targ.q_backup(o2, a2, r, d, 0.99, 0.2, logp)                # warm-up
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = targ.q_backup(o2, a2, r, d, 0.99, 0.2, logp)
        g.replay()
        s.synchronize()
        first = out.clone()
        assert torch.equal(first, targ.q_backup(o2, a2, r, d, 0.99, 0.2, logp))
        with torch.no_grad():
            for p, p_targ in zip(other.parameters(), targ.parameters()):
                p_targ.data.mul_(0.9)
                p_targ.data.add_(0.1 * p.data)
        g.replay()
        s.synchronize()
        second = out.clone()
        assert torch.equal(second, targ.q_backup(o2, a2, r, d, 0.99, 0.2, logp))
        assert not torch.equal(first, second)
    torch.cuda.current_stream().wait_stream(s)


def test_gradients_and_fused_q_false_stay_on_torch(torch_cuda, monkeypatch):
    torch = torch_cuda
    L, _, _ = _gpu()
    calls = []
    real = L.mms_q_heads_backup
    monkeypatch.setattr(L, "mms_q_heads_backup", lambda *a: (calls.append(1), real(*a))[1])
    torch.manual_seed(6)
    W, A, N = 52, 24, 256
    ac = _make("sac", W, A, (256, 256), torch.nn.ELU, fused_q=True)
    o, a = torch.randn(N, W, device="cuda"), torch.rand(N, A, device="cuda")
    q = ac.q1(o, a)                                                 # compute_loss_q's online critic: parameters want a gradient
    assert q.requires_grad and not calls
    for p in ac.q1.parameters():
        p.requires_grad_(False)                                     # compute_loss_pi: frozen critics, the action wants one
    ag = a.clone().requires_grad_(True)
    q = ac.q1(o, ag)
    assert q.requires_grad and not calls
    q.sum().backward()
    assert ag.grad is not None
    assert not ac.q1(o, a).requires_grad and len(calls) == 1         # nothing wants a gradient: fused, even with grad mode on
    with torch.no_grad():
        ac.q2(o, a)
    assert len(calls) == 2
    # fused_q=False: never the new entry, and torch's bits
    off = _make("sac", W, A, (256, 256), torch.nn.ELU, fused_q=False)
    r, d = torch.randn(N, 1, device="cuda"), torch.zeros(N, 1, dtype=torch.uint8, device="cuda")
    with torch.no_grad():
        q1 = off.q1(o, a)
        b = off.q_backup(o, a, r, d, 0.99)
        assert torch.equal(q1, off.q1.q(torch.cat([o, a], dim=-1)))
        assert torch.equal(b, r + 0.99 * (1 - d.float()) * torch.min(q1, off.q2(o, a)))
    assert len(calls) == 2
    # a parameter the kernels cannot read in place (a view 4 bytes past a 16-byte boundary, as in a flat parameter buffer): torch,
    # decided before the first launch
    last = ac.q2.q[4]
    flat = torch.zeros(last.weight.numel() + 1, device="cuda")
    flat[1:].copy_(last.weight.data.view(-1))
    last.weight.data = flat[1:].view(1, -1)
    assert last.weight.data_ptr() % 16 == 4
    with torch.no_grad():
        assert torch.equal(ac.q2(o, a), ac.q2.q(torch.cat([o, a], dim=-1)))
    assert len(calls) == 2
    # shapes the kernels do not take: torch, not an error (W + A not a multiple of 4)
    odd = _make("sac", 51, 24, (256, 256), torch.nn.ELU, fused_q=True)
    with torch.no_grad():
        assert odd.q1(torch.randn(N, 51, device="cuda"), a).shape == (N, 1)
    assert len(calls) == 2

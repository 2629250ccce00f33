"""SAC's fused policy head (mms_sac_heads_act, csrc/sac_kernels.hip) and actor-critic (algorithms/rl/sac/module.py) on the MI355X:
the kernel against float64 and against the CPU build, the noise it draws, the module's fused path against its torch path, graph
replay and SAC's collection loop."""
import copy

import numpy as np
import pytest

import sac_check as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def _gpu(torch):
    from massive_marl_benchmark_amd import _lib
    return _lib.for_device("cuda:0")


def _ac(W, A, hidden, limit=1.0, **kw):
    from massive_marl_benchmark_amd import spaces
    from massive_marl_benchmark_amd.algorithms.rl.sac import MLPActorCritic
    return MLPActorCritic(spaces.Box(-np.inf * np.ones(W), np.inf * np.ones(W)), spaces.Box(-limit * np.ones(A), limit * np.ones(A)),
                          hidden_sizes=hidden, **kw)


SHAPES = [(4096, 1024, 80), (8192, 1024, 24), (1000, 256, 8), (7, 64, 3), (333, 128, 17), (256, 64, 128)]


@pytest.mark.parametrize("N,H,A", SHAPES)
def test_kernel_against_float64(torch_cuda, N, H, A):
    L, dev, stream = _gpu(torch_cuda)
    sc.check_kernel(L, dev, stream, "cuda", N, H, A, kind="old")


@pytest.fixture
def no_dispatch_override():
    import os
    found = [v for v in sc.qc.DISPATCH_ENV if v in os.environ]
    if found:
        pytest.fail("%s set in the environment: not the shipped dispatch; unset to run these tests" % ", ".join(found))


@pytest.mark.parametrize("N,H,A", sc.CASES)
def test_kernel_table(torch_cuda, no_dispatch_override, N, H, A):
    """One case per sac_head_act_kernel<NCT, WAVES> and per way to reach it (sc.expected_kernel): sampled and deterministic, with and
    without logp_slot."""
    L, dev, stream = _gpu(torch_cuda)
    sc.check_case(L, dev, stream, "cuda", N, H, A)


@pytest.mark.parametrize("mutation", ["tile", "last"])
def test_gate_sees_a_dropped_tile_or_column(torch_cuda, no_dispatch_override, mutation):
    """test_sac_actor.py's, with the device's e_torch in the gate."""
    L, dev, stream = _gpu(torch_cuda)
    assert sc.check_kernel(L, dev, stream, "cuda", 33, 768, 113, mutation=mutation) >= 10
    assert sc.check_kernel(L, dev, stream, "cuda", 17, 256, 128, mutation=mutation) >= 10


@pytest.mark.parametrize("N,H,A", [(1000, 256, 8), (333, 128, 17), (512, 1024, 80)])
def test_kernel_against_cpu_build(torch_cuda, N, H, A):
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L, dev, stream = _gpu(torch)
    h, mw, mb, lw, lb = sc.problem(N, H, A, seed=2 * N + A)
    counters = torch.arange(N, dtype=torch.int64) % 4
    cpu = sc.run(_lib.lib_cpu(), -1, None, h, mw, mb, lw, lb, act_limit=2.0, seed=21, counters=counters.clone(), row_offset=8)
    gpu = sc.run(L, dev, stream, *(t.cuda() for t in (h, mw, mb, lw, lb)), act_limit=2.0, seed=21, counters=counters.cuda(), row_offset=8)
    torch.cuda.synchronize()
    g = {k: v.double().cpu().numpy() for k, v in gpu.items()}
    c = {k: v.double().numpy() for k, v in cpu.items()}
    _, _, s_mu, s_ls = sc.f64_head(h, mw, mb, lw, lb)
    std, z = np.exp(c["log_std"]), np.abs(c["u"] - c["mu"]) / np.exp(c["log_std"])
    du = np.abs(g["u"] - c["u"])
    # 1e-5 relative to the scale of what u is computed from, not to |u| alone: the two builds sum the GEMMs in different orders
    # (MFMA k-permuted per wave, then wave partials; an fmaf chain on the host), so mu and log_std differ by a few ulp of
    # sum_k |h_k w_jk| even where |u| is small, and z by the device's fast logf / cosf (scaled by std)
    scale = np.abs(c["u"]) + s_mu + std * (1 + z) * (1 + s_ls)
    assert (du <= 1e-5 * scale).all(), (du / scale).max()
    t = c["action"] / 2.0
    assert (np.abs(g["action"] - c["action"]) <= 2.0 * (8 * sc.ULP1 + (1 - t * t) * du)).all()
    assert (np.abs(g["logp"] - c["logp"]) <= sc.logp_gate(t, du, 1e-6)).all()


def test_noise_statistics(torch_cuda):
    torch = torch_cuda
    L, dev, stream = _gpu(torch)
    N, A = 4096, 80                                                # 327 680 draws per call
    counters = torch.zeros(N, dtype=torch.int64, device="cuda")
    z1 = sc.draws(L, dev, stream, 1234, counters, 0, N, A).double()
    z2 = sc.draws(L, dev, stream, 1234, counters + 1, 0, N, A).double()
    for z in (z1, z2):
        assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1) < 0.01
    r = float(((z1 - z1.mean()) * (z2 - z2.mean())).mean() / (z1.std() * z2.std()))
    assert abs(r) < 0.01, r
    # z = (u - mu) / std of a real call (sample mode) has the same statistics
    h, mw, mb, lw, lb = (t.cuda() for t in sc.problem(N, 64, A, seed=1, scaled=False))
    out = sc.run(L, dev, stream, h, mw, mb, lw, lb, seed=99, counters=counters.clone())
    zz = ((out["u"].double() - out["mu"].double()) / out["log_std"].double().exp())
    assert abs(float(zz.mean())) < 0.01 and abs(float(zz.std()) - 1) < 0.01


def test_module_on_device(torch_cuda):
    torch = torch_cuda
    torch.manual_seed(0)
    N, W, A = 1024, 48, 24
    ac = _ac(W, A, (256, 256, 256), limit=1.0).cuda()
    pi = ac.pi
    o = torch.randn(N, W, device="cuda")
    with torch.no_grad():
        mu = pi.mu_layer(pi.net(o))
    a = ac.act(o, deterministic=True)
    assert (a - torch.tanh(mu)).abs().max() <= 2e-5
    assert pi._counters is None                                    # deterministic: nothing drawn, no counters made

    def fused_vs_torch(o2, what):
        with torch.no_grad():
            c0 = pi.counters(o2.reshape(-1, W).shape[0], o2.device).clone()
            a2, logp2 = pi(o2)
            assert torch.equal(pi._counters[:c0.numel()], c0 + 1), what
            L, dev, stream = _gpu(torch)
            eps = sc.draws(L, dev, stream, pi.seed, c0, pi.row_offset, c0.numel(), A).view(*o2.shape[:-1], A)
            ta, tlogp = pi.torch_forward(o2, eps=eps)
        assert a2.shape == o2.shape[:-1] + (A,) and logp2.shape == o2.shape[:-1] + (1,), what
        assert (a2 - ta).abs().max() <= 2e-5, (what, float((a2 - ta).abs().max()))
        t = ta.double().cpu().numpy()
        du = 2e-5 * (1 + np.abs(np.arctanh(np.clip(t, -1 + 1e-7, 1 - 1e-7))))
        gate = sc.logp_gate(t, du, 1e-6)
        assert (np.abs(logp2.double().cpu().numpy() - tlogp.double().cpu().numpy())[..., 0] <= gate).all(), what

    o2 = torch.randn(8, N, W, device="cuda")                       # sac.py:376: the gathered minibatch [rows, envs, obs]
    fused_vs_torch(o2, "pi(o2)")
    # after an Adam step on pi and a polyak .data write the fused path reads the new parameters (nothing cached)
    opt = torch.optim.Adam(pi.parameters(), lr=1e-2)
    _, logp = pi(o)
    (-logp.mean()).backward()
    opt.step()
    targ = copy.deepcopy(ac)
    with torch.no_grad():
        for p, pt in zip(ac.parameters(), targ.parameters()):
            pt.data.mul_(0.5).add_(torch.randn_like(pt) * 0.01)
            p.data.mul_(0.99).add_(0.01 * pt.data)
    fused_vs_torch(o2, "after the update")


def test_graph_capture_draws_fresh_noise(torch_cuda):
    torch = torch_cuda
    torch.manual_seed(1)
    N, W, A = 2048, 64, 8
    ac = _ac(W, A, (128, 128)).cuda()
    o = torch.randn(N, W, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.act(o)                                                  # warm-up: the counters exist before the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ac.act(o)
        c0 = ac.pi._counters.clone()
        g.replay()
        first = out.clone()
        g.replay()
        second = out.clone()
        s.synchronize()
    assert torch.equal(ac.pi._counters, c0 + 2)
    assert not torch.equal(first, second)
    ac.pi._counters.copy_(c0)
    assert torch.equal(ac.act(o), first)                           # each replay = the eager call at the same counters
    assert torch.equal(ac.act(o), second)


def test_graph_capture_then_target_rows(torch_cuda):
    """SAC's flow: act captured at N rows, then the Q target's pi(o2) on 8 x N rows of the same actor.  With the counters reserved
    for 8 N before the capture, nothing moves: the replays and the eager calls share one counter tensor."""
    torch = torch_cuda
    torch.manual_seed(3)
    N, W, A = 1024, 64, 8
    ac = _ac(W, A, (128, 128)).cuda()
    pi = ac.pi
    o, o2 = torch.randn(N, W, device="cuda"), torch.randn(8, N, W, device="cuda")
    pi.reserve_counters(8 * N, torch.device("cuda:0"))
    ptr = pi._counters.data_ptr()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.act(o)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ac.act(o)
        s.synchronize()
    assert pi._counters_pinned and pi._counters.data_ptr() == ptr
    with torch.no_grad():
        a2, logp2 = pi(o2)                                         # 8 N rows: served by the reserved tensor
    assert pi._counters.data_ptr() == ptr and a2.shape == (8, N, A) and torch.isfinite(logp2).all()
    c0 = pi._counters.clone()
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert torch.equal(pi._counters[:N], c0[:N] + 1) and torch.equal(pi._counters[N:], c0[N:])
    pi._counters.copy_(c0)
    assert torch.equal(ac.act(o), replayed)
    with pytest.raises(RuntimeError, match="reserve_counters"):
        with torch.no_grad():
            pi(torch.randn(8 * N + 1, W, device="cuda"))           # more rows than reserved: refused, nothing moved
    assert pi._counters.data_ptr() == ptr
    del g


def test_input_that_wants_grad_takes_the_torch_path(torch_cuda):
    torch = torch_cuda
    ac = _ac(16, 4, (64, 64)).cuda().requires_grad_(False)
    o = torch.randn(32, 16, device="cuda", requires_grad=True)
    a, logp = ac.pi(o)
    assert a.requires_grad and logp.requires_grad
    with torch.no_grad():
        a, _ = ac.pi(o)
    assert not a.requires_grad


def test_collection_loop_multi_ingenuity(torch_cuda):
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.sac import ReplayBuffer
    from massive_marl_benchmark_amd.engine import Engine
    from massive_marl_benchmark_amd.model import default_cfg
    N = 1024
    cfg = default_cfg("MultiIngenuity")
    cfg["env"]["envSpacing"] = 0.0
    eng = Engine("MultiIngenuity", cfg=cfg, num_envs=N, device=0, seed=3, clip_obs=5.0)
    W, AD = eng.obs_dim, eng.num_actions
    torch.manual_seed(2)
    ac = _ac(W, AD, (1024, 1024, 1024)).cuda()
    buf = ReplayBuffer(N, 16, 32, 8, (W,), (0,), (AD,), "cuda:0")
    states = torch.zeros(N, 0, device="cuda")
    act_buf, rew, done, obs_c = eng.tensor("actions"), eng.tensor("rew"), eng.tensor("reset"), eng.tensor("obs_clipped")
    eng.reset_all()
    eng.step()
    cur = obs_c.clone()
    for _ in range(8):                                             # sac.py:164-172
        a = ac.act(cur)
        act_buf.copy_(a)
        eng.step()
        buf.add_transitions(cur, states, a, rew, obs_c, done)
        cur.copy_(obs_c)
    torch.cuda.synchronize()
    assert buf.step == 8
    acts = buf.actions[:8]
    assert torch.isfinite(acts).all() and (acts.abs() <= 1.0).all() and torch.isfinite(buf.next_observations[:8]).all()
    assert torch.equal(ac.pi._counters[:N], torch.full((N,), 8, dtype=torch.int64, device="cuda"))
    eng.close()

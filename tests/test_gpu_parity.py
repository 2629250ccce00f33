"""GPU parity tests (run with -m gpu on the MI355X box).  Everything goes through the C ABI
(massive_marl_benchmark_amd/lib/libmms.so via ctypes) and is checked against the CPU oracle and the golden
vectors produced from the reference's own functions.  Nothing here reads /root/reference.

Gates: tests/parity.py (shared with tests/test_lane_emulation.py); integer outputs are bit-exact."""
import copy
import ctypes
import os

import numpy as np
import pytest

import parity
from conftest import ROOT, angle_close, load_golden, random_dr_params, shove_ants_into_box

pytestmark = pytest.mark.gpu

STATE = parity.STATE

# Gates: tests/parity.py (physics against the double-precision evaluation of the same step, epilogue on the kernel's own state,
# integer outputs bit-exact); every teacher-forced test records its measured margins (gpurun_out/parity_margins.json).


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


def task_kw(task, **kw):
    """MultiIngenuity envs away from the global origin die on every step (its reward measures distances in the GLOBAL frame,
    multi_ingenuity.py:381-453): the physics tests keep them at the origin."""
    if task in ("MultiIngenuity", "MultiAntCircle") and "cfg" not in kw:
        from massive_marl_benchmark_amd.model import default_cfg
        cfg = default_cfg(task)
        cfg["env"]["envSpacing"] = 0.0
        kw["cfg"] = cfg
    return kw


def make_pair(task, **kw):
    from massive_marl_benchmark_amd.engine import Engine
    from oracle.oracle import OracleEngine
    return Engine(task, device=0, **kw), OracleEngine(task, **kw)


def to_np(t):
    return t.detach().cpu().numpy()


def push_state(torch, eng, ora):
    for name in STATE:
        eng.tensor(name).copy_(torch.from_numpy(np.ascontiguousarray(ora.tensor(name))).to(eng.device))


def forced(eng, ora, dr=None):
    return parity.TeacherForced(ora, lambda k: to_np(eng.tensor(k)), dr=dr)


def drive(torch, eng, ora, tf, act, what):
    """One teacher-forced step: identical state and actions in, both step, every gate of tests/parity.py."""
    push_state(torch, eng, ora)
    tf.before(act)
    eng.tensor("actions").copy_(torch.from_numpy(act).to(eng.device))
    eng.step()
    ora.step(act)
    torch.cuda.synchronize()
    tf.after(what)


# (6 and 7 envs: a partial last workgroup of the packed layouts -- 4 envs per 192-thread block / per wave)
@pytest.mark.parametrize("task,n,steps", [("TenAnt", 64, 150), ("OneAnt", 64, 150), ("MultiIngenuity", 64, 150),
                                           ("TenAnt", 6, 60), ("OneAnt", 7, 60), ("MultiIngenuity", 5, 60), ("MultiAntCircle", 64, 150),
                                           ("MultiAntCircle", 5, 60)])
def test_teacher_forced_parity_vs_oracle(torch_cuda, task, n, steps):
    """K >= 100 steps, step for step on identical state and actions, resets included."""
    torch = torch_cuda
    eng, ora = make_pair(task, **task_kw(task, num_envs=n, seed=5, total_envs=4096, env_offset=1000))
    tf = forced(eng, ora)
    rng = np.random.default_rng(1)
    for t in range(steps):
        act = rng.uniform(-1.2, 1.2, (n, ora.num_actions)).astype(np.float32)      # beyond +-1: the clamp is exercised
        if task == "MultiIngenuity":
            act[:, 2::3] = np.abs(act[:, 2::3]) * 0.12
        drive(torch, eng, ora, tf, act, "%s step %d" % (task, t))
    tf.finish("gpu/teacher_forced/%s/n%d" % (task, n), min_live_steps=steps // 2)
    assert tf.resets > n or n < 16                       # more than the first-step reset: natural terminations happened
    eng.close()


@pytest.mark.parametrize("task,n,rule", [("TenAnt", 10, "average"), ("OneAnt", 9, "average"), ("TenAnt", 7, "min"), ("OneAnt", 6, "min")])
def test_ant_box_contact_parity(torch_cuda, task, n, rule):
    """Teacher-forced parity while the ants are pressed against the box: narrow phase, contact fold (with ant-box friction under
    the default `average` combine rule, rank 1 under `min`), per-ant reaction sums through LDS and the box solve with a
    non-zero wrench.  The box must feel the ants (its x velocity goes negative)."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.model import default_cfg
    cfg = default_cfg(task)
    cfg["env"]["frictionCombine"] = rule
    eng, ora = make_pair(task, cfg=cfg, num_envs=n, seed=11, total_envs=64, env_offset=7)
    assert abs(eng.config.model.antbox_mu - (0.75 if rule == "average" else 0.0)) < 1e-7
    tf = forced(eng, ora)
    rng = np.random.default_rng(4)
    zero = np.zeros((n, ora.num_actions), np.float32)
    for _ in range(12):
        ora.step(zero)
    shove_ants_into_box(ora, rng)
    pushed = 0.0
    A = ora.num_agents
    for t in range(40):
        act = rng.uniform(-1, 1, (n, ora.num_actions)).astype(np.float32)
        drive(torch, eng, ora, tf, act, "%s contact step %d" % (task, t))
        pushed = min(pushed, float(ora.tensor("root_states").reshape(n, A + 1, 13)[:, A, 7].min()))
        if t == 20:
            shove_ants_into_box(ora, rng)
    tf.finish("gpu/ant_box_contact/%s/%s" % (task, rule))
    assert pushed < -1e-3, pushed
    eng.close()


@pytest.mark.parametrize("task,n", [("TenAnt", 9), ("OneAnt", 10)])
def test_domain_randomised_physics_parity(torch_cuda, task, n):
    """mms_set_dr: per-ant mass / damping scales and joint-limit offsets through the DR instantiation of the step kernel,
    teacher forced against the oracle; and the switch really switches."""
    torch = torch_cuda
    eng, ora = make_pair(task, num_envs=n, seed=13, total_envs=64, env_offset=2)
    rng = np.random.default_rng(9)
    dr = random_dr_params(rng, n * ora.num_agents)
    ora.tensor("dr_params")[...] = dr
    ora.set_dr(True)
    assert float(eng.tensor("dr_params")[:, :17].min()) == 1.0 and float(eng.tensor("dr_params")[:, 17:].abs().max()) == 0.0
    eng.tensor("dr_params").copy_(torch.from_numpy(dr).to(eng.device))
    eng.set_dr(True)
    tf = forced(eng, ora, dr=dr)
    for t in range(80):
        act = rng.uniform(-1.2, 1.2, (n, ora.num_actions)).astype(np.float32)
        drive(torch, eng, ora, tf, act, "%s DR step %d" % (task, t))
    tf.finish("gpu/domain_randomised/%s" % task)
    eng.set_dr(False)                                          # nominal kernel again: now it must differ from the DR oracle
    push_state(torch, eng, ora)
    eng.tensor("actions").copy_(torch.from_numpy(act).to(eng.device))
    eng.step()
    ora.step(act)
    torch.cuda.synchronize()
    assert np.max(np.abs(to_np(eng.tensor("dof_state")) - ora.tensor("dof_state"))) > 1e-3
    eng.close()


@pytest.mark.parametrize("task,n", [("TenAnt", 8), ("OneAnt", 9)])
def test_box_ground_friction_parity(torch_cuda, task, n):
    """cfg env.boxGroundFriction = 0.5: the friction branch of the box phase (27-value corner reduction + 6x6 solve) against the
    oracle while ants push the box, and the frictionless branch (`boxGroundFriction: 0`) beside it.

    What friction means physically is asserted on the KERNEL's own state in a coast phase behind the push: the ants are lifted
    away from the box (no contact any more), and from then on a box on mu = 0.5 ground decelerates at mu g = 4.9 m/s^2 and rests
    within a few steps, while on mu = 0 it keeps its horizontal speed to rounding.  (During the push itself "mu = 0.5 is slower"
    does NOT hold and round 2 was right to drop it: with ant-box friction 0.75 (the `average` rule) the ants drag the box
    sideways while it is pinned against ground friction, and the peak corner speed came out 0.655 m/s on mu = 0.5 against
    0.510 m/s on mu = 0 -- the mechanism is pinned by tests/test_oracle_physics.py::test_ant_box_friction_drags_the_box_sideways
    and ::test_box_ground_friction_option; the push-phase peak speeds are recorded in the margins file.)"""
    torch = torch_cuda
    from massive_marl_benchmark_amd.model import default_cfg
    push_speed, coast = {}, {}
    for mu in (0.5, 0.0):
        cfg = default_cfg(task)
        cfg["env"]["boxGroundFriction"] = mu
        eng, ora = make_pair(task, cfg=cfg, num_envs=n, seed=17, total_envs=64, env_offset=5)
        tf = forced(eng, ora)
        rng = np.random.default_rng(3)
        zero = np.zeros((n, ora.num_actions), np.float32)
        for _ in range(12):
            ora.step(zero)
        shove_ants_into_box(ora, rng)
        A = ora.num_agents
        for t in range(50):
            act = rng.uniform(-1, 1, (n, ora.num_actions)).astype(np.float32)
            drive(torch, eng, ora, tf, act, "%s box friction %.1f step %d" % (task, mu, t))
        tf.finish("gpu/box_ground_friction/%s/mu%.1f" % (task, mu))
        push_speed[mu] = float(np.abs(ora.tensor("root_states").reshape(n, A + 1, 13)[:, A, 7:9]).max())
        # coast phase on the engine alone: ants lifted 3 m up and frozen far from the box, the box given a known slide
        roots = ora.tensor("root_states").reshape(n, A + 1, 13).copy()
        roots[:, :A, 1] += 6.0
        roots[:, :A, 2] = 3.0
        roots[:, :A, 7:13] = 0.0
        roots[:, A, 7:13] = 0.0
        roots[:, A, 3:7] = (0.0, 0.0, 0.0, 1.0)
        roots[:, A, 2] = 0.49918                                                                # resting on the compliant ground (half height 0.5)
        roots[:, A, 7] = 0.6                                                                    # m/s along x
        ora.tensor("root_states")[...] = roots.reshape(ora.tensor("root_states").shape)
        ora.tensor("reset")[...] = 0
        ora.tensor("progress")[...] = 1
        push_state(torch, eng, ora)
        vx = []
        for t in range(12):
            eng.tensor("actions").zero_()
            eng.tensor("reset").zero_()                           # (falling ants may flag a reset: keep the box where it slides)
            eng.step()
            torch.cuda.synchronize()
            vx.append(to_np(eng.tensor("root_states")).reshape(n, A + 1, 13)[:, A, 7].copy())
        coast[mu] = np.stack(vx)                                  # [steps, n]
        eng.close()
    dt = 0.0166
    decel = (0.6 - coast[0.5][2]) / (3 * dt)                      # over the first three steps, before it rests
    assert np.all(np.abs(decel - 0.5 * 9.81) < 0.6), decel        # Coulomb: mu g (the regularised law's normal-force estimate: +-10 %)
    assert np.all(np.abs(coast[0.5][-1]) < 0.03)                  # ... and at rest (creep below 3 cm/s) after 12 steps = 0.2 s > 0.6 / 4.9
    assert np.all(np.abs(coast[0.0][-1] - 0.6) < 1e-3)            # frictionless: keeps its speed
    parity.record("gpu/box_ground_friction/%s/physics" % task, push_phase_peak_speed_mu05=push_speed[0.5], push_phase_peak_speed_mu0=push_speed[0.0],
                  coast_decel_mu05=float(decel.mean()), coast_final_speed_mu05=float(np.abs(coast[0.5][-1]).max()),
                  coast_final_speed_mu0=float(coast[0.0][-1].mean()))


@pytest.mark.parametrize("task,n", [("TenAnt", 7), ("OneAnt", 5)])
def test_unpacked_launch_shapes(torch_cuda, task, n, monkeypatch):
    """MMS_PACKING=0 (one env per workgroup: the A/B switch of mms_create) runs the same lane code through the one-wave
    reductions (DPP / permute instead of LDS): parity with the oracle, ants pressed against the box included."""
    torch = torch_cuda
    monkeypatch.setenv("MMS_PACKING", "0")
    eng, ora = make_pair(task, num_envs=n, seed=21)
    tf = forced(eng, ora)
    rng = np.random.default_rng(8)
    for t in range(50):
        if t == 15:
            shove_ants_into_box(ora, rng)
        act = rng.uniform(-1, 1, (n, ora.num_actions)).astype(np.float32)
        drive(torch, eng, ora, tf, act, "%s unpacked step %d" % (task, t))
    tf.finish("gpu/unpacked/%s" % task)
    eng.close()


@pytest.mark.parametrize("n,dr", [(70, False), (16, False), (37, True)])
def test_sixteen_env_block_layout(torch_cuda, n, dr, monkeypatch):
    """MMS_STEP_BLOCK16=1: the <768,16> layout of the TenAnt step (16 envs per block, ten pure ant waves + two pure box waves; the
    default from 16 envs per CU up, i.e. at BASELINE's 4096 envs) on small grids with a partial last block: teacher-forced
    parity with the oracle, ants shoved against the box half way, resets included; once with physical randomisation on."""
    torch = torch_cuda
    monkeypatch.setenv("MMS_STEP_BLOCK16", "1")
    eng, ora = make_pair("TenAnt", num_envs=n, seed=13, total_envs=4096, env_offset=500)
    rng = np.random.default_rng(4)
    params = None
    if dr:
        params = random_dr_params(rng, n * ora.num_agents)
        ora.tensor("dr_params")[:] = params
        eng.tensor("dr_params").copy_(torch.from_numpy(params).to(eng.device))
        ora.set_dr(True)
        eng.set_dr(True)
    tf = forced(eng, ora, dr=params)
    for t in range(70):
        if t == 25:
            shove_ants_into_box(ora, rng)
        act = rng.uniform(-1.2, 1.2, (n, ora.num_actions)).astype(np.float32)
        drive(torch, eng, ora, tf, act, "TenAnt <768,16> step %d" % t)
    tf.finish("gpu/block16/n%d%s" % (n, "_dr" if dr else ""))
    eng.close()
    # and the two layouts against each other, free running from the same seed: bit-identical trajectories (same lane code,
    # same reduction orders)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("MMS_STEP_BLOCK16", flag)
        from massive_marl_benchmark_amd.engine import Engine
        e = Engine("TenAnt", num_envs=n, device=0, seed=2)
        g = torch.Generator().manual_seed(3)
        for t in range(40):
            e.tensor("actions").copy_((torch.rand(n, 80, generator=g) * 2 - 1).cuda())
            e.step()
        torch.cuda.synchronize()
        outs.append((e.tensor("root_states").clone(), e.tensor("obs").clone(), e.tensor("rew").clone(), e.tensor("reset").clone()))
        e.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("task,n,agents", [("TenAnt", 1, 10), ("OneAnt", 1, 1), ("MultiIngenuity", 1, 4), ("TenAnt", 9, 2),
                                            ("TenAnt", 5, 14), ("TenAnt", 3, 15), ("TenAnt", 2, 33)])
def test_edge_shapes_and_timeouts(torch_cuda, task, n, agents):
    """Single env, odd env counts, ant counts at the boundaries of the launch shapes (14 = the most one wave holds, 15 = the
    first 512-thread shape), and the episode time-out: progress >= episodeLength - 1 raises the reset flag (ten_ant.py:1298)."""
    torch = torch_cuda
    kw = task_kw(task, num_envs=n, seed=2)
    if task == "TenAnt":
        kw["num_agents"] = agents
    eng, ora = make_pair(task, **kw)
    tf = forced(eng, ora)
    rng = np.random.default_rng(6)
    limit = int(ora.config.max_episode_length)
    for t in range(24):
        if t == 10:                                           # jump to the end of the episode
            ora.tensor("progress")[...] = limit - 3
        act = rng.uniform(-1, 1, (n, ora.num_actions)).astype(np.float32)
        if task == "MultiIngenuity":
            act[:, 2::3] = np.abs(act[:, 2::3]) * 0.12
        drive(torch, eng, ora, tf, act, "%s A=%d step %d" % (task, agents, t))
        if t == 11:
            assert int(ora.tensor("reset").min()) == 1        # progress reached limit - 1: every env times out
        if t == 12:
            assert int(ora.tensor("progress").max()) == 0     # ... and is reset on the following step
    tf.finish("gpu/edge_shapes/%s/n%d_a%d" % (task, n, agents))
    eng.close()


def test_first_step_is_full_reset_and_noise_matches_oracle(torch_cuda):
    torch = torch_cuda
    eng, ora = make_pair("TenAnt", num_envs=32, seed=123, total_envs=64, env_offset=32)
    a = np.zeros((32, 80), np.float32)
    eng.tensor("actions").zero_()
    eng.step()
    ora.step(a)
    torch.cuda.synchronize()
    # reset state: integer hashing (bit-exact) then 0.4 u - 0.2, which the GPU contracts into one fma: 1 ulp
    np.testing.assert_allclose(to_np(eng.tensor("dof_state")), ora.tensor("dof_state"), rtol=0, atol=3e-8)
    np.testing.assert_array_equal(to_np(eng.tensor("root_states")), ora.tensor("root_states"))
    np.testing.assert_array_equal(to_np(eng.tensor("progress")), np.zeros(32, np.int64))
    d = to_np(eng.tensor("dof_state")).reshape(32, 10, 8, 2)
    assert np.all(d[:, 0] == d[:, 5])                                       # same noise for all ten ants (ten_ant.py:822-854)
    assert np.ptp(d[:, 0, 0, 0]) > 0.05                                     # but different per env
    eng.close()


def test_step_glue_fixture_from_reference(torch_cuda):
    """tests/golden/tenant_step_glue.npz (the reference's post_physics_step / reset_idx on supplied state) through
    mms_post_step on the GPU."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    g = load_golden("tenant_step_glue")
    S, n = g["actions"].shape[0], g["actions"].shape[1]
    eng = Engine("TenAnt", num_envs=n, device=0, clip_obs=5.0, external_noise=True)
    dev = eng.device
    for t in range(S):
        loc = g["sim_root"][t].reshape(n, 11, 13).copy()
        loc[:, :, 0:3] -= g["env_origin"][:, None, :]
        eng.set_state("root_states", loc.reshape(n * 11, 13).astype(np.float32))
        eng.set_state("dof_state", g["sim_dof"][t].astype(np.float32))
        eng.set_state("reset_noise", np.concatenate([g["noise_pos"][t], g["noise_vel"][t]], 1).astype(np.float32))
        np.testing.assert_array_equal(to_np(eng.tensor("reset")), g["reset_in"][t])
        if t == 2:
            eng.set_state("progress", np.array([998], np.int64), env_ids=[7])
        eng.tensor("actions").copy_(torch.from_numpy(g["actions"][t]).to(dev))
        eng.post_step()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(to_np(eng.tensor("reset")), g["reset"][t])
        np.testing.assert_array_equal(to_np(eng.tensor("progress")), g["progress"][t])
        obs, ref = to_np(eng.tensor("obs")), g["obs"][t]
        ang = np.zeros(388, bool)
        for k in range(10):
            ang[38 * k + 9:38 * k + 12] = True
        assert np.max(np.abs(obs[:, ~ang] - ref[:, ~ang])) < 2e-4, t           # global coords up to 240 m: ulp 1.5e-5
        assert angle_close(obs[:, ang], ref[:, ang], 0) < 2e-4, t
        np.testing.assert_array_equal(to_np(eng.tensor("obs_clipped")), np.clip(obs, -5, 5))
        assert np.max(np.abs(to_np(eng.tensor("rew")) - g["rew"][t])) < 0.4, t   # 500 x 20 x position rounding (see oracle test)
        prev = to_np(eng.tensor("prev"))
        assert np.max(np.abs(prev[:, :20] - g["pos_before"][t].reshape(n, 20))) < 2e-4
        assert np.max(np.abs(prev[:, 20:40] - g["goal_before"][t].reshape(n, 20))) < 2e-4
        assert np.max(np.abs(prev[:, 40:42] - g["box_before"][t])) < 2e-4
        ra = g["root_after"][t].reshape(n, 11, 13).copy()
        ra[:, :, 0:3] -= g["env_origin"][:, None, :]
        assert np.max(np.abs(to_np(eng.tensor("root_states")).reshape(n, 11, 13) - ra)) < 2e-5
        assert np.max(np.abs(to_np(eng.tensor("dof_state")) - g["dof_after"][t])) < 1e-6
    eng.close()


def test_obs_reward_fixtures_through_kernel(torch_cuda):
    """The tenant_reward golden vectors (reference compute_ant_reward) through the fused kernel (mms_post_step): the
    fixture rows are loaded as the states of env 0..N-1, with envSpacing 0 so that the global frame is the local one."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    from massive_marl_benchmark_amd.model import default_cfg
    g = load_golden("tenant_reward")
    n = g["obs"].shape[0]
    cfg = default_cfg("TenAnt")
    cfg["env"]["envSpacing"] = 0.0
    eng = Engine("TenAnt", cfg, num_envs=n, device=0, clip_obs=5.0)
    origin = to_np(eng.tensor("env_origin"))
    assert np.all(origin == 0)
    # rebuild the state that produces the fixture's observation: positions, velocities and joints are recoverable
    # from the obs only partially (local-frame velocities), so this test checks the REWARD path: it feeds the
    # fixture's caches and checks rew/reset for rows whose obs the kernel reproduces from a consistent state.
    obs = g["obs"]                                                               # [n,10,38]
    # consistent state: identity orientation, zero velocity, joints from the unscaled positions, positions from obs
    lower = np.array(eng.config.model.dof_lower[:], np.float32)
    upper = np.array(eng.config.model.dof_upper[:], np.float32)
    root = np.zeros((n, 11, 13), np.float32)
    root[:, :, 6] = 1.0
    root[:, :10, 0:3] = obs[:, :, 0:3] - origin[:, None, :]
    root[:, 10, 0:2] = g["box_pos"] - origin[:, :2]
    root[:, 10, 2] = 0.5
    root[:, 10, 3:7] = g["box_quat"]
    dof = np.zeros((n, 10, 8, 2), np.float32)
    dof[..., 0] = 0.5 * (obs[:, :, 14:22] * (upper - lower) + upper + lower)
    dof[..., 1] = obs[:, :, 22:30] / 0.2
    prev = np.concatenate([g["pos_before"].reshape(n, 20), g["goal_before"].reshape(n, 20), g["box_before"]], 1).astype(np.float32)
    eng.set_state("root_states", root.reshape(n * 11, 13))
    eng.set_state("dof_state", dof.reshape(n * 80, 2))
    eng.set_state("prev", prev)
    eng.set_state("reset", np.zeros(n, np.int64))
    eng.set_state("progress", (g["progress"] - 1).astype(np.int64))              # the kernel increments before the reward
    eng.tensor("actions").copy_(torch.from_numpy(g["actions"]).to(eng.device))
    eng.post_step()
    torch.cuda.synchronize()
    got = to_np(eng.tensor("obs")).reshape(n, 388)
    # goals / box part of the row, joints, actions: reproduced exactly from the consistent state
    for k in range(10):
        assert np.max(np.abs(got[:, 38 * k:38 * k + 3] - obs[:, k, 0:3])) < 1e-4
        assert np.max(np.abs(got[:, 38 * k + 14:38 * k + 22] - obs[:, k, 14:22])) < 1e-5
        assert np.max(np.abs(got[:, 38 * k + 22:38 * k + 30] - obs[:, k, 22:30])) < 1e-5
        np.testing.assert_array_equal(got[:, 38 * k + 30:38 * k + 38], np.clip(g["actions"][:, 8 * k:8 * k + 8], -1, 1))
    np.testing.assert_array_equal(got[:, 380:382], g["box_pos"])
    # reward: rows where the fixture's up_proj (obs[12]) does not cross 0.93 differ only in the up term -> add it back
    rew = to_np(eng.tensor("rew"))
    up_fix = 10.0 * 0.1 * (obs[:, :, 12] > 0.93).sum(1)
    up_got = 10.0 * 0.1 * 10                                                     # identity orientation: all upright
    fallen = (obs[:, :, 2] < 0.31).any(1)
    expect = np.where(fallen, -2.0, g["rew"] - up_fix + up_got)
    reset_in_zero = g["reset_in"] == 0
    # 20 terms of magnitude up to 3e3 summed in fp32: 20 x ulp(3e3) = 5e-3
    assert np.max(np.abs(rew - expect)) < 1e-2
    exp_reset = np.where(fallen | (g["progress"] >= 999), 1, 0)
    np.testing.assert_array_equal(to_np(eng.tensor("reset")), exp_reset)
    assert reset_in_zero.any()
    eng.close()


class GpuImpl:
    """tests/parity.py adapter: the HIP engine (through the C ABI) behind the put / get / post_step / step interface."""

    def __init__(self, torch, task, cfg=None, **kw):
        from massive_marl_benchmark_amd.engine import Engine
        self.torch = torch
        self.eng = Engine(task, cfg, device=0, **kw)
        self.config = self.eng.config

    def put(self, name, arr):
        t = self.eng.tensor(name)
        a = np.ascontiguousarray(np.asarray(arr).reshape(tuple(t.shape)), dtype=np.int64 if t.dtype == self.torch.int64 else np.float32)
        self.eng.set_state(name, a)

    def get(self, name):
        self.torch.cuda.synchronize()
        return to_np(self.eng.tensor(name)).copy()

    def _act(self, actions):
        self.eng.tensor("actions").copy_(self.torch.from_numpy(np.ascontiguousarray(actions, np.float32)).to(self.eng.device))

    def post_step(self, actions):
        self._act(actions)
        self.eng.post_step()
        self.torch.cuda.synchronize()

    def step(self, actions):
        self._act(actions)
        self.eng.step()
        self.torch.cuda.synchronize()

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("check", [parity.fixture_tenant_obs, parity.fixture_tenant_goals, parity.fixture_oneant, parity.fixture_ingenuity, parity.fixture_circle])
def test_reference_fixtures_through_kernels(torch_cuda, check):
    """The fixtures produced by the reference's own task functions -- tenant_obs (gimbal-lock rows included), tenant_goals,
    oneant_obs, oneant_reward, ingenuity_reward through mms_post_step, ingenuity_thrust through one physics substep of the
    helicopter kernel -- at the tolerances of the oracle's own golden tests (tests/test_oracle_golden.py).  helpers_kat has no
    kernel-level entry point: quat_rotate(_inverse), get_euler_xyz and normalize are exercised by the observation fixtures."""
    check(lambda task, cfg=None, **kw: GpuImpl(torch_cuda, task, cfg=cfg, **kw), load_golden, "gpu/")


def test_gae_kernels_golden(torch_cuda):
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.marl.utils.separated_buffer import SeparatedReplayBuffer
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
    from massive_marl_benchmark_amd import spaces
    dev = "cuda:0"
    g = load_golden("ppo_gae")
    T, N = g["rewards"].shape
    st = RolloutStorage(N, T, (388,), (0,), (80,), device=dev)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for t in range(T):
        st.add_transitions(torch.zeros(N, 388, device=dev), torch.zeros(N, 0, device=dev), torch.zeros(N, 80, device=dev),
                           cu(g["rewards"][t]), cu(g["dones"][t]), cu(g["values"][t]), cu(g["logp"][t]),
                           torch.zeros(N, 80, device=dev), torch.zeros(N, 80, device=dev))
    np.testing.assert_array_equal(to_np(st.rewards), g["stored_rewards"])
    np.testing.assert_array_equal(to_np(st.actions_log_prob), g["stored_logp"])
    st.compute_returns(cu(g["last_values"]), float(g["gamma"]), float(g["lam"]))
    torch.cuda.synchronize()
    assert np.max(np.abs(to_np(st.returns) - g["returns"])) < 1e-4
    assert np.max(np.abs(to_np(st.advantages) - g["advantages"])) < 1e-5
    ln, mr = st.get_statistics()
    assert abs(float(ln) - float(g["mean_traj_len"])) < 1e-5 and abs(float(mr) - float(g["mean_reward"])) < 1e-5

    g = load_golden("marl_gae")
    T, N = g["rewards"].shape[:2]

    class Norm:
        def __init__(self, mean, var):
            self.m, self.v = torch.tensor(mean, device=dev), torch.tensor(var, device=dev)

        def running_mean_var(self):
            return self.m, self.v

    for tag, popart, vn in (("popart", True, False), ("valuenorm", False, True), ("plain", False, False)):
        cfg = dict(episode_length=T, n_rollout_threads=N, hidden_size=64, recurrent_N=1, gamma=float(g["gamma"]),
                   gae_lambda=float(g["gae_lambda"]), use_gae=True, use_popart=popart, use_valuenorm=vn, use_proper_time_limits=False)
        buf = SeparatedReplayBuffer(cfg, spaces.Box(-np.inf, np.inf, (46,)), spaces.Box(-np.inf, np.inf, (388,)),
                                    spaces.Box(-np.ones(8), np.ones(8)), dev)
        for t in range(T):
            buf.insert(torch.zeros(N, 388, device=dev), torch.zeros(N, 46, device=dev), torch.zeros(N, 1, 64, device=dev),
                       torch.zeros(N, 1, 64, device=dev), torch.zeros(N, 8, device=dev), torch.zeros(N, 8, device=dev),
                       cu(g["values"][t]), cu(g["rewards"][t]), cu(g["masks_in"][t]))
        np.testing.assert_array_equal(to_np(buf.masks), g["masks_" + tag])
        norm = Norm(g["norm_mean_" + tag], g["norm_var_" + tag]) if (popart or vn) else None
        buf.compute_returns(cu(g["next_value"]), norm)
        torch.cuda.synchronize()
        assert np.max(np.abs(to_np(buf.returns)[:T] - g["returns_" + tag][:T])) < 1e-4, tag
        np.testing.assert_array_equal(to_np(buf.value_preds), g["value_preds_" + tag])


def test_vec_wrappers(torch_cuda):
    """VecTaskPython / MultiVecTaskPython return values against the reference wrapper fixture semantics."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.engine import current_stream_ptr
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.multi_vec_task import MultiVecTaskPython
    from massive_marl_benchmark_amd.tasks.agent_base.vec_task import VecTaskPython
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    # the slicing kernel against the fixture produced by the reference's MultiVecTaskPython.step
    g = load_golden("vec_wrappers")
    n = g["obs_buf"].shape[0]
    clipped = torch.from_numpy(np.clip(g["obs_buf"], -7, 7)).cuda()
    out = torch.empty(n, 10, 46, device="cuda")
    _lib.check(_lib.lib().mms_marl_views(0, ctypes.c_void_p(clipped.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, 10, 38, 8,
                                         current_stream_ptr(torch.device("cuda", 0))), None, "mms_marl_views")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(to_np(out), g["obs_all"])

    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = 32
    cfg["clip_observations"] = 7.0
    task = TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=True)
    env = MultiVecTaskPython(task, "cuda:0")
    assert env.num_agents == 10 and env.num_observations == 46 and env.nums_share_observations == 388
    assert env.observation_space[0].shape == (46,) and env.share_observation_space[0].shape == (388,) and env.action_space[0].shape == (8,)
    obs, state, _ = env.reset()
    assert obs.shape == (32, 10, 46) and state.shape == (32, 10, 388)
    acts = [torch.rand(32, 8, device="cuda") * 3 - 1.5 for _ in range(10)]
    obs_all, state_all, reward_all, done_all, info_all, _ = env.step(acts)
    torch.cuda.synchronize()
    raw = task.obs_buf
    np.testing.assert_array_equal(to_np(state_all[:, 3]), np.clip(to_np(raw), -7, 7))
    ref_obs = torch.cat([torch.clamp(raw[:, 38 * 4:38 * 5], -7, 7), torch.clamp(raw[:, 380:], -7, 7)], 1)
    np.testing.assert_array_equal(to_np(obs_all[:, 4]), to_np(ref_obs))
    assert reward_all.shape == (32, 10, 1) and done_all.shape == (32, 10)
    np.testing.assert_array_equal(to_np(reward_all[:, 7, 0]), to_np(task.rew_buf))
    np.testing.assert_array_equal(to_np(done_all[:, 2]), to_np(task.reset_buf))
    # actions reach the observation clamped to +-1 (multi_vec_task.py:101)
    np.testing.assert_array_equal(to_np(raw[:, 30:38]), np.clip(to_np(acts[0]), -1, 1))
    task.engine.close()

    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = 16
    task = TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=False)
    env = VecTaskPython(task, "cuda:0", 5.0, 1.0)
    assert env.num_obs == 388 and env.num_acts == 80 and env.observation_space.shape == (388,) and env.action_space.high[0] == 1.0
    o = env.reset()
    o2, r, d, info = env.step(torch.zeros(16, 80, device="cuda"))
    assert o.shape == (16, 388) and r.shape == (16,) and d.dtype == torch.int64 and info == {}
    assert float(o2.abs().max()) <= 5.0
    assert env.get_state().shape == (16, 0)
    # the engine reads the caller's action tensor in place (mms_bind_actions; vec_task.py:126-131 copies it): same trajectory as
    # copying into the engine's "actions" buffer, clamp to +-1 included; a non-contiguous / wrong-dtype tensor falls back to the copy
    task2 = TenAnt(dict(cfg, env=dict(cfg["env"])), None, "physx", "cuda", 0, True)
    env2 = VecTaskPython(task2, "cuda:0", 5.0, 1.0)
    ref_task = TenAnt(dict(cfg, env=dict(cfg["env"])), None, "physx", "cuda", 0, True)
    ref = ref_task.engine
    g = torch.Generator().manual_seed(4)
    for t in range(12):
        a = (torch.rand(16, 80, generator=g) * 3 - 1.5).cuda()
        if t == 5:
            a = a.double()                                        # falls back to the copy
        if t == 7:
            a = a.t().contiguous().t()                            # not contiguous: copy
        o2, r2, d2, _ = env2.step(a)
        assert task2.actions_read_in_place == (t not in (5, 7)) and task2.engine._bound_actions is None      # (the binding ends with the step)
        ref.tensor("actions").copy_(a.float())
        ref.step()
        torch.cuda.synchronize()
        assert torch.equal(o2, ref.tensor("obs_clipped")) and torch.equal(r2, ref.tensor("rew")) and torch.equal(d2, ref.tensor("reset"))
        assert torch.equal(task2.actions.float().reshape(16, 80), a.float())
    ref.close()
    task2.engine.close()
    task.engine.close()


def test_full_size_properties(torch_cuda):
    """BASELINE size (4096 envs): determinism, shard invariance, finiteness, resets, joint limits, box on the ground."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    N = 4096
    g = torch.Generator().manual_seed(1234)
    ring = [(torch.rand(N, 80, generator=g) * 2 - 1).cuda() for _ in range(8)]

    def run(offsets_sizes, steps):
        engs = [Engine("TenAnt", num_envs=sz, device=0, seed=3, env_offset=off, total_envs=N) for off, sz in offsets_sizes]
        for t in range(steps):
            for e, (off, sz) in zip(engs, offsets_sizes):
                e.tensor("actions").copy_(ring[t % 8][off:off + sz])
                e.step()
        torch.cuda.synchronize()
        out = {k: torch.cat([e.tensor(k) for e in engs]).clone() for k in ("obs", "rew", "reset", "progress", "root_states", "dof_state", "reset_count")}
        for e in engs:
            e.close()
        return out

    steps = 200
    a = run([(0, N)], steps)
    b = run([(0, N)], steps)
    c = run([(0, 1024), (1024, 1024), (2048, 2048)], steps)
    for k in a:
        assert torch.equal(a[k], b[k]), "not deterministic: " + k
        assert torch.equal(a[k], c[k]), "depends on sharding: " + k
    assert torch.isfinite(a["obs"]).all() and torch.isfinite(a["rew"]).all() and torch.isfinite(a["root_states"]).all()
    assert int(a["reset_count"].sum()) > N                                  # first-step reset + natural terminations
    assert int(a["reset_count"].max()) < 40
    r = a["root_states"].view(N, 11, 13)
    assert float(r[:, :10, 2].min()) > 0.0 and float(r[:, :10, 2].max()) < 2.5
    settled = a["progress"] > 40
    assert float((r[settled, 10, 2] - 0.5).abs().max()) < 0.03
    lo = torch.tensor([-0.698132, 0.523599, -0.698132, -1.745329, -0.698132, -1.745329, -0.698132, 0.523599], device="cuda")
    hi = torch.tensor([0.698132, 1.745329, 0.698132, -0.523599, 0.698132, -0.523599, 0.698132, 1.745329], device="cuda")
    q = a["dof_state"].view(N, 10, 8, 2)[..., 0]
    assert float((q - hi).max()) < 0.1 and float((lo - q).max()) < 0.1      # compliant limits: transient overshoot < 6 deg
    assert float(a["root_states"].view(N, 11, 13)[:, :, 3:7].norm(dim=-1).sub(1).abs().max()) < 1e-5


def test_multi_ant_circle_full_size_properties(torch_cuda):
    """MultiAntCircle (intended semantics: the reference cannot construct the task) at 8192 envs on the HIP kernel
    `ant_step_kernel<MMS_TASK_MULTI_ANT_CIRCLE, 64, 1, 0>`: bit-identical reruns, shard invariance, finiteness, resets by fall and by
    time, joint limits, the engine's far-away box untouched, and the ring reward only where the reference's GLOBAL-frame ring is."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    from massive_marl_benchmark_amd.model import default_cfg
    N = 8192
    g = torch.Generator().manual_seed(77)
    ring = [(torch.rand(N, 16, generator=g) * 2 - 1).cuda() for _ in range(8)]

    def run(shards, steps, spacing):
        cfg = default_cfg("MultiAntCircle")
        cfg["env"]["envSpacing"] = spacing
        engs = [Engine("MultiAntCircle", cfg=cfg, num_envs=sz, device=0, seed=3, env_offset=off, total_envs=N) for off, sz in shards]
        rews = []
        for t in range(steps):
            for e, (off, sz) in zip(engs, shards):
                e.bind_actions(ring[t % 8][off:off + sz].contiguous())
                e.step()
            rews.append(torch.cat([e.tensor("rew") for e in engs]).clone())
        torch.cuda.synchronize()
        out = {k: torch.cat([e.tensor(k) for e in engs]).clone() for k in ("obs", "rew", "reset", "progress", "root_states", "dof_state", "reset_count", "prev")}
        for e in engs:
            e.close()
        return out, torch.stack(rews)
    a, ra = run([(0, N)], 120, 0.0)
    b, _ = run([(0, N)], 120, 0.0)
    c, _ = run([(0, 2048), (2048, 2048), (4096, 4096)], 120, 0.0)
    for k in a:
        assert torch.equal(a[k], b[k]), "not deterministic: " + k
        assert torch.equal(a[k], c[k]), "depends on sharding: " + k
    assert torch.isfinite(a["obs"]).all() and torch.isfinite(ra).all()
    r = a["root_states"].view(N, 3, 13)
    assert float(r[:, :2, 2].min()) > 0.0 and float(r[:, :2, 2].max()) < 2.5
    assert float(r[:, 2, 1].min()) > 990.0 and float((r[:, 2, 2] - 0.5).abs().max()) < 0.01          # the inert box where it was put
    assert int(a["reset_count"].sum()) > N and float(ra.max()) > 1.5 and float(ra.min()) <= -2.0 + 1e-6
    assert torch.equal(a["prev"][:, 0:2], a["obs"][:, 0:2]) and torch.equal(a["prev"][:, 2:4], a["obs"][:, 38:40])
    # away from the global origin the ring is out of reach (the reward reads global positions, multi_ant_circle.py:424): no env of a
    # spaced grid but env 0 can earn the +2
    d, rd = run([(0, N)], 60, 10.0)
    assert float(rd[:, 1:].max()) < 1.0


def test_hundred_agent_swarm_parity(torch_cuda):
    """BASELINE config 5 shape (100 ants per env, 408 lanes = the 512-thread multi-wave variant of the step kernel with
    LDS reductions across waves), small N, teacher forced against the oracle.  The reference has no 100-agent task
    (SURVEY.md section 0 fact 8): the extrapolated scene is this build's own, parity is against the oracle only."""
    torch = torch_cuda
    n, steps = 6, 40
    kw = dict(num_envs=n, num_agents=100, seed=2)
    eng, ora = make_pair("TenAnt", **kw)
    assert eng.obs_dim == 3808 and eng.num_actions == 800
    tf = forced(eng, ora)
    rng = np.random.default_rng(3)
    for t in range(steps):
        act = rng.uniform(-1, 1, (n, 800)).astype(np.float32)
        drive(torch, eng, ora, tf, act, "swarm step %d" % t)
    tf.finish("gpu/swarm100/n%d" % n)
    eng.close()


def test_swarm_full_size_properties(torch_cuda):
    """BASELINE configs[4] at its per-GPU size: 100 ants per env, 16384 envs over 8 GPUs = 2048 envs on this one (the <512,1>
    multi-wave variant of the step kernel).  Determinism, shard invariance (2 x 1024 with matching env_offset = how two GPUs
    would hold them), finiteness, joint limits, box on the ground, resets."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    N, A, TOTAL = 2048, 100, 16384
    g = torch.Generator().manual_seed(99)
    ring = [(torch.rand(N, 8 * A, generator=g) * 2 - 1).cuda() for _ in range(4)]

    def run(parts, steps, offset0=4096):
        engs = [Engine("TenAnt", num_envs=sz, num_agents=A, device=0, seed=5, env_offset=offset0 + off, total_envs=TOTAL) for off, sz in parts]
        assert engs[0].obs_dim == 3808 and engs[0].num_actions == 800
        for t in range(steps):
            for e, (off, sz) in zip(engs, parts):
                e.tensor("actions").copy_(ring[t % 4][off:off + sz])
                e.step()
        torch.cuda.synchronize()
        out = {k: torch.cat([e.tensor(k) for e in engs]).clone() for k in ("obs", "rew", "reset", "progress", "root_states", "dof_state", "reset_count")}
        for e in engs:
            e.close()
        return out

    steps = 100
    a = run([(0, N)], steps)
    b = run([(0, N)], steps)
    c = run([(0, 1024), (1024, 1024)], steps)
    for k in a:
        assert torch.equal(a[k], b[k]), "not deterministic: " + k
        assert torch.equal(a[k], c[k]), "depends on sharding: " + k
    assert torch.isfinite(a["obs"]).all() and torch.isfinite(a["rew"]).all() and torch.isfinite(a["root_states"]).all()
    assert int(a["reset_count"].sum()) > N                                  # first-step reset + natural terminations
    r = a["root_states"].view(N, A + 1, 13)
    assert float(r[:, :A, 2].min()) > 0.0 and float(r[:, :A, 2].max()) < 2.5
    settled = a["progress"] > 40
    assert bool(settled.any()) and float((r[settled, A, 2] - 0.5).abs().max()) < 0.03     # the 280 m box rests on the ground
    lo = torch.tensor([-0.698132, 0.523599, -0.698132, -1.745329, -0.698132, -1.745329, -0.698132, 0.523599], device="cuda")
    hi = torch.tensor([0.698132, 1.745329, 0.698132, -0.523599, 0.698132, -0.523599, 0.698132, 1.745329], device="cuda")
    q = a["dof_state"].view(N, A, 8, 2)[..., 0]
    assert float((q - hi).max()) < 0.1 and float((lo - q).max()) < 0.1
    assert float(r[:, :, 3:7].norm(dim=-1).sub(1).abs().max()) < 1e-5
    parity.record("gpu/swarm100_full_size", envs=N, ants=A, steps=steps, resets=int(a["reset_count"].sum()),
                  max_speed=float(r[:, :, 7:10].abs().max()))


def test_mappo_datapath_full_size(torch_cuda):
    """BASELINE configs[3] on one GPU's shard: 4096 TenAnt envs through the MAPPO rollout data path -- MultiVecTaskPython +
    SharedRolloutBuffers (env step writing share_obs[t+1], mms_marl_views, one mms_gae_marl_agents launch for all ten agents)
    -- for two rollouts of 8 steps: the per-agent views hold what the wrapper returned, returns match a float64 GAE."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.marl.utils.shared_buffer import SharedRolloutBuffers
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.multi_vec_task import MultiVecTaskPython
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    n, T, A = 4096, 8, 10
    conf = dict(episode_length=T, n_rollout_threads=n, hidden_size=16, recurrent_N=1, gamma=0.99, gae_lambda=0.95, use_gae=True,
                use_popart=False, use_valuenorm=True, use_proper_time_limits=False)
    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = n
    cfg["clip_observations"] = 7.0
    cfg["seed"] = 4
    env = MultiVecTaskPython(TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=True), "cuda:0")
    sh = SharedRolloutBuffers(conf, env, "cuda:0")
    sh.warmup()

    class Norm:
        def __init__(self, k):
            self.m, self.v = torch.tensor([0.1 * k], device="cuda"), torch.tensor([1.0 + 0.2 * k], device="cuda")

        def running_mean_var(self):
            return self.m, self.v

    norms = [Norm(k) for k in range(A)]
    g = torch.Generator(device="cuda").manual_seed(1)
    for it in range(2):
        vals = []
        for t in range(T):
            acts = [torch.rand(n, 8, generator=g, device="cuda") * 2 - 1 for _ in range(A)]
            logp = [torch.randn(n, 8, generator=g, device="cuda") for _ in range(A)]
            v = torch.randn(n, A, generator=g, device="cuda")
            rew, dones = sh.env_step(acts)
            sh.insert_step(rew, dones, v, acts, logp)
            vals.append(v)
            torch.cuda.synchronize()
            assert torch.equal(sh.share_obs[t + 1], env.task.engine.tensor("obs_clipped")), (it, t)
            assert torch.equal(sh.agents[3].obs[t + 1][:, :38], sh.share_obs[t + 1][:, 38 * 3:38 * 4])
            assert torch.equal(sh.agents[3].obs[t + 1][:, 38:], sh.share_obs[t + 1][:, 380:])
        nxt = torch.randn(n, A, generator=g, device="cuda")
        sh.compute_returns(nxt, norms)
        torch.cuda.synchronize()
        # float64 GAE of agent 7 from the stored planes (separated_buffer.py:153-164 with ValueNorm denormalisation)
        k = 7
        vp = torch.cat([torch.stack(vals)[:, :, k], nxt[None, :, k]]).double() * float(norms[k].v.sqrt()) + float(norms[k].m)
        rw, mk = sh.agents[k].rewards[..., 0].double(), sh.agents[k].masks[..., 0].double()
        gae, want = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(T, n, dtype=torch.float64, device="cuda")
        for t in reversed(range(T)):
            delta = rw[t] + 0.99 * vp[t + 1] * mk[t + 1] - vp[t]
            gae = delta + 0.99 * 0.95 * mk[t + 1] * gae
            want[t] = gae + vp[t]
        err = float((sh.agents[k].returns[:T, :, 0].double() - want).abs().max() / want.abs().max().clamp(min=1.0))
        assert err < 1e-5, err
        assert bool(torch.isfinite(sh.share_obs).all())
        sh.after_update()
    parity.record("gpu/mappo_datapath_full_size", envs=n, agents=A, gae_rel_err=err)
    env.task.engine.close()


def test_ingenuity_full_size_properties(torch_cuda):
    """BASELINE config 3 size (MultiIngenuity, 8192 envs): determinism, shard invariance, finiteness, resets."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    N = 8192
    g = torch.Generator().manual_seed(7)
    ring = []
    for _ in range(8):
        a = torch.rand(N, 24, generator=g) * 2 - 1
        a[:, 2::3] = a[:, 2::3].abs() * 0.2
        ring.append(a.cuda())

    def run(parts, steps):
        engs = [Engine("MultiIngenuity", num_envs=sz, device=0, seed=1, env_offset=off, total_envs=N) for off, sz in parts]
        for t in range(steps):
            for e, (off, sz) in zip(engs, parts):
                e.tensor("actions").copy_(ring[t % 8][off:off + sz])
                e.step()
        torch.cuda.synchronize()
        out = {k: torch.cat([e.tensor(k) for e in engs]).clone() for k in ("obs", "rew", "reset", "progress", "root_states", "reset_count")}
        for e in engs:
            e.close()
        return out

    a = run([(0, N)], 150)
    b = run([(0, 4096), (4096, 4096)], 150)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["obs"]).all() and torch.isfinite(a["rew"]).all()
    assert int(a["reset_count"].sum()) > N and float(a["rew"].min()) >= 0.0
    assert float(a["root_states"][:, 10:13].norm(dim=-1).max()) <= 4 * np.pi + 1e-3      # max_angular_velocity (multi_ingenuity.py:149)


def test_ingenuity_in_flight_full_size_properties(torch_cuda):
    """BASELINE configs[2] with the helicopters actually FLYING: MultiIngenuity, 8192 envs, envSpacing 0 -- every env
    sits at the global origin, so the reference's global-frame reset rule (multi_ingenuity.py:381-453: any helicopter more than 8 m from
    its goal, or below 0.5 m) fires only when a helicopter really leaves, not on every step of every env away from the origin as under
    the default env grid.  Near-hover actions (thrust around weight / 2 per rotor, small lateral fractions): finite, speeds bounded,
    resets on fewer than 5 % of the env-steps, and the flight is not a standstill (the helicopters move)."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    from massive_marl_benchmark_amd.model import default_cfg
    N, steps = 8192, 200
    cfg = default_cfg("MultiIngenuity")
    cfg["env"]["envSpacing"] = 0.0
    eng = Engine("MultiIngenuity", cfg=cfg, num_envs=N, device=0, seed=2)
    hover = 1.5 * 3.721 / (2.0 * 2000.0 * eng.config.dt)             # per-rotor action whose thrust carries half the 1.5 kg on Mars
    g = torch.Generator().manual_seed(9)
    ring = []
    for _ in range(8):
        a = (torch.rand(N, 24, generator=g) * 2 - 1) * 0.1
        a[:, 2::3] = hover * (1.0 + 0.2 * (torch.rand(N, 8, generator=g) * 2 - 1))
        ring.append(a.cuda())
    eng.reset_all()
    eng.tensor("actions").copy_(ring[0])
    eng.step()                                                        # (whatever reset_all leaves pending has happened by now)
    torch.cuda.synchronize()
    base = int(eng.tensor("reset_count").sum())
    start = eng.tensor("root_states").clone()
    vmax, moved = 0.0, 0.0
    for t in range(steps):
        eng.tensor("actions").copy_(ring[t % 8])
        eng.step()
        if t % 20 == 19:
            rs = eng.tensor("root_states")
            assert torch.isfinite(rs).all() and torch.isfinite(eng.tensor("obs")).all() and torch.isfinite(eng.tensor("rew")).all()
            vmax = max(vmax, float(rs[:, 7:10].norm(dim=-1).max()))
            moved = max(moved, float((rs[:, 0:3] - start[:, 0:3]).norm(dim=-1).median()))
            assert float(rs[:, 10:13].norm(dim=-1).max()) <= 4 * np.pi + 1e-3
    torch.cuda.synchronize()
    resets = int(eng.tensor("reset_count").sum()) - base
    frac = resets / float(N * steps)
    assert vmax < 30.0, vmax
    assert moved > 0.01, moved
    assert 0 <= frac < 0.05, frac
    assert float(eng.tensor("rew").min()) >= 0.0
    parity.record("gpu/ingenuity_in_flight_8192", resets_per_env_step=frac, max_speed=vmax, median_displacement=moved)
    eng.close()


def test_shared_rollout_buffers_equal_separated_buffers(torch_cuda):
    """Rollout-buffer fusion: SharedRolloutBuffers driven through env_step / insert_step holds exactly
    what ten SeparatedReplayBuffers hold when driven the reference's way (runner.py:128-255), with share_obs stored once."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.marl.utils.separated_buffer import SeparatedReplayBuffer
    from massive_marl_benchmark_amd.algorithms.marl.utils.shared_buffer import SharedRolloutBuffers
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.multi_vec_task import MultiVecTaskPython
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    n, T, A = 64, 8, 10
    conf = dict(episode_length=T, n_rollout_threads=n, hidden_size=16, recurrent_N=1, gamma=0.99, gae_lambda=0.95, use_gae=True,
                use_popart=True, use_valuenorm=False, use_proper_time_limits=False)

    def make_env():
        cfg = default_cfg("TenAnt")
        cfg["env"]["numEnvs"] = n
        cfg["clip_observations"] = 7.0
        cfg["seed"] = 3
        return MultiVecTaskPython(TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=True), "cuda:0")

    class Norm:
        def __init__(self, k):
            self.m, self.v = torch.tensor([0.3 * k], device="cuda"), torch.tensor([1.0 + 0.5 * k], device="cuda")

        def running_mean_var(self):
            return self.m, self.v

    norms = [Norm(k) for k in range(A)]
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = [[torch.rand(n, 8, generator=g, device="cuda") * 2 - 1 for _ in range(A)] for _ in range(2 * T + 1)]
    vals = [torch.randn(n, A, generator=g, device="cuda") for _ in range(2 * T + 1)]
    logp = [[torch.randn(n, 8, generator=g, device="cuda") for _ in range(A)] for _ in range(2 * T + 1)]

    # reference way: ten separated buffers, MultiVecTaskPython.step, Runner.insert
    env = make_env()
    bufs = [SeparatedReplayBuffer(conf, env.observation_space[k], env.share_observation_space[k], env.action_space[k], "cuda:0") for k in range(A)]
    obs, share, _ = env.reset()
    for k in range(A):
        bufs[k].share_obs[0].copy_(share[:, k]); bufs[k].obs[0].copy_(obs[:, k])
    for it in range(2):
        for t in range(T):
            i = it * T + t
            obs, share, rew, dones, _, _ = env.step(acts[i])
            dones_env = torch.all(dones != 0, dim=1)
            masks = torch.ones(n, A, 1, device="cuda")
            masks[dones_env] = 0
            for k in range(A):
                bufs[k].insert(share[:, k], obs[:, k], torch.zeros(n, 1, 16, device="cuda"), torch.zeros(n, 1, 16, device="cuda"), acts[i][k],
                               logp[i][k], vals[i][:, k:k + 1], rew[:, k], masks[:, k])
        for k in range(A):
            bufs[k].compute_returns(vals[2 * T][:, k:k + 1], norms[k])
        if it == 0:
            for k in range(A):
                bufs[k].after_update()
    torch.cuda.synchronize()
    env.task.engine.close()

    # fused way
    env = make_env()
    sh = SharedRolloutBuffers(conf, env, "cuda:0")
    sh.warmup()
    for it in range(2):
        for t in range(T):
            i = it * T + t
            rew, dones = sh.env_step(acts[i])
            sh.insert_step(rew, dones, vals[i], acts[i], logp[i])
        sh.compute_returns(vals[2 * T], norms)
        if it == 0:
            sh.after_update()
    torch.cuda.synchronize()
    assert sh.share_obs.numel() * A == sum(b.share_obs.numel() for b in bufs)            # stored once instead of A times
    for k in range(A):
        v = sh.agents[k]
        assert torch.equal(v.share_obs, bufs[k].share_obs), k
        assert torch.equal(v.obs, bufs[k].obs), k
        assert torch.equal(v.rewards, bufs[k].rewards) and torch.equal(v.masks, bufs[k].masks), k
        assert torch.equal(v.actions, bufs[k].actions) and torch.equal(v.action_log_probs, bufs[k].action_log_probs), k
        assert torch.equal(v.value_preds, bufs[k].value_preds), k
        assert torch.allclose(v.returns[:T], bufs[k].returns[:T], atol=1e-5, rtol=1e-6), k
    # per-agent facade keeps the reference API: insert through the views gives the same buffers
    run = torch.zeros(n, device="cuda")
    tot, cnt = sh.finished_episode_rewards(run, torch.ones(n, device="cuda"), torch.tensor([1] + [0] * (n - 1), device="cuda"))
    assert float(tot) == 1.0 and int(cnt) == 1 and float(run[0]) == 0.0 and float(run[1]) == 1.0
    env.task.engine.close()


def test_domain_randomisation_noise(torch_cuda):
    """Observation / action noise lambdas (base_task.py:246-316): additive gaussian with the YAML's ranges, linear schedule."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = 256
    cfg["task"]["randomize"] = True
    cfg["task"]["randomization_params"]["observations"]["range"] = [0.0, 0.05]
    cfg["task"]["randomization_params"]["actions"]["range"] = [0.0, 0.02]
    task = TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=False)
    assert set(task.dr_randomizations) == {"observations", "actions"}
    a = torch.zeros(256, 80, device="cuda")
    task.step(a)
    torch.cuda.synchronize()
    noise = task.obs_buf - task._engine_obs
    assert abs(float(noise.std()) - 0.05) < 0.004 and abs(float(noise.mean())) < 0.002
    assert torch.equal(task.obs_buf_clipped, torch.clamp(task.obs_buf, -5, 5))
    seen = task._engine_obs[:, 30:38]                   # the actions the engine received = 0 + N(0, 0.02), clamped to +-1
    assert 0.015 < float(seen.std()) < 0.025
    task.engine.close()
    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = 16
    t2 = TenAnt(cfg, None, "physx", "cuda", 0, True)
    assert t2.dr_randomizations == {}                   # cfg/TenAnt.yaml ships randomize: False
    t2.step(torch.zeros(16, 80, device="cuda"))
    assert t2.obs_buf.data_ptr() == t2._engine_obs.data_ptr()
    t2.engine.close()


def test_actor_params_randomisation(torch_cuda):
    """actor_params of cfg/TenAnt.yaml:97-122 through BaseTask.apply_randomizations (base_task.py:343-395): ranges, setup_only,
    the frequency / reset gate, and that the engine is switched to the randomised kernel."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.one_ant import OneAnt
    from massive_marl_benchmark_amd.tasks.ten_ant import TenAnt
    np.random.seed(3)
    cfg = default_cfg("TenAnt")
    cfg["env"]["numEnvs"] = 128
    cfg["task"]["randomize"] = True
    cfg["task"]["randomization_params"]["frequency"] = 5
    task = TenAnt(cfg, None, "physx", "cuda", 0, True, is_multi_agent=False)
    dr = task.engine.tensor("dr_params").view(128, 10, 33).clone()
    mass, damp, lims = dr[..., 0:9], dr[..., 9:17], dr[..., 17:33]
    assert 0.5 <= float(mass.min()) < 0.6 and 1.4 < float(mass.max()) <= 1.5
    assert 0.5 <= float(damp.min()) < 0.6 and 1.4 < float(damp.max()) <= 1.5
    assert abs(float(lims.std()) - 0.01) < 0.001 and abs(float(lims.mean())) < 0.001
    assert float((dr[:, 0] - dr[:, 1]).abs().max()) > 0.1            # every ant its own draw
    a = torch.zeros(128, 80, device="cuda")
    for _ in range(8):                                                  # first step resets everything: frequency not reached yet
        task.step(a)
    torch.cuda.synchronize()
    assert torch.equal(task.engine.tensor("dr_params").view(128, 10, 33), dr)
    task.reset_buf[:64] = 1                                             # 64 envs reset after >= 5 steps: they are redrawn ...
    task.step(a)
    torch.cuda.synchronize()
    new = task.engine.tensor("dr_params").view(128, 10, 33)
    assert torch.equal(new[64:], dr[64:])
    assert float((new[:64, :, 9:] - dr[:64, :, 9:]).abs().min(dim=-1).values.max()) > 0    # damping and limits: new draws
    assert torch.equal(new[:64, :, 0:9], dr[:64, :, 0:9])               # ... except the mass: setup_only
    assert bool(torch.isfinite(task.obs_buf).all())
    task.engine.close()
    cfg = default_cfg("OneAnt")
    cfg["env"]["numEnvs"] = 32
    cfg["task"]["randomize"] = True
    cfg["task"]["randomization_params"]["actor_params"]["ant"]["rigid_shape_properties"] = {"friction": {"range": [0.7, 1.3], "operation": "scaling", "distribution": "uniform"}}
    with pytest.raises(NotImplementedError):
        OneAnt(cfg, None, "physx", "cuda", 0, True)


def test_bound_obs_out_and_graph_replay(torch_cuda):
    """Zero-copy rollout slot and hipGraph capture of the step: replay == eager."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    n = 256
    acts = [(torch.rand(n, 80) * 2 - 1).cuda() for _ in range(4)]
    e1 = Engine("TenAnt", num_envs=n, device=0, seed=9)
    e2 = Engine("TenAnt", num_envs=n, device=0, seed=9)
    slot = torch.zeros(n, 388, device="cuda")
    e2.bind_obs_out(slot)
    for e in (e1, e2):
        for t in range(20):
            e.tensor("actions").copy_(acts[t % 4])
            e.step()
    torch.cuda.synchronize()
    assert torch.equal(slot, e2.tensor("obs_clipped"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for t in range(4):
                e2.tensor("actions").copy_(acts[t])
                e2.step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(5):
        graph.replay()
    # capture does not execute; 5 replays = 20 more steps on e2, the same 20 steps eagerly on e1
    for t in range(20):
        e1.tensor("actions").copy_(acts[t % 4])
        e1.step()
    torch.cuda.synchronize()
    assert torch.equal(e1.tensor("root_states"), e2.tensor("root_states"))
    assert torch.equal(e1.tensor("obs"), e2.tensor("obs"))
    e1.close()
    e2.close()


def test_ppo_act_kernel_vs_oracle(torch_cuda):
    """mms_ppo_act (sampling tail of ActorCritic.act + the add_transitions stores) against the oracle's restatement with
    the same seed / counters: noise stream bit-compatible up to libm rounding, every destination written, counters
    advanced, and a captured graph draws fresh noise on every replay."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    from oracle.oracle import fp, ip, lib as olib_
    olib = olib_()
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for (N, A, ref) in ((1001, 80, 1), (1001, 80, 0), (130, 8, 1), (64, 128, 0)):
        mean = rng.standard_normal((N, A)).astype(np.float32)
        value = rng.standard_normal(N).astype(np.float32)
        ls = np.linspace(-0.6, 0.15, A).astype(np.float32)
        c0 = (np.arange(N) % 5).astype(np.int64)
        d = {k: torch.zeros(N, A, device="cuda") for k in ("actions_out", "act", "mu", "sigma")}
        logp, val = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        counters = torch.from_numpy(c0).cuda()
        tm, tv, tl = torch.from_numpy(mean).cuda(), torch.from_numpy(value).cuda(), torch.from_numpy(ls).cuda()
        _lib.check(L.mms_ppo_act(0, p(tm), p(tv), p(tl), 1234, p(counters), 7000, ref, p(d["actions_out"]), p(d["act"]), p(logp),
                                 p(val), p(d["mu"]), p(d["sigma"]), N, A, stream), None, "mms_ppo_act")
        torch.cuda.synchronize()
        oc = c0.copy()
        oact, ologp, osig = np.zeros((N, A), np.float32), np.zeros(N, np.float32), np.zeros((N, A), np.float32)
        olib.mo_ppo_act(N, A, fp(mean), fp(ls), ctypes.c_uint64(1234), ip(oc), 7000, ref, fp(oact), fp(ologp), fp(osig))
        np.testing.assert_array_equal(to_np(counters), oc)
        assert np.max(np.abs(to_np(d["act"]) - oact)) < 2e-5, (N, A, ref)       # logf / cosf / expf: a few ulp of |noise| <= 6
        assert torch.equal(d["act"], d["actions_out"])
        assert np.max(np.abs(to_np(logp) - ologp)) < 2e-3 * (A / 80.0 + 1.0)
        np.testing.assert_array_equal(to_np(d["mu"]), mean)
        np.testing.assert_array_equal(to_np(d["sigma"]), osig)
        np.testing.assert_array_equal(to_np(val), value)
    # NULL destinations are skipped; graph replays advance the device-side counters -> fresh noise
    N, A = 256, 80
    tm, tl = torch.zeros(N, A, device="cuda"), torch.zeros(A, device="cuda")
    counters = torch.zeros(N, dtype=torch.int64, device="cuda")
    out = torch.zeros(N, A, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _lib.check(L.mms_ppo_act(0, p(tm), None, p(tl), 5, p(counters), 0, 0, p(out), None, None, None, None, None, N, A,
                                     ctypes.c_void_p(side.cuda_stream)), None, "mms_ppo_act")
    torch.cuda.current_stream().wait_stream(side)
    draws = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        draws.append(out.clone())
    assert int(counters.min()) == 3 and int(counters.max()) == 3
    assert float((draws[0] == draws[1]).float().mean()) < 0.01 and float((draws[1] == draws[2]).float().mean()) < 0.01
    z = torch.cat(draws).flatten()
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1.0) < 0.01


def test_ppo_heads_act_kernel(torch_cuda):
    """mms_ppo_heads_act without the value head: the actor's last Linear layer on the matrix cores (fp32 MFMA) + the sampling.
    The mean against a float64 product of the same operands, everything downstream of it against the oracle fed with the
    kernel's own mean.  (37, 512, 128): 8 column tiles at H = 512, the shape whose 8-wave form would need 73.7 KB of LDS.)"""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    from oracle.oracle import fp, ip, lib as olib_
    olib = olib_()
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(8)
    for (N, H, A) in ((4096, 512, 80), (1003, 64, 8), (37, 256, 128), (37, 512, 128), (16, 128, 1)):
        hid = rng.standard_normal((N, H)).astype(np.float32)
        W = (rng.standard_normal((A, H)) / np.sqrt(H)).astype(np.float32)
        b = rng.standard_normal(A).astype(np.float32)
        ls = np.linspace(-0.5, 0.1, A).astype(np.float32)
        value = rng.standard_normal(N).astype(np.float32)
        th, tw, tb, tl, tv = (torch.from_numpy(x).cuda() for x in (hid, W, b, ls, value))
        counters = torch.zeros(N, dtype=torch.int64, device="cuda")
        act, mu, sigma = (torch.zeros(N, A, device="cuda") for _ in range(3))
        logp, val = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        _lib.check(L.mms_ppo_heads_act(0, p(th), p(tw), p(tb), H, p(tv), None, None, None, 0, p(tl), 77, p(counters), 5, 1, None, p(act), p(logp),
                                       p(val), p(mu), p(sigma), N, A, stream), None, "mms_ppo_heads_act")
        torch.cuda.synchronize()
        ref = hid.astype(np.float64) @ W.astype(np.float64).T + b
        scale = np.abs(hid).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b)
        assert np.max(np.abs(to_np(mu) - ref) / scale) < 4e-7, (N, H, A)          # fp32 products and sums, K <= 512
        oc = np.zeros(N, np.int64)
        oact, ologp, osig = np.zeros((N, A), np.float32), np.zeros(N, np.float32), np.zeros((N, A), np.float32)
        kmu = np.ascontiguousarray(to_np(mu))
        olib.mo_ppo_act(N, A, fp(kmu), fp(ls), ctypes.c_uint64(77), ip(oc), 5, 1, fp(oact), fp(ologp), fp(osig))
        assert np.max(np.abs(to_np(act) - oact)) < 2e-5
        assert np.max(np.abs(to_np(logp) - ologp)) < 2e-3 * (A / 80.0 + 1.0)
        np.testing.assert_array_equal(to_np(val), value)
        np.testing.assert_array_equal(to_np(counters), oc)
    rc = L.mms_ppo_heads_act(0, p(th), p(tw), p(tb), 100, p(tv), None, None, None, 0, p(tl), 77, p(counters), 5, 1, None, p(act), p(logp), p(val), p(mu), p(sigma), N, A, stream)
    assert rc != 0 and "multiple of 64" in _lib.last_error(None)


def test_linear2_act_kernel(torch_cuda):
    """mms_linear2_act (hidden layer of both policy networks: fp32 MFMA GEMM + bias + ELU) against torch's Linear + ELU; ragged
    M / N / K (partial tiles, K not a multiple of the 32-wide slice), one or two problems, identity epilogue."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(5)
    # (the first three shapes take the software-pipelined fast path: M, N multiples of 128, K of 64; the rest the generic kernel)
    for (M, N, K, act, two) in ((4096, 512, 1024, 1, True), (256, 128, 64, 0, True), (128, 256, 192, 1, False),
                                 (4096, 1024, 388, 1, True), (300, 200, 36, 1, True), (1, 1, 4, 0, False), (129, 257, 1024, 0, True),
                                 (64, 512, 1028, 1, False)):
        x = [torch.randn(M, K, device="cuda") for _ in range(2)]
        w = [torch.randn(N, K, device="cuda") / K ** 0.5 for _ in range(2)]
        b = [torch.randn(N, device="cuda") for _ in range(2)]
        y = [torch.full((M, N), float("nan"), device="cuda") for _ in range(2)]
        rc = L.mms_linear2_act(0, M, N, K, p(x[0]), p(w[0]), p(b[0]), p(y[0]), p(x[1] if two else None), p(w[1] if two else None),
                               p(b[1] if two else None), p(y[1] if two else None), act, stream)
        assert rc == 0, _lib.last_error(None)
        torch.cuda.synchronize()
        for g in range(2 if two else 1):
            ref = torch.nn.functional.linear(x[g].double(), w[g].double(), b[g].double())
            if act:
                ref = torch.nn.functional.elu(ref)
            scale = x[g].abs().double() @ w[g].abs().double().t() + b[g].abs().double()
            assert float(((y[g].double() - ref).abs() / scale).max()) < 5e-7, (M, N, K, act, g)   # fp32 products and sums, K <= 1028
    assert L.mms_linear2_act(0, 8, 8, 6, p(x[0]), p(w[0]), p(b[0]), p(y[0]), None, None, None, None, 1, stream) != 0     # K % 4


def _p32_bytes(rows, K):
    return rows * ((K + 31) // 32) * 192


def _planes_to_f32(torch, planes, rows, K):
    """P32 planes (include/mms.h) -> [rows, K] float32: the three planes of an element sum to it exactly"""
    KC = (K + 31) // 32
    v = planes.view(torch.bfloat16).view(rows, KC, 3, 32).float()
    return ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]).reshape(rows, KC * 32)[:, :K], v


def test_split_planes_exact(torch_cuda):
    """mms_split_planes: every fp32 value is EXACTLY the sum of its three bf16 planes (so the split layers multiply the fp32 operands
    themselves, not roundings of them), columns past K are zero, row pitches other than K are honoured; extremes included."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(2)
    for (rows, K, pitch) in ((4096, 388, 388), (1024, 1024, 1024), (7, 36, 40), (3, 1, 4), (5, 1028, 1028), (130, 64, 64)):
        x = torch.randn(rows, pitch, device="cuda")
        x[0, :min(K, 8)] = torch.tensor([0.0, -0.0, 1e-30, -3e38, 1.0 + 2 ** -23, 2 ** -126, 65504.0, -1e-20], device="cuda")[:min(K, 8)]
        planes = torch.full((_p32_bytes(rows, K),), 0xAB, dtype=torch.uint8, device="cuda")
        _lib.check(L.mms_split_planes(0, rows, K, pitch, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(planes.data_ptr()), stream), None, "split")
        back, v = _planes_to_f32(torch, planes, rows, K)
        assert torch.equal(back, x[:, :K]), (rows, K, pitch)
        KC = (K + 31) // 32
        if KC * 32 > K:
            assert float(v.permute(0, 1, 3, 2).reshape(rows, KC * 32, 3)[:, K:].abs().max()) == 0.0
    x = torch.randn(8, 8, device="cuda")
    planes = torch.empty(_p32_bytes(8, 8), dtype=torch.uint8, device="cuda")
    assert L.mms_split_planes(0, 8, 8, 4, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(planes.data_ptr()), stream) != 0      # pitch < K
    assert L.mms_split_planes(0, 8, 8, 8, None, ctypes.c_void_p(planes.data_ptr()), stream) != 0


def test_split_layers_error(torch_cuda):
    """mms_linear_group_act_split (fp32 operands as three bf16 planes, six bf16 MFMA products, fp32 accumulation) against the float64
    product, NEXT TO the exact-fp32 MFMA kernel (mms_linear2_act) on the same inputs: the split kernel's error must not be larger --
    that is what makes it the same fp32 arithmetic on a faster pipe and not a narrower precision.  Gates: every element within the
    fp32 kernel's own per-element bound (5e-7 of sum |x||w| + |b|, test_linear2_act_kernel), rms error <= 0.5 x the fp32 kernel's
    rms error on every shape (measured 0.32 x: the leading accumulator rounds once per 32 k, the fp32 MFMA chain 32 times), worst
    error <= 0.8 x its worst error (measured 0.35-0.42 x), mean error not above the fp32 kernel's own.  Shapes: the PPO policy's three hidden
    layers at 4096 rows (both tilings: 256 x 128 and 128 x 128 blocks), one and two networks, all four epilogues, planes-out and
    fp32-out; the P32 output of one launch is the input of the next."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(5)
    acts = {0: lambda v: v, 1: torch.nn.functional.elu, 2: torch.relu, 3: torch.tanh}
    margins = {}
    for (M, N, K, act, G, planes_out) in ((4096, 1024, 388, 1, 2, 1), (4096, 1024, 1024, 1, 2, 1), (4096, 512, 1024, 1, 2, 0),
                                          (4096, 1024, 1024, 1, 1, 0), (128, 128, 32, 0, 1, 1), (256, 384, 100, 2, 2, 1),
                                          (384, 128, 1028, 3, 3, 0), (8192, 256, 256, 2, 1, 1)):
        x = [torch.randn(M, K, device="cuda") for _ in range(G)]
        x = [torch.where(t > 0, t, torch.expm1(t)).contiguous() for t in x]                      # ELU-shaped activations
        w = [torch.randn(N, K, device="cuda") / K ** 0.5 for _ in range(G)]
        b = [torch.randn(N, device="cuda") * 0.1 for _ in range(G)]
        xp = [torch.empty(_p32_bytes(M, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        wp = [torch.empty(_p32_bytes(N, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        for g in range(G):
            _lib.check(L.mms_split_planes(0, M, K, 0, p(x[g]), p(xp[g]), stream), None, "split x")
            _lib.check(L.mms_split_planes(0, N, K, 0, p(w[g]), p(wp[g]), stream), None, "split w")
        ys = [torch.full((_p32_bytes(M, N) if planes_out else M * N * 4,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(G)]
        rc = L.mms_linear_group_act_split(0, G, M, N, K, arr(xp), arr(wp), arr(b), arr(ys), act, planes_out, None, None, None, None, None, 0, stream)
        assert rc == 0, _lib.last_error(None)
        y32 = [torch.empty(M, N, device="cuda") for _ in range(G)]
        for g in range(G):
            assert L.mms_linear2_act(0, M, N, (K + 3) // 4 * 4, p(torch.nn.functional.pad(x[g], (0, (-K) % 4))), p(torch.nn.functional.pad(w[g], (0, (-K) % 4))),
                                     p(b[g]), p(y32[g]), None, None, None, None, act, stream) == 0
        torch.cuda.synchronize()
        e_split, e_f32 = [], []
        for g in range(G):
            out = _planes_to_f32(torch, ys[g], M, N)[0] if planes_out else ys[g].view(torch.float32).view(M, N)
            ref = acts[act](torch.nn.functional.linear(x[g].double(), w[g].double(), b[g].double()))
            scale = x[g].abs().double() @ w[g].abs().double().t() + b[g].abs().double()
            assert float(((out.double() - ref).abs() / scale).max()) < 5e-7, (M, N, K, act, g)
            assert float(((y32[g].double() - ref).abs() / scale).max()) < 5e-7, ("the yardstick itself", M, N, K, act, g)
            e_split.append(out.double() - ref)
            e_f32.append(y32[g].double() - ref)
        es, ef = torch.cat(e_split), torch.cat(e_f32)
        rms_ratio = float(es.pow(2).mean().sqrt() / ef.pow(2).mean().sqrt())
        max_ratio = float(es.abs().max() / ef.abs().max())
        margins["%dx%dx%d" % (M, N, K)] = {"rms_ratio": rms_ratio, "max_ratio": max_ratio}
        if K >= 100:                                                 # (tiny K: both errors are a few ulps of single roundings)
            assert rms_ratio <= 0.5 and max_ratio <= 0.8, (M, N, K, rms_ratio, max_ratio)
            # no bias of its own: the mean error stays at the exact-fp32 kernel's (both carry the epilogue's ~1e-9 rms(Y)), far below
            # the -5e-8 rms(Y) a single accumulator for all six products shows
            assert abs(float(es.mean())) <= max(2.0 * abs(float(ef.mean())), 0.02 * float(es.pow(2).mean().sqrt())), "biased"
        if planes_out and N % 128 == 0 and act == 1:                 # chained: this layer's planes feed the next split layer unchanged
            w2 = [torch.randn(128, N, device="cuda") / N ** 0.5 for _ in range(G)]
            w2p = [torch.empty(_p32_bytes(128, N), dtype=torch.uint8, device="cuda") for _ in range(G)]
            for g in range(G):
                _lib.check(L.mms_split_planes(0, 128, N, 0, p(w2[g]), p(w2p[g]), stream), None, "split w2")
            y2 = [torch.empty(M, 128, device="cuda") for _ in range(G)]
            b2 = [torch.zeros(128, device="cuda") for _ in range(G)]
            assert L.mms_linear_group_act_split(0, G, M, 128, N, arr(ys), arr(w2p), arr(b2), arr(y2), 0, 0, None, None, None, None, None, 0, stream) == 0
            torch.cuda.synchronize()
            for g in range(G):
                h = _planes_to_f32(torch, ys[g], M, N)[0]
                ref2 = h.double() @ w2[g].double().t()
                assert float((y2[g].double() - ref2).abs().max() / ref2.abs().max()) < 2e-6
    parity.record("gpu/split_layers_vs_fp32_mfma", **margins)
    # argument checks: M, N multiples of 128; groups in range; null pointers
    z = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    zb = torch.zeros(256, device="cuda")
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    assert L.mms_linear_group_act_split(0, 1, 100, 128, 32, one(z), one(z), one(zb), one(z), 1, 0, None, None, None, None, None, 0, stream) != 0
    assert L.mms_linear_group_act_split(0, 1, 128, 100, 32, one(z), one(z), one(zb), one(z), 1, 0, None, None, None, None, None, 0, stream) != 0
    assert L.mms_linear_group_act_split(0, 0, 128, 128, 32, one(z), one(z), one(zb), one(z), 1, 0, None, None, None, None, None, 0, stream) != 0
    assert L.mms_linear_group_act_split(0, 1, 128, 128, 32, one(z), (ctypes.c_void_p * 1)(None), one(zb), one(z), 1, 0, None, None, None, None, None, 0, stream) != 0
    assert "null pointer" in _lib.last_error(None)


def _h32_bytes(rows, K):
    return rows * ((K + 31) // 32) * 128


def _h32_to_f64(torch, planes, rows, K, inv):
    v = planes.view(torch.float16).view(rows, (K + 31) // 32, 2, 32).double()
    return ((v[:, :, 0] + v[:, :, 1] / 2048.0).reshape(rows, -1) * inv.double()[:, None])[:, :K], v


def test_split16_planes(torch_cuda):
    """mms_split_planes16_group: two fp16 planes under a power-of-two scale per row.  Every element is kept to 2^-22 of itself (or, far
    below its row's largest magnitude, to 2^-35 of that magnitude: subnormal halves), the scale puts the row's largest magnitude in
    [2^13, 2^14], columns past K are zero, row pitches are honoured, and the planes equal the CPU build's value for value (the same
    round-to-nearest-even conversions); the bound chain's scales are the ones the formula gives."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L, C = _lib.lib(), _lib.lib_cpu()
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(2)
    for (rows, K, pitch) in ((4096, 388, 388), (1024, 1024, 1024), (7, 36, 40), (3, 1, 4), (5, 1028, 1028), (130, 64, 64), (9, 2500, 2500), (4096, 46, 460), (33, 46, 47),
                             (100, 100, 100), (13, 200, 203)):
        x = torch.randn(rows, pitch, device="cuda") * torch.exp2(torch.randint(-24, 16, (rows, 1), device="cuda").float())
        if K >= 8:
            x[0, :8] = torch.tensor([0.0, -0.0, 1e-30, -3e4, 1.0 + 2 ** -23, 2 ** -20, 65504.0, -1e-20], device="cuda")
        if rows > 2:
            x[2] = 0.0
        planes = torch.full((_h32_bytes(rows, K),), 0xAB, dtype=torch.uint8, device="cuda")
        sc, iv = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        st = torch.full((rows, 2), float("nan"), device="cuda")
        _lib.check(L.mms_split_planes16_group(0, 1, rows, K, pitch, arr([x]), arr([planes]), arr([sc]), arr([iv]), 0, 0, None, None, None, arr([st]), 1e-5, stream), None, "split16")
        torch.cuda.synchronize()
        # the LayerNorm statistics of the rows ride along (two-pass form), whatever the rows' magnitude
        xd = x[:, :K].double()
        mean64, var64 = xd.mean(1), xd.var(1, unbiased=False)
        assert float(((st[:, 0].double() - mean64).abs() / (xd.abs().max(1).values + 1e-30)).max()) < 1e-6, (rows, K)
        assert float((st[:, 1].double() * (var64 + 1e-5).sqrt() - 1.0).abs().max()) < 1e-5, (rows, K)
        back, v = _h32_to_f64(torch, planes, rows, K, iv)
        ref = x[:, :K].double()
        big = ref.abs().max(1, keepdim=True).values
        assert float(((back - ref).abs() - 2.0 ** -21 * ref.abs() - 2.0 ** -35 * big).max()) <= 0.0, (rows, K)
        top = (big[:, 0] * sc.double())
        assert bool(((top <= 2.0 ** 14) & ((top > 2.0 ** 13) | (big[:, 0] == 0))).all()) and torch.equal(sc * iv, torch.ones_like(sc))
        KC = (K + 31) // 32
        if KC * 32 > K:
            assert float(v.permute(0, 1, 3, 2).reshape(rows, KC * 32, 2)[:, K:].abs().max()) == 0.0
        xc = x.cpu()
        pc, scc, ivc = torch.empty(_h32_bytes(rows, K), dtype=torch.uint8), torch.empty(rows), torch.empty(rows)
        assert C.mms_split_planes16_group(-1, 1, rows, K, pitch, arr([xc]), arr([pc]), arr([scc]), arr([ivc]), 0, 0, None, None, None, None, 0.0, None) == 0
        # (as values: the device build's no-signed-zeros arithmetic leaves -0 where the host has +0 in the lo plane of a -0 input)
        assert torch.equal(planes.cpu().view(torch.float16), pc.view(torch.float16)) and torch.equal(sc.cpu(), scc), (rows, K)
    # chains: bound_{l+1} = (mult_l bound_l + add_l) 1.001, scale = 2^(14 - e) with bound <= 2^e
    rows, K = 300, 64
    x = torch.randn(rows, K, device="cuda") * torch.exp2(torch.randint(-10, 10, (rows, 1), device="cuda").float())
    chain = torch.tensor([[[20.0, 0.5], [30.0, 0.1], [0.0, 7.0]], [[1e-3, 0.0], [5.0, 5.0], [2.0, 0.0]]], device="cuda")
    planes, sc, iv = torch.empty(_h32_bytes(rows, K), dtype=torch.uint8, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    cs, ci = torch.empty(2, 3, rows, device="cuda"), torch.empty(2, 3, rows, device="cuda")
    _lib.check(L.mms_split_planes16_group(0, 1, rows, K, 0, arr([x]), arr([planes]), arr([sc]), arr([iv]), 2, 3, arr([chain]), arr([cs]), arr([ci]), None, 0.0, stream), None, "split16 chain")
    torch.cuda.synchronize()
    bound = x.abs().max(1).values
    for c in range(2):
        bd = bound.clone()
        for l in range(3):
            bd = (chain[c, l, 0] * bd + chain[c, l, 1]) * 1.001
            e = torch.frexp(bd)[1].float()
            assert torch.equal(cs[c, l], torch.exp2(14 - e)) and torch.equal(cs[c, l] * ci[c, l], torch.ones(rows, device="cuda"))
    assert L.mms_split_planes16_group(0, 1, rows, K, 0, arr([x]), arr([planes]), arr([sc]), arr([iv]), 2, 3, None, arr([cs]), arr([ci]), None, 0.0, stream) != 0
    assert "chain" in _lib.last_error(None)


def test_split16_layers_error(torch_cuda):
    """mms_linear_group_act_split16 (fp32 operands as two scaled fp16 planes, three f16 MFMA products, fp32 accumulation) against the
    float64 product, NEXT TO the exact-fp32 MFMA kernel (mms_linear2_act) on the same inputs, as test_split_layers_error does for the
    three-plane kernel.  Gates: every element within the fp32 kernel's own per-element bound (5e-7 of sum |x||w| + |b|), rms error <=
    0.6 x the fp32 kernel's (measured 0.38-0.45 x), worst error <= 0.8 x (measured 0.3-0.45 x), no mean error of its own.  The hidden
    activations' scales come from the bound chain; a row with a huge input and one with a tiny input ride along (their scales differ
    by 2^40)."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(5)
    acts = {0: lambda v: v, 1: torch.nn.functional.elu, 2: torch.relu, 3: torch.tanh}
    margins = {}
    f32 = lambda *sh: torch.empty(*sh, device="cuda")
    for (M, N, K, act, G, planes_out, wscale) in ((4096, 1024, 388, 1, 2, 1, 1.0), (4096, 1024, 1024, 1, 2, 1, 1.0), (4096, 512, 1024, 1, 2, 0, 1.0),
                                                  (4096, 1024, 1024, 1, 1, 0, 1.0), (128, 128, 32, 0, 1, 1, 1.0), (256, 384, 100, 2, 2, 1, 1.0),
                                                  (384, 128, 1028, 3, 3, 0, 1.0), (8192, 256, 256, 2, 1, 1, 1.0), (2560, 512, 64, 1, 20, 1, 1.0),
                                                  (2560, 512, 32, 1, 32, 1, 1.0), (2560, 512, 96, 1, 32, 0, 1.0),     # one / three k-steps, five tiles per CU (the rolling loop's short ends)
                                                  (512, 256, 512, 2, 2, 1, 1e4), (512, 256, 512, 0, 2, 1, 1e-5)):    # weights (and the bound chain) far from 1
        x = [torch.randn(M, K, device="cuda") for _ in range(G)]
        x = [torch.where(t > 0, t, torch.expm1(t)).contiguous() for t in x]                      # ELU-shaped activations
        for t in x:
            t[1] *= 1e6
            t[2] *= 1e-6
        w = [torch.randn(N, K, device="cuda") / K ** 0.5 * wscale for _ in range(G)]
        b = [torch.randn(N, device="cuda") * 0.1 * wscale for _ in range(G)]
        xp = [torch.empty(_h32_bytes(M, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        wp = [torch.empty(_h32_bytes(N, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        xs, xi, ws, wi = [[f32(n) for _ in range(G)] for n in (M, M, N, N)]
        chain = [torch.stack([w[g].abs().sum(1).max(), b[g].abs().max()]).view(1, 1, 2).contiguous() for g in range(G)]
        cs, ci = [f32(1, 1, M) for _ in range(G)], [f32(1, 1, M) for _ in range(G)]
        _lib.check(L.mms_split_planes16_group(0, G, M, K, 0, arr(x), arr(xp), arr(xs), arr(xi), 1, 1, arr(chain), arr(cs), arr(ci), None, 0.0, stream), None, "split16 x")
        _lib.check(L.mms_split_planes16_group(0, G, N, K, 0, arr(w), arr(wp), arr(ws), arr(wi), 0, 0, None, None, None, None, 0.0, stream), None, "split16 w")
        ys = [torch.full((_h32_bytes(M, N) if planes_out else M * N * 4,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(G)]
        rc = L.mms_linear_group_act_split16(0, G, M, N, K, arr(xp), arr(wp), arr(b), arr(ys), arr(xi), arr(wi), arr([c[0, 0] for c in cs]) if planes_out else None,
                                            act, planes_out, None, None, None, None, None, 0, stream)
        assert rc == 0, _lib.last_error(None)
        y32 = [torch.empty(M, N, device="cuda") for _ in range(G)]
        for g in range(G):
            assert L.mms_linear2_act(0, M, N, (K + 3) // 4 * 4, p(torch.nn.functional.pad(x[g], (0, (-K) % 4))), p(torch.nn.functional.pad(w[g], (0, (-K) % 4))),
                                     p(b[g]), p(y32[g]), None, None, None, None, act, stream) == 0
        torch.cuda.synchronize()
        e_split, e_f32, e_torch = [], [], []
        for g in range(G):
            if planes_out:
                out, v = _h32_to_f64(torch, ys[g], M, N, ci[g][0, 0])
                assert float(v[:, :, 0].abs().max()) <= 2.0 ** 14, "a hidden activation left the bound"
            else:
                out = ys[g].view(torch.float32).view(M, N).double()
            ref = acts[act](torch.nn.functional.linear(x[g].double(), w[g].double(), b[g].double()))
            scale = x[g].abs().double() @ w[g].abs().double().t() + b[g].abs().double()
            # (+ 1.2e-7: ELU is evaluated as expf(v) - 1 in both kernels, half an ulp of 1 whatever |v| -- visible only in the tiny row)
            assert float(((out - ref).abs() - 5e-7 * scale).max()) < 1.2e-7 * max(1.0, wscale), (M, N, K, act, g)
            assert float(((y32[g].double() - ref).abs() - 5e-7 * scale).max()) < 1.2e-7 * max(1.0, wscale), ("the yardstick itself", M, N, K, act, g)
            keep = torch.ones(M, dtype=torch.bool, device="cuda")
            keep[1] = keep[2] = False                               # (the two rescaled rows would dominate / vanish in an rms over all rows)
            e_split.append((out - ref)[keep])
            e_f32.append((y32[g].double() - ref)[keep])
            # the reference's own arithmetic on this box: torch's fp32 F.linear (the library's fp32 GEMM) + the activation in fp32
            e_torch.append((acts[act](torch.nn.functional.linear(x[g], w[g], b[g])).double() - ref)[keep])
        es, ef, et = torch.cat(e_split), torch.cat(e_f32), torch.cat(e_torch)
        rms_ratio = float(es.pow(2).mean().sqrt() / ef.pow(2).mean().sqrt())
        max_ratio = float(es.abs().max() / ef.abs().max())
        rms_vs_torch = float(es.pow(2).mean().sqrt() / et.pow(2).mean().sqrt())
        max_vs_torch = float(es.abs().max() / et.abs().max())
        margins["%dx%dx%dx%d%s" % (G, M, N, K, "" if wscale == 1.0 else "_w%g" % wscale)] = {
            "rms_ratio": rms_ratio, "max_ratio": max_ratio, "mean_over_rms": float(es.mean() / es.pow(2).mean().sqrt()),
            "rms_ratio_vs_torch_fp32": rms_vs_torch, "max_ratio_vs_torch_fp32": max_vs_torch}
        # against torch's fp32 F.linear, the arithmetic the reference runs -- not only against this build's own fp32 kernel
        if K >= 256:
            assert rms_vs_torch <= 1.0 and max_vs_torch <= 1.0, (M, N, K, rms_vs_torch, max_vs_torch)
        # The fp32 chain's error grows with the number of its roundings (~ sqrt(K)), this kernel's floor is the operands' 22-23 bits
        # (4e-8 rms each): 0.38 x at K = 1024, 0.45 x at K = 388, 0.65 x at K = 100, and about equal below K = 64, where both are a
        # few ulps of single roundings.
        if K >= 100:
            assert (rms_ratio <= 0.6 and max_ratio <= 0.8) if K >= 256 else (rms_ratio <= 0.9 and max_ratio <= 1.0), (M, N, K, rms_ratio, max_ratio)
            # mean error: a few 1e-9 of rms(Y) at most (measured <= 0.01 of the rms error at K >= 388, 0.03 at K = 100 where the rms
            # error itself is 6e-8) -- the -5e-8 rms(Y) of a single accumulator for all products is what this gate is for
            assert abs(float(es.mean())) <= max(2.0 * abs(float(ef.mean())), (0.02 if K >= 256 else 0.05) * float(es.pow(2).mean().sqrt())), "biased"
        else:
            assert rms_ratio <= 1.5, (M, N, K, rms_ratio, max_ratio)
        if planes_out and N % 128 == 0 and act == 1:                 # chained: this layer's planes feed the next split layer unchanged
            w2 = [torch.randn(128, N, device="cuda") / N ** 0.5 for _ in range(G)]
            w2p = [torch.empty(_h32_bytes(128, N), dtype=torch.uint8, device="cuda") for _ in range(G)]
            w2s, w2i = [f32(128) for _ in range(G)], [f32(128) for _ in range(G)]
            _lib.check(L.mms_split_planes16_group(0, G, 128, N, 0, arr(w2), arr(w2p), arr(w2s), arr(w2i), 0, 0, None, None, None, None, 0.0, stream), None, "split16 w2")
            y2 = [torch.empty(M, 128, device="cuda") for _ in range(G)]
            b2 = [torch.zeros(128, device="cuda") for _ in range(G)]
            assert L.mms_linear_group_act_split16(0, G, M, 128, N, arr(ys), arr(w2p), arr(b2), arr(y2), arr([c[0, 0] for c in ci]), arr(w2i), None, 0, 0,
                                                  None, None, None, None, None, 0, stream) == 0
            torch.cuda.synchronize()
            for g in range(G):
                h = _h32_to_f64(torch, ys[g], M, N, ci[g][0, 0])[0]
                ref2 = h @ w2[g].double().t()
                assert float(((y2[g].double() - ref2).abs() / ref2.abs().max(1, keepdim=True).values).max()) < 2e-6
    parity.record("gpu/split16_layers_vs_fp32_mfma", **margins)
    z = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    zb = torch.zeros(256, device="cuda")
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    bad = lambda M, N, G=1, w=None, ysc=None, out_mode=0: L.mms_linear_group_act_split16(0, G, M, N, 32, one(z), w or one(z), one(zb), one(z), one(zb), one(zb), ysc,
                                                                                         1, out_mode, None, None, None, None, None, 0, stream)
    assert bad(100, 128) != 0 and bad(128, 100) != 0 and bad(128, 128, G=0) != 0 and bad(128, 128, out_mode=1) != 0
    assert bad(128, 128, w=(ctypes.c_void_p * 1)(None)) != 0 and "null pointer" in _lib.last_error(None)
    assert bad(128, 128, ysc=one(zb), out_mode=1) == 0


def test_split16_layers_repeatable(torch_cuda):
    """Race screen for the three-stage LDS-DMA pipeline of linear_split16_kernel (counted vmcnt + raw barriers, persistent tiles with
    the next tile's slices prefetched under the epilogue): the kernel has no atomics, so every launch on the same operands must
    reproduce the first one BIT FOR BIT -- 300 launches each of a one-tile-per-CU shape, a five-tiles-per-CU grouped shape (stores in
    flight across tiles), a short-K shape (K = 64: two k-steps, the prefetch path dominates) and K = 32 (one step), planes and fp32 out;
    one and three k-steps at five tiles per CU (the rolling k-loop's first / last-slice paths with stores in flight) and the PPO first layer."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(11)
    f32 = lambda *sh: torch.empty(*sh, device="cuda")
    for (G, M, N, K, planes_out) in ((2, 4096, 1024, 1024, 1), (20, 4096, 512, 512, 1), (20, 2560, 512, 64, 0), (6, 1024, 256, 32, 1), (3, 384, 128, 96, 0),
                                   (32, 2560, 512, 32, 1), (32, 2560, 512, 96, 0), (2, 4096, 1024, 388, 1)):
        x = [torch.randn(M, K, device="cuda") for _ in range(G)]
        w = [torch.randn(N, K, device="cuda") / K ** 0.5 for _ in range(G)]
        b = [torch.randn(N, device="cuda") * 0.1 for _ in range(G)]
        xp = [torch.empty(_h32_bytes(M, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        wp = [torch.empty(_h32_bytes(N, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
        xs, xi, ws, wi = [[f32(n) for _ in range(G)] for n in (M, M, N, N)]
        _lib.check(L.mms_split_planes16_group(0, G, M, K, 0, arr(x), arr(xp), arr(xs), arr(xi), 0, 0, None, None, None, None, 0.0, stream), None, "split16 x")
        _lib.check(L.mms_split_planes16_group(0, G, N, K, 0, arr(w), arr(wp), arr(ws), arr(wi), 0, 0, None, None, None, None, 0.0, stream), None, "split16 w")
        ysc = [torch.full((M,), 256.0, device="cuda") for _ in range(G)]
        nbytes = _h32_bytes(M, N) if planes_out else M * N * 4
        ys = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(G)]
        run = lambda: L.mms_linear_group_act_split16(0, G, M, N, K, arr(xp), arr(wp), arr(b), arr(ys), arr(xi), arr(wi), arr(ysc) if planes_out else None, 1, planes_out,
                                                     None, None, None, None, None, 0, stream)
        assert run() == 0, _lib.last_error(None)
        torch.cuda.synchronize()
        first = [t.clone() for t in ys]
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        for it in range(300):
            for t in ys:
                t.zero_()
            assert run() == 0
            for t, f in zip(ys, first):
                bad += (t != f).sum()
        assert int(bad) == 0, (G, M, N, K, planes_out, int(bad))


def test_layer_clock_probe(torch_cuda):
    """mms_layer_clock_probe: with a buffer bound, workgroup 0 of every two-plane layer launch stores {shader cycles, 100-MHz ticks} of its
    life into the launch's slot (n % slots, counting from the call); the ratio is a plausible shader clock (the kernel runs power-limited,
    1.4-1.7 GHz at the PPO shape, higher on short launches: DESIGN.md 5.10), the ticks agree with the launch's HIP-event duration, the
    layer's output does not depend on the probe, and after switching it off nothing is stored."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    L = _lib.lib()
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(3)
    G, M, N, K = 2, 4096, 1024, 1024
    f32 = lambda *sh: torch.empty(*sh, device="cuda")
    x = [torch.randn(M, K, device="cuda") for _ in range(G)]
    w = [torch.randn(N, K, device="cuda") / K ** 0.5 for _ in range(G)]
    b = [torch.randn(N, device="cuda") * 0.1 for _ in range(G)]
    xp = [torch.empty(_h32_bytes(M, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
    wp = [torch.empty(_h32_bytes(N, K), dtype=torch.uint8, device="cuda") for _ in range(G)]
    xs, xi, ws, wi = [[f32(n) for _ in range(G)] for n in (M, M, N, N)]
    _lib.check(L.mms_split_planes16_group(0, G, M, K, 0, arr(x), arr(xp), arr(xs), arr(xi), 0, 0, None, None, None, None, 0.0, stream), None, "split16 x")
    _lib.check(L.mms_split_planes16_group(0, G, N, K, 0, arr(w), arr(wp), arr(ws), arr(wi), 0, 0, None, None, None, None, 0.0, stream), None, "split16 w")
    ys = [torch.zeros(M * N * 4, dtype=torch.uint8, device="cuda") for _ in range(G)]
    run = lambda: L.mms_linear_group_act_split16(0, G, M, N, K, arr(xp), arr(wp), arr(b), arr(ys), arr(xi), arr(wi), None, 1, 0, None, None, None, None, None, 0, stream)
    for _ in range(4):
        assert run() == 0, _lib.last_error(None)
    torch.cuda.synchronize()
    want = [t.clone() for t in ys]
    probe = torch.zeros(3, 2, dtype=torch.int64, device="cuda")
    tries = []
    for _ in range(3):                                                  # (the event interval of ONE launch can catch a runtime stall: best of three)
        assert L.mms_layer_clock_probe(0, ctypes.c_void_p(probe.data_ptr()), 3) == 0
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            assert run() == 0 and run() == 0                            # slots 0 and 1
            e0.record()
            assert run() == 0                                           # slot 2
            e1.record()
            assert run() == 0                                           # slot 0 again
            torch.cuda.synchronize()
        finally:
            assert L.mms_layer_clock_probe(0, None, 0) == 0
        got = probe.cpu().tolist()
        for cyc, ticks in got:
            assert cyc > 0 and ticks > 0, got
            ghz = cyc / ticks * 0.1
            assert 0.8 < ghz < 2.6, got
        tries.append((got, e0.elapsed_time(e1) * 1e3))
    got, us_events = min(tries, key=lambda t: t[1])
    assert 0.5 * us_events < got[2][1] * 0.01 < 1.1 * us_events, tries   # workgroup 0 lives most of the launch, never longer
    for a, b_ in zip(want, ys):
        assert torch.equal(a, b_)
    probe.zero_()
    assert run() == 0
    torch.cuda.synchronize()
    assert int(probe.abs().sum()) == 0                                   # off: nothing stored
    parity.record("gpu/layer_clock_probe", clock_ghz=[c / t * 0.1 for c, t in got], workgroup0_us=[t * 0.01 for _, t in got], launch_us_events=us_events)


def test_obs_planes_from_the_step_kernel(torch_cuda):
    """mms_bind_obs_planes16 on the HIP build, every ant layout of the step kernel's write-out (TenAnt packed 4 / 16 envs per block and
    one env per block at 6 ants, OneAnt, MultiAntCircle): tests/obs_planes_check.py."""
    from obs_planes_check import check_obs_planes
    worst = {}
    for task, n in (("TenAnt", 128), ("TenAnt", 4096), ("OneAnt", 256), ("MultiAntCircle", 256)):
        worst["%s/%d" % (task, n)] = check_obs_planes("cuda", task=task, num_envs=n)
    parity.record("gpu/obs_planes_from_step_kernel", **worst)


def test_actor_critic_split_layers(torch_cuda):
    """ActorCritic.act / .value with the hidden layers on the split path (batch and hidden widths multiples of 128) against the torch
    modules and against the exact-fp32 kernel path; an in-place optimizer step is picked up (the weight planes are re-split when the
    parameter's version moves)."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    torch.manual_seed(0)
    n = 256
    ac = ActorCritic((388,), (0,), (80,), 0.8, {"pi_hid_sizes": [256, 128, 128], "vf_hid_sizes": [256, 128, 128], "activation": "elu"}, seed=3).cuda()
    obs = torch.randn(n, 388, device="cuda").clamp(-5, 5)
    states = torch.zeros(n, 0, device="cuda")
    hidden_lins = [m for m in ac.actor if isinstance(m, torch.nn.Linear)][:-1]
    assert ac.split_layers and not ac._split_applies(n, hidden_lins)      # too little work for a 256-CU chip: the exact-fp32 kernel is chosen ...
    ac.split_min_tiles = 0                                                 # ... unless asked (this test is about the split path's results)
    assert ac._split_applies(n, hidden_lins)
    assert ac.split_format == "f16x2"
    for trial in range(4):
        ac.split_format = "f16x2" if trial < 2 else "bf16x3"
        _, _, v_s, mu_s, _ = ac.act(obs, states)
        val_s = ac.value(obs)
        assert ac._split_bufs, "the split path did not run"
        ac.split_layers = False
        _, _, v_f, mu_f, _ = ac.act(obs, states)
        ac.split_layers = True
        torch.cuda.synchronize()
        with torch.no_grad():
            mu_t, v_t = ac.actor(obs), ac.critic(obs)
            mu_d, v_d = copy.deepcopy(ac.actor).double()(obs.double()), copy.deepcopy(ac.critic).double()(obs.double())
        assert float((mu_s - mu_t).abs().max()) < 1e-5 and float((v_s - v_t).abs().max()) < 1e-5 and float((val_s - v_t).abs().max()) < 1e-5
        # against float64: not worse than the exact-fp32 kernel path
        assert float((mu_s.double() - mu_d).abs().max()) <= 1.0 * float((mu_f.double() - mu_d).abs().max()) + 1e-7
        assert float((v_s.double() - v_d).abs().max()) <= 1.0 * float((v_f.double() - v_d).abs().max()) + 1e-7
        # ... and not worse than torch's own fp32 modules (the reference's arithmetic)
        assert float((mu_s.double() - mu_d).abs().max()) <= 1.0 * float((mu_t.double() - mu_d).abs().max()) + 1e-7
        assert float((v_s.double() - v_d).abs().max()) <= 1.0 * float((v_t.double() - v_d).abs().max()) + 1e-7
        with torch.no_grad():                                        # "optimizer step": in place, the version counters move
            for q in ac.parameters():
                q.add_(0.01 * torch.randn_like(q))


def test_refresh_entry_points_and_module_refresh(torch_cuda):
    """tests/refresh_check.py on the HIP build (the CPU build runs the same list): the device-side refresh of the f16x2 layers' weight
    planes and bound chain, which parameter updates ActorCritic follows and when; and the weights' row 1-norms -- hence every hidden
    activation's power-of-two scale -- are the SAME numbers on both builds."""
    torch = torch_cuda
    import refresh_check
    gpu = refresh_check.check_refresh_entry_points("cuda")
    cpu = refresh_check.check_refresh_entry_points("cpu")
    for key in gpu:
        assert torch.equal(gpu[key], cpu[key]), key
    fold_gpu, fold_cpu = refresh_check.check_fold_entry_points("cuda"), refresh_check.check_fold_entry_points("cpu")
    for key in fold_gpu:                                              # the row bounds of the LayerNorm folds: the two builds sum in different orders
        assert float(((fold_gpu[key] - fold_cpu[key]).abs() / fold_cpu[key]).max()) < 1e-5, key
    stale = refresh_check.check_module_refresh("cuda", hid=(256, 128, 128), n=256, obs_dim=388)
    assert refresh_check.check_module_refresh("cuda", hid=(256, 128, 128), n=256, obs_dim=388, fmt="bf16x3") > 1e-3
    parity.record("gpu/module_refresh", stale_error_without_refresh_after_data_write=stale)


def test_actor_critic_graph_follows_parameter_updates(torch_cuda):
    """a captured rollout step replayed after an optimizer step computes with the UPDATED parameters, bit for
    bit what an eager call computes -- because every buffer derived from the parameters (operand planes, row scales, bound chain, the
    given-planes path's constant scales) lives at a stable address and ActorCritic.refresh() rebuilds them with device work only, so it
    can sit inside the graph.  Both forms: (a) a RolloutStorage is bound -> the first act of a rollout refreshes by itself (what
    bench.py captures); (b) nothing bound -> the caller puts refresh() at the head of the captured region.  Each with the policy
    splitting the observation itself and with the step kernel's operand planes (obs_planes).  Updates: torch.optim.SGD.step() (version
    counters move) and `param.data.copy_()` (they do not: hatrpo_trainer.py:122)."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
    from massive_marl_benchmark_amd.engine import Engine
    torch.manual_seed(0)
    n = 256
    eng = Engine("TenAnt", num_envs=n, device=0, seed=3, clip_obs=5.0)
    planes = torch.empty(n * ((eng.obs_dim + 31) // 32) * 128, dtype=torch.uint8, device="cuda")
    eng.bind_obs_planes(planes, 2048.0)
    for _ in range(3):
        eng.tensor("actions").uniform_(-1, 1)
        eng.step()
    obs = eng.tensor("obs_clipped").clone()
    eng.bind_obs_planes(None)
    states = torch.zeros(n, 0, device="cuda")
    cfg = {"pi_hid_sizes": [256, 128, 128], "vf_hid_sizes": [256, 128, 128], "activation": "elu"}
    n_cases = 0
    rel = lambda got, ref: float((got - ref).abs().max() / (1.0 + ref.abs().max()))
    for bound in (True, False):
        for use_planes in (False, True):
            ac = ActorCritic((388,), (0,), (80,), 0.8, cfg, seed=3).cuda()
            ac.split_min_tiles = 0
            storage = RolloutStorage(n, 2, (388,), (0,), (80,), device="cuda") if bound else None
            actions = torch.zeros(n, 80, device="cuda")
            ac.bind_rollout(storage, actions if bound else None)
            pl = (planes, 2048.0) if use_planes else None

            def eager():
                if storage is not None:
                    storage.clear()
                ac._counters.zero_()
                out = ac.act(obs, states, obs_planes=pl)
                torch.cuda.synchronize()
                return [t.clone() for t in out]

            ac.act(obs, states, obs_planes=pl)                      # warm-up: allocations happen outside the capture
            assert ac._split_bufs, "the split path did not run"
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            if storage is not None:
                storage.clear()
            with torch.cuda.stream(side):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    if not bound:
                        ac.refresh()                                # nothing bound: the caller's refresh at the head of the captured region
                    captured = ac.act(obs, states, obs_planes=pl)
            torch.cuda.current_stream().wait_stream(side)

            def replay():
                ac._counters.zero_()
                graph.replay()
                torch.cuda.synchronize()
                return [t.clone() for t in captured]

            before = eager()
            for a, b in zip(before, replay()):
                assert torch.equal(a, b)
            # 1. an optimizer step, in place
            opt = torch.optim.SGD(ac.parameters(), lr=0.3)
            for q in ac.parameters():
                q.grad = torch.randn_like(q) * 0.1
            opt.step()
            got = replay()                                           # (the replay runs BEFORE any eager call could refresh for it)
            want = eager()
            for a, b in zip(want, got):
                assert torch.equal(a, b)
            assert float((want[3] - before[3]).abs().max()) > 1e-3   # the means moved with the parameters
            with torch.no_grad():
                assert rel(got[3], ac.actor(obs)) < 1e-5 and rel(got[2], ac.critic(obs)) < 1e-5
            # 2. an update through .data (no version counter moves)
            with torch.no_grad():
                for q in ac.parameters():
                    q.data.copy_(q.data + 0.05 * torch.randn_like(q))
            got = replay()
            with torch.no_grad():
                assert rel(got[3], ac.actor(obs)) < 1e-5 and rel(got[2], ac.critic(obs)) < 1e-5
            if not bound:
                ac.refresh()                                         # eager, unbound: the documented explicit call after a .data write
            for a, b in zip(eager(), got):
                assert torch.equal(a, b)
            n_cases += 1
    eng.close()
    assert n_cases == 4


def test_ppo_training_loop_on_the_hip_path(torch_cuda):
    """a training loop where the kernels are.  tools/train_ppo_demo.py's learner (this build's restatement of
    agents/algorithms/rl/ppo/ppo.py:243-317 with cfg/ppo/config.yaml's hyper-parameters; tests/golden/run_reference_learners.py runs
    the reference's own learner classes on the CPU build) for 90 iterations at 2048 OneAnt envs through VecTaskPython + ActorCritic with the
    split layers FORCED on (hidden widths multiples of 128, split_min_tiles 0) + RolloutStorage: everything stays finite, the policy
    learns (fewer lost episodes than an untrained control, rising mean return of the episodes that end), and the layers' operand planes follow EVERY
    optimizer step (1800 Adam steps) -- after the last update `act` agrees with the torch modules evaluated on the updated parameters."""
    torch = torch_cuda
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ppo_demo
    base = ["--task", "OneAnt", "--num-envs", "2048", "--iterations", "90", "--hidden", "256", "128", "128", "--split-min-tiles", "0", "--log-every", "1000"]
    control = train_ppo_demo.train(train_ppo_demo.parse(base + ["--lr", "0", "--fixed-lr"]), log=lambda m: None)
    control_late = sum(c for _, c in control["episodes"][60:])
    control_total = sum(c for _, c in control["episodes"])
    control["env"].task.engine.close()
    for use_planes in (False, True):
        args = train_ppo_demo.parse(base + (["--obs-planes"] if use_planes else []))
        out = train_ppo_demo.train(args, log=lambda m: None)
        ac, obs, states, hist, eps = out["ac"], out["obs"], out["states"], out["reward_per_step"], out["episodes"]
        assert ac._split_bufs and ac._h16 is not None, "the split path did not run"
        assert all(np.isfinite(hist)) and bool(torch.isfinite(obs).all())
        # learning: against a CONTROL run of the same loop from the same seed with a learning rate of zero (the initial policy, whose
        # ants keep falling at a steady rate: ~850 episodes lost in each of the last two thirds of the run) the trained policy loses
        # fewer episodes -- over the whole run fewer than 0.6 x the control's, in the last third fewer than the control.  WHICH gait a
        # run finds moves with the arithmetic's last bits (so with the compiler) and with the seed: over seeds 1-8 x both observation
        # paths, 13 of 16 runs pass every gate here at 2048 envs (total 0.12-0.50 x, late 0.01-0.62 x; this seed 0.18 / 0.23 x) against
        # 6 of 16 at 1024 envs, where the gate sat on the edge of the spread.  The mean return of the episodes that end -- the quantity
        # the reference logs, ppo.py:196-201 -- does not fall (second half of the ended episodes against the first; only guarded
        # against a drop)
        ended_late = sum(c for _, c in eps[60:])
        ended_total = sum(c for _, c in eps)
        assert control_late > 10 and ended_late < control_late, (ended_late, control_late)
        assert ended_total < 0.6 * control_total, (ended_total, control_total)
        ended = [(r / c, c) for r, c in eps if c > 0]
        total = sum(c for _, c in ended)
        assert total >= 20, total
        half, acc, first_sum, first_n = total // 2, 0, 0.0, 0
        for m, c in ended:
            take = min(c, half - acc)
            first_sum += m * take; first_n += take; acc += take
            if acc >= half:
                break
        first = first_sum / max(first_n, 1)
        last = (sum(m * c for m, c in ended) - first_sum) / max(total - first_n, 1)
        assert last >= 0.9 * first, (first, last)                     # (recorded; the control comparison above is the learning signal with a margin)
        with torch.no_grad():
            _, _, v, mu, _ = ac.act(obs, states)
            mu_t, v_t = ac.actor(obs), ac.critic(obs)
        rel = lambda a, b: float((a - b).abs().max() / (1.0 + b.abs().max()))
        assert rel(mu, mu_t) < 1e-5 and rel(v, v_t) < 1e-5, (rel(mu, mu_t), rel(v, v_t))
        parity.record("gpu/ppo_training_loop/%s" % ("obs_planes" if use_planes else "own_split"), mean_return_first_half_of_ended_episodes=first, mean_return_second_half=last, episodes_lost_last_third=ended_late,
                      episodes_lost_last_third_untrained_control=control_late, episodes_lost=ended_total, episodes_lost_untrained_control=control_total,
                      act_vs_torch_after_last_update=max(rel(mu, mu_t), rel(v, v_t)))
        out["env"].task.engine.close()


def test_policy_head_fused_into_the_step(torch_cuda):
    """mms_bind_policy_head on the HIP build at BASELINE size (4096 TenAnt envs: the 16-envs-per-workgroup layout the fused prologue exists
    for), policy [1024, 1024, 512] as in the bench: six rollout steps with the heads + sampling in the step kernel's prologue leave, bit for
    bit, what mms_ppo_heads_act + mms_step leave (tests/head_fusion_check.py: rollout slots, draw counters, engine state)."""
    import head_fusion_check
    assert head_fusion_check.check_head_fusion("cuda", 4096, hidden=(1024, 1024, 512))
    assert head_fusion_check.check_head_bind_errors("cuda", 4096)


def test_fused_head_graph_follows_parameter_updates(torch_cuda):
    """The captured form of the fused policy head (bench.py's graph: refresh at the head of a rollout, `act` binds the head, the step kernel
    evaluates it) after an optimizer step and after a `.data` write: a replay leaves in the rollout slots, bit for bit, what the UNFUSED
    path (mms_ppo_heads_act reading the row-major weight itself) leaves for the updated parameters -- so the tiled copy of the actor's last
    layer (mms_policy_head.weight_tiles) is rebuilt inside the graph like every other derived buffer."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
    from massive_marl_benchmark_amd.engine import Engine
    torch.manual_seed(1)
    n = 4096
    eng = Engine("TenAnt", num_envs=n, device=0, seed=5, clip_obs=5.0)
    assert eng.takes_policy_head()
    ac = ActorCritic((eng.obs_dim,), (0,), (eng.num_actions,), 0.8, {"pi_hid_sizes": [256, 512], "vf_hid_sizes": [256, 512], "activation": "elu"}, seed=9).cuda()
    ac.split_min_tiles = 0
    obs = torch.randn(n, eng.obs_dim, device="cuda").clamp(-5, 5)
    states = torch.zeros(n, 0, device="cuda")
    storage = RolloutStorage(n, 2, (eng.obs_dim,), (0,), (eng.num_actions,), device="cuda")
    actions = eng.tensor("actions")

    def slots():
        torch.cuda.synchronize()
        return [t[0].clone() for t in (storage.actions, storage.actions_log_prob, storage.values, storage.mu, storage.sigma)] + [actions.clone()]

    def unfused():
        ac.bind_rollout(storage, actions, step_engine=None)
        storage.clear()
        ac._counters.zero_()
        act, logp, value, mu, sigma = ac.act(obs, states)
        storage.add_transitions(obs, states, act, storage.rewards[0], storage.dones[0], value, logp, mu, sigma)
        out = slots()
        ac.bind_rollout(storage, actions, step_engine=eng)
        storage.clear()
        return out

    ac.bind_rollout(storage, actions, step_engine=eng)
    assert ac._step_engine is not None
    ac.act(obs, states)                                             # warm-up: buffers (among them the tiled copy) are allocated outside the capture
    eng.step()
    storage.clear()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ac.act(obs, states)                                     # storage.step == 0: refresh() is inside; the head is bound ...
            eng.step()                                              # ... and evaluated in this launch's prologue
    torch.cuda.current_stream().wait_stream(side)

    def replay():
        ac._counters.zero_()
        graph.replay()
        return slots()

    want = unfused()
    for a, b in zip(want, replay()):
        assert torch.equal(a, b)
    before_mu = want[3]
    opt = torch.optim.SGD(ac.parameters(), lr=0.3)
    for q in ac.parameters():
        q.grad = torch.randn_like(q) * 0.1
    opt.step()
    got = replay()                                                  # (BEFORE any eager call could refresh for it)
    want = unfused()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert float((want[3] - before_mu).abs().max()) > 1e-3          # the means moved with the parameters
    with torch.no_grad():
        for q in ac.parameters():
            q.data.copy_(q.data + 0.05 * torch.randn_like(q))        # no version counter moves
    got = replay()
    want = unfused()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    with torch.no_grad():
        rel = float((got[3] - ac.actor(obs)).abs().max() / (1.0 + ac.actor(obs).abs().max()))
    assert rel < 1e-5, rel
    parity.record("gpu/fused_head_graph_after_updates", mean_vs_torch=rel)
    ac.bind_rollout(None, None)
    eng.close()


def test_abi_error_paths_and_indexed_set_state(torch_cuda):
    """The status-code contract of include/mms.h on the HIP build (the list of tests/abi_errors.py, as on the CPU build), and
    mms_set_state with more than 16 env ids: one scatter launch (the reference's indexed setters take thousands of ids,
    ten_ant.py:867-875), from a host array and from a device tensor, equal to the per-row result."""
    torch = torch_cuda
    import abi_errors
    from massive_marl_benchmark_amd import _lib
    from massive_marl_benchmark_amd.engine import Engine
    assert abi_errors.check_abi_error_paths(_lib.lib(), 0) >= 40
    n = 4096
    eng = Engine("TenAnt", num_envs=n, device=0, seed=1)
    g = torch.Generator().manual_seed(0)
    ids = torch.randperm(n, generator=g)[:1500].tolist()
    rows = torch.randn(1500, 11 * 13, generator=g)
    want = eng.tensor("root_states").clone().view(n, -1)
    want[ids] = rows.cuda()
    eng.set_state("root_states", rows.numpy(), env_ids=ids)          # host source
    torch.cuda.synchronize()
    assert torch.equal(eng.tensor("root_states").view(n, -1), want)
    rows2 = torch.randn(1500, 80 * 2, generator=g).cuda()
    want2 = eng.tensor("dof_state").clone().view(n, -1)
    want2[ids] = rows2
    eng.set_state("dof_state", rows2, env_ids=ids)                   # device source
    torch.cuda.synchronize()
    assert torch.equal(eng.tensor("dof_state").view(n, -1), want2)
    prog = torch.arange(20, dtype=torch.int64)
    eng.set_state("progress", prog.numpy(), env_ids=list(range(100, 120)))      # int64 rows of one element
    torch.cuda.synchronize()
    assert torch.equal(eng.tensor("progress")[100:120].cpu(), prog)
    with pytest.raises(_lib.MmsError, match="out of range"):
        eng.set_state("progress", prog.numpy(), env_ids=list(range(100, 119)) + [n])
    assert torch.equal(eng.tensor("progress")[100:120].cpu(), prog)
    eng.close()


# the calls of tests/abi_errors.py whose failure IS the device argument: each build names its own device rule, in its own words
DEVICE_ARGUMENT_CALLS = ["mms_create, the other library's device", "mms_create, device out of range", "mms_gae_ppo, the other library's device"]


def test_both_builds_refuse_in_the_same_words(torch_cuda):
    """The CPU build stands in for the HIP build's boundary on machines without a GPU, so a call one of them refuses the other refuses with
    the same message (csrc/mms_host.h holds each rule once): the list of tests/abi_errors.py on both builds, message against message.
    The exceptions are the calls that fail on the device argument itself, and the one call only the HIP build can make (an ordinal
    past the last device)."""
    import abi_errors
    from massive_marl_benchmark_amd import _lib
    hip, cpu = [], []
    assert abi_errors.check_abi_error_paths(_lib.lib(), 0, hip) >= 40
    assert abi_errors.check_abi_error_paths(_lib.lib_cpu(), -1, cpu) >= 40
    hip, cpu = dict(hip), dict(cpu)
    assert set(hip) - set(cpu) == {"mms_create, device out of range"} and not set(cpu) - set(hip)
    assert set(DEVICE_ARGUMENT_CALLS) <= set(hip)
    compared = [k for k in cpu if k not in DEVICE_ARGUMENT_CALLS]
    assert len(compared) >= 40
    for k in compared:
        assert hip[k] == cpu[k], (k, hip[k], cpu[k])


@pytest.mark.parametrize("task,kw", [("TenAnt", {}), ("OneAnt", {}), ("MultiAntCircle", {}), ("MultiIngenuity", {}), ("TenAnt", {"num_agents": 100})])
def test_both_builds_construct_the_same_scene(torch_cuda, task, kw):
    """Right after mms_create every named buffer is bit-identical between the builds (one scene function, csrc/mms_host.h), for a shard in
    the middle of a larger grid: non-zero env_offset, total_envs above num_envs."""
    from massive_marl_benchmark_amd.engine import Engine
    names = ["actions", "obs", "obs_clipped", "rew", "reset", "progress", "reset_count", "root_states", "initial_root_states", "dof_state",
             "env_origin", "prev", "reset_noise", "foot_sensors", "dr_params"]
    args = dict(num_envs=24, seed=5, env_offset=37, total_envs=200, **kw)
    hip, cpu = Engine(task, device=0, **args), Engine(task, device="cpu", **args)
    try:
        origin = hip.tensor("env_origin").cpu()
        assert float(origin[:, 0].max()) > 0 and float(origin[:, 1].min()) > 0       # (a shard away from the grid's first row)
        for name in names:
            a, b = hip.tensor(name).cpu(), cpu.tensor(name)
            assert a.dtype == b.dtype and a.shape == b.shape, name
            assert torch_cuda.equal(a.view(torch_cuda.uint8), b.view(torch_cuda.uint8)), name
    finally:
        hip.close()
        cpu.close()


def test_bench_under_torchrun_single_rank(torch_cuda):
    """bench.py launched the way the driver launches the multi-GPU runs -- `python -m torch.distributed.run --nproc-per-node 1
    --master-addr 127.0.0.1 ... bench.py --gpus 1` as a fresh child process -- takes the RCCL path (init_process_group("nccl"),
    barrier, all_reduce(MAX) of the timings) at world size 1 and prints one well-formed JSON line.  A rehearsal of the control
    flow only: no scaling figure can come from one GPU."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MMS_BENCH_TRACE_DIST="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "16", "--warmup", "8", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 16 and out["warmup"] == 8 and out["scaling"] == "weak" and out["value"] > 1e6
    assert out["config"]["distributed"] == {"backend": "nccl", "world_size": 1}
    assert out["roofline"]["frac"] > 0 and out["config"]["finite"]
    # the default path and its A/Bs are all in the line: two fp16 planes (headline), three bf16 planes, exact fp32; the layers' roofline
    assert out["config"]["obs_planes_from_step_kernel"] is True and "mms_linear_group_act_split16" in out["config"]["policy_layers"]
    assert out["rollout_bf16x3_layers"]["value"] > 1e6 and out["rollout_exact_fp32_layers"]["value"] > 1e6
    assert out["value"] > out["rollout_bf16x3_layers"]["value"] > out["rollout_exact_fp32_layers"]["value"]
    err = out["policy_layers_error_vs_f64"]
    assert err["split_2xf16"]["rms"] < err["exact_fp32_mfma"]["rms"] and err["split_3xbf16"]["rms"] < err["exact_fp32_mfma"]["rms"]
    roof = out["roofline_policy_layers"]
    assert roof["bound"] == "mfma" and roof["peak"] == 2500.0 and 0.05 < roof["frac"] < 1.0 and roof["plane_products_per_fp32_product"] == 3


def test_bench_plain_run_dumps_the_last_step(torch_cuda, tmp_path):
    """A plain `bench.py` run (no --full) times the headline only and, with --dump-outputs, leaves what its last timed step computed:
    K = 12 ends inside a rollout (slot 3, no returns yet), the arrays are float32, finite and shaped as the rollout slots."""
    import json
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "4", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 12 and out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["value"] > 1e6
    assert abs(out["ms_per_step"] - 1e3 * 4096 / out["value"]) < 1e-6 * out["ms_per_step"] and "split16" in out["config"]["policy_layers"]
    assert not {"sim_only", "roofline", "cpu_baseline", "rollout_eager", "policy_layers_error_vs_f64", "ms_per_step_repeat"} & set(out)
    shapes = {"obs": (4096, 388), "next_obs": (4096, 388), "actions": (4096, 80), "mu": (4096, 80), "sigma": (4096, 80),
              "actions_log_prob": (4096, 1), "values": (4096, 1), "rewards": (4096, 1), "dones": (4096, 1)}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    for name, shape in shapes.items():
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), name
    assert float(np.abs(np.load(tmp_path / "actions.npy")).max()) > 0


def test_fused_act_and_bound_rollout(torch_cuda):
    """ActorCritic.act (fused tail) + RolloutStorage + engine, all zero-copy: slot t of the storage holds exactly what the
    reference's act -> step -> add_transitions sequence would have copied there."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
    from massive_marl_benchmark_amd.engine import Engine
    n, T = 192, 4
    eng = Engine("TenAnt", num_envs=n, device=0, seed=3)
    torch.manual_seed(0)
    ac = ActorCritic((388,), (0,), (80,), 0.8, {"pi_hid_sizes": [64, 64], "vf_hid_sizes": [64, 64], "activation": "elu"},
                     seed=11).cuda()
    ac.fuse_head = True                                            # exercise mms_ppo_heads_act through the module (H = 64)
    st = RolloutStorage(n, T, (388,), (0,), (80,), device="cuda:0")
    ac.bind_rollout(st, eng.tensor("actions"))
    states = torch.zeros(n, 0, device="cuda")
    eng.tensor("actions").zero_()
    eng.step()                                                     # first step = full reset
    cur = eng.tensor("obs_clipped").clone()
    for t in range(T):
        st.observations[t].copy_(cur)
        actions, logp, values, mu, sigma = ac.act(st.observations[t], states)
        assert actions.data_ptr() == st.actions[t].data_ptr() and values.data_ptr() == st.values[t].data_ptr()
        assert torch.equal(eng.tensor("actions"), actions)
        with torch.no_grad():
            lp2, _, v2, mu2, sg2 = ac.evaluate(st.observations[t], states, actions)
        assert float((lp2 - logp).abs().max()) < 5e-3              # (a - mu) / sigma^2 in fp32 vs the noise itself
        assert float((v2 - values).abs().max()) < 1e-5 and float((mu2 - mu).abs().max()) < 1e-5
        assert torch.equal(sg2, sigma)
        eng.bind_rollout_out(st.rewards[t].view(-1), st.dones[t].view(-1))
        eng.step()
        st.add_transitions(st.observations[t], states, actions, st.rewards[t], st.dones[t], values, logp, mu, sigma)
        torch.cuda.synchronize()
        assert torch.equal(st.rewards[t].view(-1), eng.tensor("rew"))
        assert torch.equal(st.dones[t].view(-1).long(), eng.tensor("reset"))
        assert torch.equal(st.actions[t], actions) and torch.equal(st.actions_log_prob[t].view(-1), logp)
        cur = eng.tensor("obs_clipped").clone()
    assert st.step == T
    # hidden layers through mms_linear2_act (+ both heads in the sampling kernel): same means / values as the library path
    for heads in (False, True):
        ac.fuse_layers, ac.fuse_head = True, heads
        st.clear()
        _, _, v_f, mu_f, _ = ac.act(st.observations[0], states)
        torch.cuda.synchronize()
        with torch.no_grad():
            assert float((ac.actor(st.observations[0]) - mu_f).abs().max()) < 1e-5 and float((ac.critic(st.observations[0]) - v_f).abs().max()) < 1e-5
    ac.fuse_layers, ac.fuse_head = True, True
    st.clear()
    _, _, v_f, mu_f, _ = ac.act(st.observations[0], states)
    ac.fuse_layers = False
    with torch.no_grad():
        assert float((ac.actor(st.observations[0]) - mu_f).abs().max()) < 1e-5 and float((ac.critic(st.observations[0]) - v_f).abs().max()) < 1e-5
    # deferred critic: act returns before the value is there; after join() the slot holds the critic's output
    st.clear()
    ac.defer_value = True
    _, _, values, _, _ = ac.act(st.observations[0], states)
    ac.join()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert float((ac.critic(st.observations[0]) - values).abs().max()) < 1e-5
    ac.defer_value = False
    z = (st.actions - st.mu) / torch.exp(2.0 * ac.log_std.detach())
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    eng.bind_rollout_out(None, None)
    eng.close()


def test_replay_buffer_bound_slots(torch_cuda):
    """The DDPG / TD3 collection loop (ddpg.py:151-159) on MultiIngenuity (BASELINE configs[2]) and OneAnt, twice: through the
    wrapper's return values + copies, and with the step kernel bound to the ring row `ReplayBuffer.slot()` names.  Same seed,
    same actions -> identical rings, across the overflow that skips row 0."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.td3.storage import ReplayBuffer
    from massive_marl_benchmark_amd.engine import Engine
    for task in ("MultiIngenuity", "OneAnt"):
        n, R, steps = 200, 5, 13
        e1 = Engine(task, num_envs=n, device=0, seed=6)
        e2 = Engine(task, num_envs=n, device=0, seed=6)
        W, AD = e1.obs_dim, e1.num_actions
        b1 = ReplayBuffer(n, R, 64, 8, (W,), (0,), (AD,), "cuda:0")
        b2 = ReplayBuffer(n, R, 64, 8, (W,), (0,), (AD,), "cuda:0")
        g = torch.Generator().manual_seed(9)
        states = torch.zeros(n, 0, device="cuda")
        for e in (e1, e2):
            e.tensor("actions").zero_()
            e.step()                                                   # first step = full reset
        cur1, cur2 = e1.tensor("obs_clipped").clone(), e2.tensor("obs_clipped").clone()
        for t in range(steps):
            a = (torch.rand(n, AD, generator=g) * 2 - 1).cuda()
            # copies
            e1.tensor("actions").copy_(a)
            e1.step()
            b1.add_transitions(cur1, states, a, e1.tensor("rew"), e1.tensor("obs_clipped"), e1.tensor("reset"))
            cur1.copy_(e1.tensor("obs_clipped"))
            # in place
            k = b2.slot()
            e2.bind_obs_out(b2.next_observations[k])
            e2.bind_rollout_out(b2.rewards[k].view(-1), b2.dones[k].view(-1))
            e2.tensor("actions").copy_(a)
            e2.step()
            b2.add_transitions(cur2, states, a, b2.rewards[k], b2.next_observations[k], b2.dones[k])
            cur2.copy_(b2.next_observations[k])
            assert b1.step == b2.step and b1.fullfill == b2.fullfill
        torch.cuda.synchronize()
        for name in ("observations", "next_observations", "actions", "rewards", "dones"):
            assert torch.equal(getattr(b1, name), getattr(b2, name)), (task, name)
        assert b1.fullfill and torch.isfinite(b1.next_observations).all()
        s1, s2 = b1.get_statistics(), b2.get_statistics()
        assert float(s1[0]) == float(s2[0]) and float(s1[1]) == float(s2[1])
        e2.bind_obs_out(None)
        e2.bind_rollout_out(None, None)
        e1.close(); e2.close()


def test_offpolicy_actor_fused_layers(torch_cuda):
    """The DDPG / TD3 actor through mms_linear2_act (ReLU hidden layers, tanh output; act codes 2 and 3 of the kernel) against the
    same nn.Sequential run by the library, on the three kernel variants (K tail, K % 32 == 0, ragged N); then act() on the
    device: deterministic = the library forward, noisy = within the limit and N(0, act_noise) around it."""
    torch = torch_cuda
    import torch.nn as nn
    from massive_marl_benchmark_amd import spaces
    from massive_marl_benchmark_amd.algorithms.rl.ddpg.module import fused_mlp_forward, mlp
    from massive_marl_benchmark_amd.algorithms.rl.td3.module import MLPActorCritic
    torch.manual_seed(3)
    for (M, sizes, act) in ((8192, [52, 256, 256, 256, 24], nn.ReLU), (1000, [60, 128, 64, 8], nn.ELU), (384, [388, 256, 128, 80], nn.Tanh),
                            (7, [4, 12, 3], nn.Identity)):
        seq = mlp(sizes, act, nn.Tanh).cuda()
        x = 2.0 * torch.randn(M, sizes[0], device="cuda")
        with torch.no_grad():
            y = fused_mlp_forward(seq, x)
            ref = seq(x)
        assert y is not None and y.shape == ref.shape
        assert float((y - ref).abs().max()) < 2e-5, (M, sizes)
        assert fused_mlp_forward(seq, x) is None                     # gradients wanted: the library path keeps the graph
    ac = MLPActorCritic(spaces.Box(-np.inf * np.ones(52), np.inf * np.ones(52)), spaces.Box(-np.ones(24), np.ones(24)), 0.1, "cuda:0",
                        hidden_sizes=[256, 256, 256]).cuda()
    o = torch.randn(8192, 52, device="cuda")
    det = ac.act(o)
    with torch.no_grad():
        assert float((det - ac.act_limit * ac.pi.pi(o)).abs().max()) < 2e-5
    noisy = ac.act(o, deterministic=False)
    assert float(noisy.abs().max()) <= 1.0
    inner = det.abs() < 0.5                                           # away from the clip
    z = ((noisy - det) / 0.1)[inner]
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    assert ac.pi(o).requires_grad


def test_optional_observation_rows(torch_cuda):
    """mms_set_obs_outputs: a switched-off engine row keeps its last contents, the bound slot and everything else still follow
    the state; switching back on resumes."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    for task, width in (("TenAnt", 388), ("MultiIngenuity", 52)):
        n = 96
        e1 = Engine(task, num_envs=n, device=0, seed=4)
        e2 = Engine(task, num_envs=n, device=0, seed=4)
        acts = [(torch.rand(n, e1.num_actions) * 2 - 1).cuda() for _ in range(3)]
        slot = torch.zeros(n, width, device="cuda")
        e2.bind_obs_out(slot)
        for e in (e1, e2):
            e.tensor("actions").copy_(acts[0])
            e.step()
        torch.cuda.synchronize()
        kept_raw, kept_clip = e2.tensor("obs").clone(), e2.tensor("obs_clipped").clone()
        e2.set_obs_outputs(raw=False, clipped=False)
        for e in (e1, e2):
            e.tensor("actions").copy_(acts[1])
            e.step()
        torch.cuda.synchronize()
        assert torch.equal(e2.tensor("obs"), kept_raw) and torch.equal(e2.tensor("obs_clipped"), kept_clip)
        assert torch.equal(slot, e1.tensor("obs_clipped")) and torch.equal(e1.tensor("rew"), e2.tensor("rew"))
        e2.set_obs_outputs(raw=True, clipped=True)
        for e in (e1, e2):
            e.tensor("actions").copy_(acts[2])
            e.step()
        torch.cuda.synchronize()
        assert torch.equal(e2.tensor("obs"), e1.tensor("obs")) and torch.equal(e2.tensor("obs_clipped"), e1.tensor("obs_clipped"))
        e1.close()
        e2.close()


def test_rollout_kernels_random_shapes(torch_cuda):
    """GAE scans, the advantage normalisation and the MARL view gather against the oracle on ragged sizes: one env, one
    step, sizes that are not multiples of the 256-thread blocks, an empty batch."""
    torch = torch_cuda
    from massive_marl_benchmark_amd import _lib
    from oracle.oracle import U8, fp, lib as olib_
    olib, L = olib_(), _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(12)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for (T, N) in ((1, 1), (8, 1), (1, 257), (8, 4097), (13, 1000), (3, 65536 + 5)):
        rew = (5 * rng.standard_normal((T, N))).astype(np.float32)
        val = rng.standard_normal((T, N)).astype(np.float32)
        done = (rng.random((T, N)) < 0.15).astype(np.uint8)
        last = rng.standard_normal(N).astype(np.float32)
        ret, adv = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
        norm = T * N > 1
        olib.mo_gae_ppo(T, N, fp(rew), done.ctypes.data_as(U8), fp(val), fp(last), 0.96, 0.95, fp(ret), fp(adv), 1 if norm else 0)
        d = {k: cu(v) for k, v in (("rew", rew), ("done", done), ("val", val), ("last", last))}
        gret, gadv = torch.zeros(T, N, device="cuda"), torch.zeros(T, N, device="cuda")
        stats = torch.zeros(3, dtype=torch.float64, device="cuda")
        _lib.check(L.mms_gae_ppo(0, p(d["rew"]), p(d["done"]), p(d["val"]), p(d["last"]), p(gret), p(gadv), p(stats), T, N, 0.96, 0.95, stream), None, "gae")
        if norm:
            _lib.check(L.mms_adv_normalize(0, p(gadv), p(stats), T * N, stream), None, "norm")
        torch.cuda.synchronize()
        assert np.max(np.abs(to_np(gret) - ret)) < 1e-4, (T, N)
        assert np.max(np.abs(to_np(gadv) - adv)) < 2e-5 * max(1.0, float(np.abs(adv).max())), (T, N)
        if norm:                                                      # the one-rank form: per-block partials, fixed summation order
            fret, fadv = torch.full((T, N), 7.0, device="cuda"), torch.full((T, N), 7.0, device="cuda")
            fstats = torch.full((3 + 2 * 2048,), 1e30, dtype=torch.float64, device="cuda")      # MMS_GAE_STATS_DOUBLES; needs no zeroing
            runs = []
            for _ in range(2):
                _lib.check(L.mms_gae_ppo_normalized(0, p(d["rew"]), p(d["done"]), p(d["val"]), p(d["last"]), p(fret), p(fadv), p(fstats), T, N, 0.96, 0.95, stream),
                           None, "gae normalized")
                torch.cuda.synchronize()
                runs.append((fret.clone(), fadv.clone(), fstats[:3].clone()))
            assert np.max(np.abs(to_np(fret) - ret)) < 1e-4, (T, N)
            assert np.max(np.abs(to_np(fadv) - adv)) < 2e-5 * max(1.0, float(np.abs(adv).max())), (T, N)
            assert abs(float(fstats[2]) - T * N) == 0 and abs(float(fstats[0]) - float(stats[0])) <= 1e-9 * float(stats[1]) ** 0.5 + 1e-9
            assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), (T, N)       # fixed summation order: bit-reproducible
        # MARL scan on the same data (masks = 1 - done, value_preds with the bootstrap row appended)
        vp = np.concatenate([val, last[None]], 0)
        masks = np.concatenate([np.ones((1, N), np.float32), 1.0 - done.astype(np.float32)], 0)
        for use_norm, mean, var in ((0, 0.0, 1.0), (1, 0.3, 2.5)):
            mret = np.zeros((T + 1, N), np.float32)
            olib.mo_gae_marl(T, N, fp(rew), fp(vp), fp(masks), 0.99, 0.95, use_norm, mean, var, fp(mret))
            gm = torch.zeros(T + 1, N, device="cuda")
            tm, tv = torch.tensor([mean], device="cuda"), torch.tensor([var], device="cuda")
            tvp, tmask = cu(vp), cu(masks)                  # named: a temporary would be freed (and its block reused) before the launch
            _lib.check(L.mms_gae_marl(0, p(d["rew"]), p(tvp), p(tmask), p(gm), T, N, 0.99, 0.95, use_norm, p(tm), p(tv), stream), None, "marl")
            torch.cuda.synchronize()
            assert np.max(np.abs(to_np(gm)[:T] - mret[:T])) < 1e-4 * max(1.0, float(np.abs(mret).max())), (T, N, use_norm)
    for (n, agents, per, shared) in ((1, 1, 3, 2), (7, 10, 38, 8), (300, 100, 38, 8), (5, 4, 13, 0)):
        row = agents * per + shared
        obs = (6 * rng.standard_normal((n, row))).astype(np.float32)
        want = np.zeros((n, agents, per + shared), np.float32)
        olib.mo_marl_views(n, agents, per, shared, 7.0, fp(obs), fp(want))
        got = torch.zeros(n, agents, per + shared, device="cuda")
        clipped = cu(np.clip(obs, -7.0, 7.0))
        _lib.check(L.mms_marl_views(0, p(clipped), p(got), n, agents, per, shared, stream), None, "views")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(to_np(got), want)
    # empty batches are accepted and touch nothing
    z = torch.zeros(4, device="cuda")
    zc = torch.zeros(4, dtype=torch.int64, device="cuda")
    _lib.check(L.mms_ppo_act(0, p(z), p(z), p(z), 1, p(zc), 0, 1, p(z), None, None, None, None, None, 0, 4, stream), None, "empty act")
    _lib.check(L.mms_marl_views(0, p(z), p(z), 0, 2, 1, 0, stream), None, "empty views")
    torch.cuda.synchronize()
    assert int(zc.sum()) == 0


def test_rccl_backend_world_size_one(torch_cuda):
    """The collectives of the multi-GPU paths on the RCCL backend itself (the 2-rank tests run on gloo, CPU): a one-rank "nccl"
    group on this GPU -- RolloutStorage's global advantage statistics (all_reduce of the float64 triple between the two
    kernels) and all_gather_envs give what the group-less calls give."""
    torch = torch_cuda
    import torch.distributed as dist
    from massive_marl_benchmark_amd.algorithms.marl.utils.shared_buffer import all_gather_envs
    from massive_marl_benchmark_amd.algorithms.rl.ppo.storage import RolloutStorage
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        T, N = 8, 1000
        g = torch.Generator(device="cuda").manual_seed(5)
        outs = []
        for pg in (None, dist.group.WORLD):
            st = RolloutStorage(N, T, (4,), (0,), (2,), device="cuda:0", process_group=pg)
            g.manual_seed(5)
            st.rewards.copy_(torch.randn(T, N, 1, generator=g, device="cuda"))
            st.values.copy_(torch.randn(T, N, 1, generator=g, device="cuda"))
            st.dones.copy_((torch.rand(T, N, 1, generator=g, device="cuda") < 0.1).byte())
            st.compute_returns(torch.randn(N, 1, generator=g, device="cuda"), 0.96, 0.95)
            torch.cuda.synchronize()
            outs.append((st.returns.clone(), st.advantages.clone()))
        # (the group-less call is the one-launch form with a fixed summation order, the grouped one sums with float64 atomics: the
        #  statistics agree to ~1e-16 relative, the normalised advantages to an ulp or two)
        assert torch.equal(outs[0][0], outs[1][0]) and float((outs[0][1] - outs[1][1]).abs().max()) <= 1e-6
        x = {"obs": torch.randn(T + 1, N, 46, device="cuda"), "rewards": torch.randn(T, N, 1, device="cuda")}
        y = all_gather_envs(x, dist.group.WORLD)
        assert all(torch.equal(x[k], y[k]) for k in x)
    finally:
        dist.destroy_process_group()


def test_long_soak_stays_bounded(torch_cuda):
    """5000 control steps (83 simulated seconds, 10000 substeps) of 4096 TenAnt envs under full-range random actions, captured as
    a hipGraph: no NaN / Inf, speeds, heights and joint angles stay physical, episodes keep terminating and restarting."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.engine import Engine
    N = 4096
    eng = Engine("TenAnt", num_envs=N, device=0, seed=1)
    g = torch.Generator().manual_seed(7)
    ring = [(torch.rand(N, 80, generator=g) * 2 - 1).cuda() for _ in range(10)]
    act = eng.tensor("actions")
    for i in range(10):
        act.copy_(ring[i]); eng.step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for i in range(10):
                act.copy_(ring[i]); eng.step()
    torch.cuda.current_stream().wait_stream(side)
    worst_v = worst_w = 0.0
    for chunk in range(10):
        for _ in range(50):
            graph.replay()
        torch.cuda.synchronize()
        r = eng.tensor("root_states").view(N, 11, 13)
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(eng.tensor("dof_state")).all()) and bool(torch.isfinite(eng.tensor("obs")).all())
        worst_v = max(worst_v, float(r[:, :, 7:10].abs().max()))
        worst_w = max(worst_w, float(r[:, :, 10:13].norm(dim=-1).max()))
        assert float(r[:, :10, 2].max()) < 3.0 and float(r[:, :10, 2].min()) > 0.0        # nobody launched, nobody under the ground
        assert 0.45 < float(r[:, 10, 2].min()) and float(r[:, 10, 2].max()) < 1.01         # the box: resting (0.5) or just reset (dropped from 1.0)
        q = eng.tensor("dof_state").view(N, 80, 2)[:, :, 0]
        assert float(q.abs().max()) < 2.0                                                  # joint limits are +-0.7 / up to 1.75 rad
    assert worst_v < 15.0 and worst_w <= 64.0 + 1e-3, (worst_v, worst_w)                   # 64 rad/s is the model's spin clamp
    rc = eng.tensor("reset_count")
    assert int(rc.min()) >= 2 and int(rc.max()) < 400                                      # every env has fallen and restarted, none is stuck resetting
    eng.close()


@pytest.mark.gpu
def test_actor_critic_value_path(torch_cuda):
    """ActorCritic.value (the bootstrap value of a rollout: the critic alone through mms_linear2_act with one network + a
    matrix-vector output layer) against the torch module it replaces; fp32 products and sums on both sides: 1e-5 of the scale."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    torch.manual_seed(3)
    ac = ActorCritic((388,), (0,), (80,), 0.8, {"pi_hid_sizes": [1024, 1024, 512], "vf_hid_sizes": [1024, 1024, 512], "activation": "elu"}, seed=1).cuda()
    x = torch.randn(4096, 388, device="cuda") * 2
    with torch.no_grad():
        want = ac.critic(x)
    got = ac.value(x)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-5 * (1.0 + want.abs().max().item())
    odd = torch.randn(37, 388, device="cuda")                       # a batch the fast tiling does not cover
    with torch.no_grad():
        assert (ac.value(odd) - ac.critic(odd)).abs().max().item() <= 1e-5 * (1.0 + ac.critic(odd).abs().max().item())


@pytest.mark.gpu
def test_actor_critic_deferred_critic_path(torch_cuda):
    """`defer_value`: the actor's layers alone in front of the sampling kernel, the whole critic pass on the second stream until
    `join()`.  Same noise stream, same layer arithmetic: actions / log-probs equal the default path's, values to rounding."""
    torch = torch_cuda
    from massive_marl_benchmark_amd.algorithms.rl.ppo.module import ActorCritic
    cfg = {"pi_hid_sizes": [256, 128], "vf_hid_sizes": [256, 128], "activation": "elu"}
    x = torch.randn(512, 388, device="cuda")
    states = torch.zeros(512, 0, device="cuda")
    outs = []
    for defer in (False, True):
        torch.manual_seed(5)
        ac = ActorCritic((388,), (0,), (80,), 0.8, cfg, seed=11).cuda()
        ac.defer_value = defer
        act, logp, val, mu, sigma = ac.act(x, states)
        ac.join()
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (act, logp, val, mu)])
    for a, b in zip(outs[0][:2] + outs[0][3:], outs[1][:2] + outs[1][3:]):
        assert (a - b).abs().max().item() <= 1e-5
    assert (outs[0][2] - outs[1][2]).abs().max().item() <= 1e-5 * (1.0 + outs[0][2].abs().max().item())

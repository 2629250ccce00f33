"""tests/step_physics_check.py on the HIP build (run with -m gpu on an MI355X): the step kernel's own read-back state against
first principles, under every launch layout of csrc/step_kernels.hip launch_step.  The fast-math build cannot be compared bit
for bit with the CPU build, and the teacher-forced gates of tests/parity.py are statistical; these checks need no reference
trajectory, so a sparse error -- one lane of a rare branch, one env of a 16-env block, one ant index of a reaction sum -- has
nowhere to hide.  A failing exact check (bits under a symmetry of the launch) is a kernel bug by construction.

Layouts (TenAnt): the default packed <192,4> blocks with a partial last one; MMS_PACKING=0, the one-wave DPP reductions;
MMS_STEP_BLOCK16=1, the <768,16> blocks (16 envs: one full block; 37: two and a partial one); the DR instantiation with the
nominal dr_params the engine starts with (the same physical model, so the same gates); num_agents 2 / 14 (one wave per env), 15 /
33 (the 512-thread shape).  OneAnt and MultiAntCircle packed and unpacked, MultiIngenuity with a partial and with a second block.
The head-fused instantiation takes its actions from the policy and is pinned bit for bit to the unfused kernel elsewhere.

Every analytic residual and every measured gate (with the fp32 oracle's value beside it) lands in the parity margins file
(parity.record, written at the end of the session) under gpu/step_physics/<layout>/..."""
import numpy as np
import pytest

import parity
import step_physics_check as spc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product path has no CPU fallback")
    return torch


class Layout:
    def __init__(self, name, env=None, dr=False, num_agents=None, ns=(6, 37), n=6):
        self.name, self.env, self.dr, self.num_agents, self.ns, self.n = name, env or {}, dr, num_agents, ns, n

    def __repr__(self):
        return self.name

    def make(self, monkeypatch, **env):
        """make(task, **kw) -> Engine on device 0 in this layout (the switches are read by mms_create and by every launch: they stay set
        for the rest of the test)."""
        switches = dict(self.env, **env)

        def make(task, **kw):
            from massive_marl_benchmark_amd.engine import Engine
            for k in ("MMS_PACKING", "MMS_STEP_BLOCK16"):
                monkeypatch.delenv(k, raising=False)
            for k, v in switches.items():
                monkeypatch.setenv(k, v)
            eng = Engine(task, device=0, **kw)
            if self.dr:
                dr = eng.tensor("dr_params")
                assert float(dr[:, :17].min()) == 1.0 == float(dr[:, :17].max()) and float(dr[:, 17:].abs().max()) == 0.0
                eng.set_dr(True)
            return eng
        return make

    def tag(self):
        return "gpu/step_physics/" + self.name


TEN = [Layout("packed"), Layout("unpacked", {"MMS_PACKING": "0"}), Layout("block16", {"MMS_STEP_BLOCK16": "1"}, ns=(16, 37), n=16),
       Layout("block16_n37", {"MMS_STEP_BLOCK16": "1"}, ns=(), n=37), Layout("dr", dr=True),
       Layout("dr_block16", {"MMS_STEP_BLOCK16": "1"}, dr=True, ns=(37,), n=37)]
AGENTS = [Layout("agents%d" % a, num_agents=a, ns=(6,), n=5) for a in (2, 14, 15, 33)]
TEN_ALL = TEN + AGENTS
ONE = [Layout("packed"), Layout("unpacked", {"MMS_PACKING": "0"}, n=5)]
HELI = [Layout("n6", n=6), Layout("n70", n=70)]
ids = lambda layouts: [l.name for l in layouts]


def record(layout, what, res):
    parity.record("%s/%s" % (layout.tag(), what), **res)


def pairs_for(a):
    """Ant pairs to exchange: far apart, neighbours across a wave boundary (thread 40 e + 4 k of the packed layouts: ants 5 | 6 of
    env 1; thread 4 k of the one-env 512-thread shape: ants 15 | 16), first and last."""
    return {2: [(0, 1)], 33: [(2, 7), (15, 16), (0, 32)]}.get(a, [(2, 7), (5, 6), (0, a - 1)])


# ---- exact: bits under symmetries of the launch ---------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [l for l in TEN_ALL if l.ns], ids=ids([l for l in TEN_ALL if l.ns]))
def test_identical_envs_give_identical_bits(torch_cuda, layout, monkeypatch):
    for n in layout.ns:
        spc.check_identical_envs(layout.make(monkeypatch), n, num_agents=layout.num_agents)
    spc.check_identical_envs(layout.make(monkeypatch), layout.ns[0], spacing=0, num_agents=layout.num_agents)


@pytest.mark.parametrize("contact", [False, True], ids=["free", "contact"])
@pytest.mark.parametrize("layout", [l for l in TEN_ALL if l.ns], ids=ids([l for l in TEN_ALL if l.ns]))
def test_env_isolation(torch_cuda, layout, contact, monkeypatch):
    """(env 2 sits inside the first block of every layout; env 20 in block 5 of <192,4> and in the second block of <768,16>)"""
    for n in layout.ns:
        spc.check_env_isolation(layout.make(monkeypatch), n, (2, 20) if n > 20 else (2,), contact=contact, num_agents=layout.num_agents)


@pytest.mark.parametrize("layout", [l for l in TEN_ALL if l.ns], ids=ids([l for l in TEN_ALL if l.ns]))
def test_ant_relabelling(torch_cuda, layout, monkeypatch):
    for pair in pairs_for(layout.num_agents or 10):
        spc.check_ant_relabelling(layout.make(monkeypatch), pair, num_agents=layout.num_agents)


@pytest.mark.parametrize("box_mu", [None, 0.5], ids=["mu_default", "mu0.5"])
@pytest.mark.parametrize("n", [16, 37])
def test_block_layouts_agree_under_contact(torch_cuda, n, box_mu, monkeypatch):
    """test_sixteen_env_block_layout's pair (MMS_STEP_BLOCK16=0 / 1, same lane code and same reduction orders) free-runs from a
    reset, where no ant reaches the box; here every ant starts pressed against it."""
    packed = Layout("packed")
    spc.check_layouts_agree_under_contact([packed.make(monkeypatch, MMS_STEP_BLOCK16="0"), packed.make(monkeypatch, MMS_STEP_BLOCK16="1")],
                                          n, box_mu=box_mu)


# ---- analytic -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_free_fall(torch_cuda, layout, monkeypatch):
    record(layout, "free_fall", spc.check_free_fall(layout.make(monkeypatch), "TenAnt", n=layout.n, num_agents=layout.num_agents))


@pytest.mark.parametrize("layout", ONE, ids=ids(ONE))
@pytest.mark.parametrize("task", ["OneAnt", "MultiAntCircle"])
def test_free_fall_small_tasks(torch_cuda, task, layout, monkeypatch):
    record(layout, "free_fall/" + task, spc.check_free_fall(layout.make(monkeypatch), task, n=layout.n))


@pytest.mark.parametrize("layout", HELI, ids=ids(HELI))
def test_free_fall_and_hover_ingenuity(torch_cuda, layout, monkeypatch):
    record(layout, "free_fall/MultiIngenuity", spc.check_free_fall(layout.make(monkeypatch), "MultiIngenuity", n=layout.n))
    record(layout, "hover", spc.check_hover(layout.make(monkeypatch), n=layout.n))


@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_torque_sign_and_size(torch_cuda, layout, monkeypatch):
    lo_hi = spc.check_torque(layout.make(monkeypatch), num_agents=layout.num_agents)
    record(layout, "torque", {"dqd_over_dt_min": min(a for a, _ in lo_hi), "dqd_over_dt_max": max(b for _, b in lo_hi)})


@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_energy_never_rises_and_dissipates(torch_cuda, layout, monkeypatch):
    record(layout, "energy", spc.check_energy(layout.make(monkeypatch), "TenAnt", n=layout.n, num_agents=layout.num_agents))


@pytest.mark.parametrize("layout", ONE, ids=ids(ONE))
@pytest.mark.parametrize("task", ["OneAnt", "MultiAntCircle"])
def test_energy_small_tasks(torch_cuda, task, layout, monkeypatch):
    record(layout, "energy/" + task, spc.check_energy(layout.make(monkeypatch), task, n=layout.n))


@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_momentum_error_is_first_order(torch_cuda, layout, monkeypatch):
    res = spc.check_first_order(layout.make(monkeypatch), num_agents=layout.num_agents)
    record(layout, "first_order", {"drift": res["drift"], "ratio_min": res["ratios"][0], "ratio_max": res["ratios"][1]})


@pytest.mark.parametrize("rule", ["average", "min"])
@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_action_reaction_with_the_box(torch_cuda, layout, rule, monkeypatch):
    spc.check_action_reaction(layout.make(monkeypatch), rule, n=layout.n, num_agents=layout.num_agents, tag=layout.tag())


@pytest.mark.parametrize("rule", ["average", "min"])
@pytest.mark.parametrize("layout", ONE, ids=ids(ONE))
def test_action_reaction_one_ant(torch_cuda, layout, rule, monkeypatch):
    spc.check_action_reaction(layout.make(monkeypatch), rule, task="OneAnt", n=layout.n, tag=layout.tag() + "/OneAnt")


@pytest.mark.parametrize("layout", TEN, ids=ids(TEN))
def test_sliding_ant_drags_the_box_only_with_friction(torch_cuda, layout, monkeypatch):
    vy = spc.check_sliding_ant_drags_the_box(layout.make(monkeypatch))
    record(layout, "sliding_ant", {"box_vy_min_rule": float(np.abs(vy["min"]).max()), "box_vy_average_rule": float(vy["average"].min())})


@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_joint_limits_under_full_torque(torch_cuda, layout, monkeypatch):
    spc.check_joint_limits(layout.make(monkeypatch), num_agents=layout.num_agents, tag=layout.tag())


@pytest.mark.parametrize("layout", TEN_ALL, ids=ids(TEN_ALL))
def test_rest_on_the_ground(torch_cuda, layout, monkeypatch):
    record(layout, "rest", spc.check_rest(layout.make(monkeypatch), "TenAnt", n=layout.n, num_agents=layout.num_agents))


@pytest.mark.parametrize("layout", ONE, ids=ids(ONE))
@pytest.mark.parametrize("task", ["OneAnt", "MultiAntCircle"])
def test_rest_small_tasks(torch_cuda, task, layout, monkeypatch):
    record(layout, "rest/" + task, spc.check_rest(layout.make(monkeypatch), task, n=layout.n))

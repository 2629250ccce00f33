"""tests/step_physics_check.py on the CPU build (Engine(device="cpu"): the step kernel's lane code compiled for the host).  This
proves the checks themselves where no GPU is needed; tests/test_step_physics_gpu.py runs the same list on the HIP build under
every launch layout.  The last block shows, per analytic check, that a wrong model misses its gate."""
import pytest

import step_physics_check as spc


def make(task, **kw):
    from massive_marl_benchmark_amd.engine import Engine
    return Engine(task, device="cpu", **kw)


@pytest.mark.parametrize("n,spacing", [(6, None), (37, None), (6, 0)])
def test_identical_envs_give_identical_bits(n, spacing):
    spc.check_identical_envs(make, n, spacing=spacing)


@pytest.mark.parametrize("n,perturbed", [(6, (2,)), (37, (2, 20))])
@pytest.mark.parametrize("contact", [False, True])
def test_env_isolation(n, perturbed, contact):
    spc.check_env_isolation(make, n, perturbed, contact=contact)


@pytest.mark.parametrize("pair", [(2, 7), (5, 6)])
def test_ant_relabelling(pair):
    spc.check_ant_relabelling(make, pair)


@pytest.mark.parametrize("box_mu", [None, 0.5])
def test_two_runs_agree_under_contact(box_mu):
    spc.check_layouts_agree_under_contact([make, make], 16, box_mu=box_mu)


@pytest.mark.parametrize("task", ["TenAnt", "OneAnt", "MultiAntCircle", "MultiIngenuity"])
def test_free_fall(task):
    spc.check_free_fall(make, task)


def test_hover():
    spc.check_hover(make)


def test_torque_sign_and_size():
    spc.check_torque(make)


@pytest.mark.parametrize("task", ["TenAnt", "OneAnt", "MultiAntCircle"])
def test_energy_never_rises_and_dissipates(task):
    spc.check_energy(make, task)


def test_momentum_error_is_first_order():
    spc.check_first_order(make)


@pytest.mark.parametrize("rule", ["average", "min"])
def test_action_reaction_with_the_box(rule):
    spc.check_action_reaction(make, rule, tag="cpu/step_physics")


def test_sliding_ant_drags_the_box_only_with_friction():
    spc.check_sliding_ant_drags_the_box(make)


def test_joint_limits_under_full_torque():
    spc.check_joint_limits(make, tag="cpu/step_physics")


@pytest.mark.parametrize("task", ["TenAnt", "OneAnt", "MultiAntCircle"])
def test_rest_on_the_ground(task):
    spc.check_rest(make, task)


# ---- the checks can fail: a wrong model (through the configuration, not a mutated kernel) misses each gate --------------------

def test_free_fall_gate_sees_one_percent_of_gravity():
    with pytest.raises(AssertionError):
        spc.check_free_fall(make, "TenAnt", g_formula=1.01 * 9.81)
    with pytest.raises(AssertionError):
        spc.check_free_fall(make, "MultiIngenuity", g_formula=1.01 * 3.721)


def test_hover_gate_sees_one_percent_of_thrust():
    with pytest.raises(AssertionError):
        spc.check_hover(make, g_thrust=1.01 * 3.721)


def test_torque_gate_sees_a_wrong_power_scale():
    with pytest.raises(AssertionError):
        spc.check_torque(make, power_scale=3.0, tau_formula=1.0)


def test_energy_gate_sees_actuation():
    with pytest.raises(AssertionError):
        spc.check_energy(make, "TenAnt", action=0.3)


def test_first_order_gate_sees_two_runs_of_the_same_step():
    with pytest.raises(AssertionError):
        spc.check_first_order(make, dts=(spc.DT, spc.DT, spc.DT / 2))


def test_conservation_gate_sees_two_percent_of_box_mass():
    with pytest.raises(AssertionError):
        spc.check_action_reaction(make, "average", box_mass_scale=1.02)


def test_isolation_gate_sees_the_perturbed_env():
    with pytest.raises(AssertionError, match="env 2 changed"):
        spc.check_env_isolation(make, 6, (2,), claim_untouched=range(6))

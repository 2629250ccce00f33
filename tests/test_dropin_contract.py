"""The drop-in boundary on the CPU build: the learners' loops (dropin_check.py, restated from ppo.py:126-139, ddpg.py:151-160,
marl/maddpg/runner.py:107-150, marl/runner.py:128-151) over VecTaskPython / MultiVecTaskPython with this build's ActorCritic,
RolloutStorage and ReplayBuffer store the observation the policy ACTED ON -- every comparison exact.  Shapes: OneAnt 64 envs
(obs 60, act 8), MultiIngenuity 64 envs (obs 52, act 24), TenAnt 16 envs x 10 agents; 8 steps with episodeLength 4, so every env
is reset inside the window.

Before the wrappers returned tensors of their own (they returned views of engine memory that the next step overwrites) these
failed (nine of these eleven; the noise-lambda and inserted-at-once cases passed): on-policy max |observations[0] - seen[0]| = 5.0
(the clamp) with observations[t] == seen[t + 1] exactly; every off-policy transition (s', a, r, s'), max |stored - seen| 0.26 - 0.61;
the multi-agent rows held across a step off by 7.0 (the clamp) and equal to the step's result; tensors returned by reset() / step()
changed by up to 10 (single-agent) and 12 (obs_all / state_all; reward_all by 25) after two more steps and a reset."""
import pytest
import torch

import dropin_check as dc


@pytest.fixture
def env(request):
    e = dc.make_env(*request.param, "cpu")
    yield e
    e.task.engine.close()


def _id(p):
    return "-".join(str(x) for x in p)


@pytest.mark.parametrize("env", [("OneAnt", 64)], indirect=True, ids=_id)
def test_on_policy_loop_stores_what_act_saw(env):
    ac, storage = dc.ppo_parts(env)
    dc.check_on_policy(env, ac, storage)


def test_on_policy_loop_with_observation_noise():
    """The 'observations' noise lambda (base_task.py:141-143): obs_buf_clipped is then a torch.clamp result; the same contract."""
    env = dc.make_env("OneAnt", 64, "cpu", obs_noise=True)
    ac, storage = dc.ppo_parts(env)
    dc.check_on_policy(env, ac, storage)
    assert not torch.equal(env.task.obs_buf, env.task.engine.tensor("obs"))       # the noise branch ran
    env.task.engine.close()


@pytest.mark.parametrize("env", [("OneAnt", 64)], indirect=True, ids=_id)
def test_bound_on_policy_loop_through_the_wrapper(env):
    """INTEGRATION.md section 1's bound loop -- bind_rollout, bind_obs_out on the next slot, bind_rollout_out on this one -- around
    the unchanged PPO loop, through the wrapper: the same contract.  (act's five outputs are found in place by add_transitions; the
    observation, reward and done rows are copied, the wrapper's tensors not being the slots -- the document says so.)"""
    ac, storage = dc.ppo_parts(env)
    dc.check_on_policy(env, ac, storage, bound=True)


@pytest.mark.parametrize("algo", ["ddpg", "td3", "sac"])
def test_off_policy_loop_stores_transitions(algo):
    env = dc.make_env("MultiIngenuity", 64, "cpu")
    act, buf = dc.off_policy_parts(env, algo)
    dc.check_off_policy(env, act, buf)
    env.task.engine.close()


@pytest.mark.parametrize("env", [("TenAntMulti", 16)], indirect=True, ids=_id)
def test_multi_agent_held_across_the_step(env):
    dc.check_marl(env, held=True)


@pytest.mark.parametrize("env", [("TenAntMulti", 16)], indirect=True, ids=_id)
def test_multi_agent_inserted_at_once(env):
    dc.check_marl(env, held=False)


@pytest.mark.parametrize("env", [("OneAnt", 64), ("MultiIngenuity", 64)], indirect=True, ids=_id)
def test_vec_task_returns_fresh_observations(env):
    """VecTaskPython: the observation of step() / reset() has storage of its own.  rew / done follow vec_task.py:131: `.to(rl_device)`
    of the task's buffers -- on the engine's own device an ALIAS of engine memory (allowed, as in the reference), holding the step's
    values when returned."""
    rew_alias, done_alias, rew_now, done_now = dc.check_wrapper_freshness(env, multi=False)
    assert rew_now and done_now
    assert rew_alias and done_alias          # .to() on the same device copies nothing: the rule above is what the wrapper does


@pytest.mark.parametrize("env", [("TenAntMulti", 16)], indirect=True, ids=_id)
def test_multi_vec_task_returns_fresh_tensors(env):
    """MultiVecTaskPython: obs, share_obs (state_all), rewards and dones all have storage of their own, as the reference's
    torch.stack results have (multi_vec_task.py:138-141); state_all may be a stride-0 expansion of one fresh [N, 388] copy."""
    dc.check_wrapper_freshness(env, multi=True)

"""What the three off-policy learners (sac/sac.py, ddpg/ddpg.py, td3/td3.py) share: the reference's training loop (sac.py:128-221;
ddpg.py / td3.py:117-204 are the same loop but for the three hooks below), its log, its checkpoint methods, the minibatch gather and
the device-side form of what clip_grad_norm_ leaves in the stored gradients.  A learner supplies `actor_critic`, `storage`, `vec_env`,
`update()` and the attributes the reference's constructor sets.  Where the env exposes this package's engine and nothing rewrites its
observations, `run` binds the engine's observation output to the ring row the next `add_transitions` fills (ReplayBuffer.slot()), so
the step kernel writes next_observations in place.  tensorboard is optional."""
import os
import statistics
import time
from collections import deque

import torch

try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:                                       # tensorboard is not installed: nothing is logged
    class SummaryWriter:
        def __init__(self, *args, **kwargs):
            pass

        def __getattr__(self, name):
            return lambda *args, **kwargs: None


class OffPolicyLearner:
    def test(self, path):
        self.actor_critic.load_state_dict(torch.load(path))
        self.actor_critic.eval()

    def load(self, path):
        self.actor_critic.load_state_dict(torch.load(path))
        self.current_learning_iteration = int(path.split("_")[-1].split(".")[0])
        self.actor_critic.train()

    def save(self, path):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        torch.save(self.actor_critic.state_dict(), path)

    # ---- the loop ------------------------------------------------------------------------------------------------------------------

    def _engine(self):
        """This package's engine behind the env, where its observation output is what `step` returns; None otherwise."""
        task = getattr(self.vec_env, "task", None)
        engine = getattr(task, "engine", None)
        if engine is None or not hasattr(engine, "bind_obs_out") or not hasattr(self.storage, "slot"):
            return None
        if getattr(task, "dr_randomizations", None) and task.dr_randomizations.get("observations"):
            return None                     # (the task replaces its observations by torch results: the bound row would not be them)
        return engine

    # What the loops of the three off-policy learners differ in (sac.py:128-221 against ddpg.py / td3.py:117-204): DDPG and TD3 share `run`
    def _act(self, obs, explore):
        return self.actor_critic.act(obs) if explore else self.actor_critic.act(obs, deterministic=True)

    def _warm_up_over(self):
        return self.storage.step >= self.batch_size

    scales_rewards = True                   # `rews *= self.reward_scale` (sac.py:169)

    def run(self, num_learning_iterations, log_interval=1):
        """The main loop of training (sac.py:128-221).  log_interval: how often the model is saved."""
        current_obs = self.vec_env.reset()
        current_states = self.vec_env.get_state()
        if self.is_testing:
            while True:
                with torch.no_grad():
                    if self.apply_reset:
                        current_obs = self.vec_env.reset()
                    actions = self._act(current_obs, False)
                    next_obs, rews, dones, infos = self.vec_env.step(actions)
                    current_obs.copy_(next_obs)
        rewbuffer = deque(maxlen=100)
        lenbuffer = deque(maxlen=100)
        cur_reward_sum = torch.zeros(self.vec_env.num_envs, dtype=torch.float, device=self.device)
        cur_episode_length = torch.zeros(self.vec_env.num_envs, dtype=torch.float, device=self.device)
        reward_sum = []
        episode_length = []
        engine = self._engine()
        try:
            for it in range(self.current_learning_iteration, num_learning_iterations):
                start = time.time()
                ep_infos = []
                for _ in range(self.num_transitions_per_env):
                    if self.apply_reset:
                        current_obs = self.vec_env.reset()
                        current_states = self.vec_env.get_state()
                    actions = self._act(current_obs, True)
                    row = None
                    if engine is not None:          # the step kernel writes next_observations where add_transitions would copy them
                        row = self.storage.next_observations[self.storage.slot()]
                        engine.bind_obs_out(row)
                    next_obs, rews, dones, infos = self.vec_env.step(actions)
                    if self.scales_rewards:
                        rews *= self.reward_scale
                    next_states = self.vec_env.get_state()
                    self.storage.add_transitions(current_obs, current_states, actions, rews, next_obs if row is None else row, dones)
                    current_obs.copy_(next_obs)
                    current_states.copy_(next_states)
                    ep_infos.append(infos)

                    if self.print_log:
                        cur_reward_sum[:] += rews
                        cur_episode_length[:] += 1
                        new_ids = (dones > 0).nonzero(as_tuple=False)
                        reward_sum.extend(cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
                        episode_length.extend(cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
                        cur_reward_sum[new_ids] = 0
                        cur_episode_length[new_ids] = 0

                    if self._warm_up_over():
                        self.warm_up = False
                    if self.warm_up == False:       # noqa: E712
                        mean_value_loss, mean_surrogate_loss = self.update()

                if self.print_log:
                    rewbuffer.extend(reward_sum)
                    lenbuffer.extend(episode_length)
                stop = time.time()
                collection_time = stop - start
                mean_trajectory_length, mean_reward = self.storage.get_statistics()
                start = stop
                if self.warm_up == False:           # noqa: E712
                    stop = time.time()
                    learn_time = stop - start
                    if self.print_log:
                        self.log(locals())
                    if it % log_interval == 0:
                        self.save(os.path.join(self.log_dir, 'model_{}.pt'.format(it)))
                    ep_infos.clear()
        finally:
            if engine is not None:
                engine.bind_obs_out(None)
        self.save(os.path.join(self.log_dir, 'model_{}.pt'.format(num_learning_iterations)))

    def log(self, locs, width=80, pad=35):
        """Print and record the iteration's figures (sac.py:223-291)."""
        self.tot_timesteps += self.num_transitions_per_env * self.vec_env.num_envs
        iteration_time = locs['collection_time'] + locs['learn_time']
        self.tot_time += iteration_time
        it = locs['it']

        ep_string = ''
        if locs['ep_infos']:
            for key in locs['ep_infos'][0]:
                infotensor = torch.tensor([], device=self.device)
                for ep_info in locs['ep_infos']:
                    infotensor = torch.cat((infotensor, ep_info[key].to(self.device)))
                value = torch.mean(infotensor)
                self.writer.add_scalar('Episode/' + key, value, it)
                ep_string += "%*s %.4f\n" % (pad, 'Mean episode %s:' % key, value)

        fps = int(self.num_transitions_per_env * self.vec_env.num_envs / iteration_time)
        self.writer.add_scalar('Loss/value_function', locs['mean_value_loss'], it)
        self.writer.add_scalar('Loss/surrogate', locs['mean_surrogate_loss'], it)
        episodes = len(locs['rewbuffer']) > 0
        if episodes:
            self.writer.add_scalar('Train/mean_reward', statistics.mean(locs['rewbuffer']), it)
            self.writer.add_scalar('Train/FPS', fps, it)
            self.writer.add_scalar('Train/mean_episode_length', statistics.mean(locs['lenbuffer']), it)
            self.writer.add_scalar('Train/mean_reward/time', statistics.mean(locs['rewbuffer']), self.tot_time)
            self.writer.add_scalar('Train/mean_episode_length/time', statistics.mean(locs['lenbuffer']), self.tot_time)
        self.writer.add_scalar('Train2/mean_reward/step', locs['mean_reward'], it)
        self.writer.add_scalar('Train2/mean_episode_length/episode', locs['mean_trajectory_length'], it)

        title = " \033[1m Learning iteration %d/%d \033[0m " % (it, locs['num_learning_iterations'])
        lines = ['#' * width, title.center(width, ' '), '',
                 "%*s %.0f steps/s (collection: %.3fs, learning %.3fs)" % (pad, 'Computation:', fps, locs['collection_time'], locs['learn_time']),
                 "%*s %.4f" % (pad, 'Value function loss:', locs['mean_value_loss']),
                 "%*s %.4f" % (pad, 'Surrogate loss:', locs['mean_surrogate_loss'])]
        if episodes:
            lines += ["%*s %.2f" % (pad, 'Mean reward:', statistics.mean(locs['rewbuffer'])),
                      "%*s %.2f" % (pad, 'Mean episode length:', statistics.mean(locs['lenbuffer']))]
        lines += ["%*s %.2f" % (pad, 'Mean reward/step:', locs['mean_reward']),
                  "%*s %.2f" % (pad, 'Mean episode length/episode:', locs['mean_trajectory_length'])]
        tail = ['-' * width, "%*s %d" % (pad, 'Total timesteps:', self.tot_timesteps), "%*s %.2fs" % (pad, 'Iteration time:', iteration_time),
                "%*s %.2fs" % (pad, 'Total time:', self.tot_time),
                "%*s %.1fs" % (pad, 'ETA:', self.tot_time / (it + 1) * (locs['num_learning_iterations'] - it))]
        print("\n".join(lines) + "\n" + ep_string + "\n".join(tail) + "\n")

    # ---- pieces of the update --------------------------------------------------------------------------------------------------

    def _gather(self, indices):
        """The minibatch of ring rows `indices` (sac.py:309-323)."""
        s = self.storage
        return {'obs': s.observations[indices], 'act': s.actions[indices], 'r': s.rewards[indices], 'obs2': s.next_observations[indices],
                'done': s.dones[indices]}

    def _rescale(self, params, norm):
        """What clip_grad_norm_ leaves in the stored gradients, from clip_and_step's norm, on the device."""
        grads = [p.grad for p in params if p.grad is not None]
        if grads and self.max_grad_norm is not None and self.max_grad_norm > 0:
            torch._foreach_mul_(grads, torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0))

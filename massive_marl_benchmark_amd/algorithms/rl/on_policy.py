"""What the two on-policy learners (ppo/ppo.py, trpo/trpo.py) share, which in the reference is everything before `update`
(agents/algorithms/rl/ppo/ppo.py:22-241, trpo/trpo.py:30-256: the two files differ there in the constructor's keys and in one tensorboard
line): the space checks and the attributes every constructor sets, the training loop, its log and its checkpoint methods.  A learner
supplies its `learn` keys, its optimizer and `update()`.  Shaped as off_policy.OffPolicyLearner is; tensorboard is optional, as there."""
import copy
import os
import statistics
import time
from collections import deque

import torch

from ...spaces import Space
from .off_policy import SummaryWriter


class OnPolicyLearner:
    logs_fps = False                        # trpo.py:214 writes 'Train/FPS'; ppo.py does not

    def _init_common(self, vec_env, cfg_train, device, sampler, log_dir, is_testing, print_log, apply_reset, asymmetric, ActorCritic, RolloutStorage,
                     **module_kwargs):
        """ppo.py:34-62 / trpo.py:42-68: the spaces, the keys both files read, the module and the storage.  Returns the `learn` dict."""
        for name in ("observation_space", "state_space", "action_space"):
            if not isinstance(getattr(vec_env, name), Space):
                raise TypeError("vec_env.%s must be a gym Space" % name)
        self.observation_space = vec_env.observation_space
        self.action_space = vec_env.action_space
        self.state_space = vec_env.state_space
        self.cfg_train = copy.deepcopy(cfg_train)
        learn_cfg = self.cfg_train["learn"]
        self.device = device
        self.asymmetric = asymmetric

        self.schedule = learn_cfg.get("schedule", "fixed")
        self.step_size = learn_cfg["optim_stepsize"]
        self.init_noise_std = learn_cfg.get("init_noise_std", 0.3)
        self.model_cfg = self.cfg_train["policy"]
        self.num_transitions_per_env = learn_cfg["nsteps"]
        self.learning_rate = learn_cfg["optim_stepsize"]

        self.vec_env = vec_env
        self.actor_critic = ActorCritic(self.observation_space.shape, self.state_space.shape, self.action_space.shape, self.init_noise_std,
                                        self.model_cfg, asymmetric=asymmetric, **module_kwargs)
        self.actor_critic.to(self.device)
        self.storage = RolloutStorage(self.vec_env.num_envs, self.num_transitions_per_env, self.observation_space.shape, self.state_space.shape,
                                      self.action_space.shape, self.device, sampler)
        return learn_cfg

    def _init_log(self, log_dir, print_log, is_testing, apply_reset):
        self.log_dir = log_dir
        self.print_log = print_log
        self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
        self.tot_timesteps = 0
        self.tot_time = 0
        self.is_testing = is_testing
        self.current_learning_iteration = 0
        self.apply_reset = apply_reset

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------------

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

    def run(self, num_learning_iterations, log_interval=1):
        """The main loop of training (ppo.py:99-177).  log_interval: how often the model is saved."""
        current_obs = self.vec_env.reset()
        current_states = self.vec_env.get_state()
        if self.is_testing:
            while True:
                with torch.no_grad():
                    if self.apply_reset:
                        current_obs = self.vec_env.reset()
                    actions = self.actor_critic.act_inference(current_obs)
                    next_obs, rews, dones, infos = self.vec_env.step(actions)
                    current_obs.copy_(next_obs)
        rewbuffer = deque(maxlen=100)
        lenbuffer = deque(maxlen=100)
        cur_reward_sum = torch.zeros(self.vec_env.num_envs, dtype=torch.float, device=self.device)
        cur_episode_length = torch.zeros(self.vec_env.num_envs, dtype=torch.float, device=self.device)
        reward_sum = []
        episode_length = []
        for it in range(self.current_learning_iteration, num_learning_iterations):
            start = time.time()
            ep_infos = []
            for _ in range(self.num_transitions_per_env):
                if self.apply_reset:
                    current_obs = self.vec_env.reset()
                    current_states = self.vec_env.get_state()
                actions, actions_log_prob, values, mu, sigma = self.actor_critic.act(current_obs, current_states)
                next_obs, rews, dones, infos = self.vec_env.step(actions)
                next_states = self.vec_env.get_state()
                self.storage.add_transitions(current_obs, current_states, actions, rews, dones, values, actions_log_prob, mu, sigma)
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

            if self.print_log:
                rewbuffer.extend(reward_sum)
                lenbuffer.extend(episode_length)

            _, _, last_values, _, _ = self.actor_critic.act(current_obs, current_states)
            stop = time.time()
            collection_time = stop - start
            mean_trajectory_length, mean_reward = self.storage.get_statistics()

            start = stop
            self.storage.compute_returns(last_values, self.gamma, self.lam)
            mean_value_loss, mean_surrogate_loss = self.update()
            self.storage.clear()
            stop = time.time()
            learn_time = stop - start
            if self.print_log:
                self.log(locals())
            if it % log_interval == 0:
                self.save(os.path.join(self.log_dir, 'model_{}.pt'.format(it)))
            ep_infos.clear()
        self.save(os.path.join(self.log_dir, 'model_{}.pt'.format(num_learning_iterations)))

    def log(self, locs, width=80, pad=35):
        """Print and record the iteration's figures (ppo.py:179-241)."""
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
        mean_std = self.actor_critic.log_std.exp().mean()

        fps = int(self.num_transitions_per_env * self.vec_env.num_envs / iteration_time)
        self.writer.add_scalar('Loss/value_function', locs['mean_value_loss'], it)
        self.writer.add_scalar('Loss/surrogate', locs['mean_surrogate_loss'], it)
        self.writer.add_scalar('Policy/mean_noise_std', mean_std.item(), it)
        episodes = len(locs['rewbuffer']) > 0
        if episodes:
            self.writer.add_scalar('Train/mean_reward', statistics.mean(locs['rewbuffer']), it)
            if self.logs_fps:
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
                 "%*s %.4f" % (pad, 'Surrogate loss:', locs['mean_surrogate_loss']),
                 "%*s %.2f" % (pad, 'Mean action noise std:', mean_std.item())]
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
        """The minibatch's rows of the rollout's flat views (ppo.py:253-264, trpo.py:268-279)."""
        s = self.storage
        A = s.actions.size(-1)
        return {'obs': s.observations.view(-1, *s.observations.size()[2:])[indices],
                'states': s.states.view(-1, *s.states.size()[2:])[indices] if self.asymmetric else None,
                'actions': s.actions.view(-1, A)[indices], 'target_values': s.values.view(-1, 1)[indices], 'returns': s.returns.view(-1, 1)[indices],
                'old_logp': s.actions_log_prob.view(-1, 1)[indices], 'adv': s.advantages.view(-1, 1)[indices], 'old_mu': s.mu.view(-1, A)[indices],
                'old_sigma': s.sigma.view(-1, A)[indices]}

    def _value_loss(self, value_batch, b):
        """ppo.py:293-300, trpo.py:325-332."""
        if self.use_clipped_value_loss:
            value_clipped = b['target_values'] + (value_batch - b['target_values']).clamp(-self.clip_param, self.clip_param)
            value_losses = (value_batch - b['returns']).pow(2)
            value_losses_clipped = (value_clipped - b['returns']).pow(2)
            return torch.max(value_losses, value_losses_clipped).mean()
        return (b['returns'] - value_batch).pow(2).mean()

    @staticmethod
    def _kl(sigma_batch, mu_batch, b):
        """ppo.py:273-274, trpo.py:294-297: the per-row KL of the old policy from the new one."""
        return torch.sum(sigma_batch - b['old_sigma'] + (torch.square(b['old_sigma'].exp()) + torch.square(b['old_mu'] - mu_batch)) /
                         (2.0 * torch.square(sigma_batch.exp())) - 0.5, axis=-1)

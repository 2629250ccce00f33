"""Runner of MADDPG (agents/algorithms/marl/maddpg/runner.py): `Runner(vec_env, config, model_dir="")` with the reference's methods
`run`, `collect`, `insert`, `train`, `save`, `restore`, `eval`.

The reference's `run` cannot execute (its train.py:25 says so).  Repairs, limited to what cannot execute:
  * `share_obs[0]` / `obs[0]` for `states[0]` / `observations[0]` (the buffer's fields);
  * `collect(step)` read `buffer.obs[step]`, a ring row indexed by the EPISODE step (an index error once episode_length exceeds
    replay_size, stale rows otherwise): the current observation is staged into the ring row the next `add_transitions` fills
    (`slot()`) and the actors read it there;
  * `eval` takes the single return of `act`; `get_values` calls `critic.get_value` (module.py);
  * the first, shadowed `log_train` (np.mean on a device tensor) is gone: the second definition is the one Python keeps.
What changes besides: the per-env Python loop over `dones_env` (runner.py:138-141; one host synchronisation per env and step) is
masked tensor arithmetic with the same mean of finished episodes' rewards; all agents act through `MADDPG.act_all`, whose head kernel
writes every action into its ring row and the joint action into ONE joint ring shared by all buffers (`insert` finds those rows in
place); tensorboard is optional (a writer that does nothing when it is not installed)."""
import os
import time

import torch

from .module import MADDPG as TrainAlgo
from .module import MADDPG_policy as Policy
from .storage import ReplayBuffer

try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:                                       # tensorboard is not installed: nothing is logged
    class SummaryWriter:
        def __init__(self, *args, **kwargs):
            pass

        def __getattr__(self, name):
            return lambda *args, **kwargs: None


class Runner:
    def __init__(self, vec_env, config, model_dir=""):
        self.envs = vec_env
        self.eval_envs = vec_env
        cfg = vec_env.task.cfg
        self.env_name = cfg["env"].get("env_name", getattr(vec_env.task, "TASK_NAME", "env"))
        self.algorithm_name = config["algorithm_name"]
        self.experiment_name = config["experiment_name"]
        self.num_env_steps = config["num_env_steps"]
        self.episode_length = config["episode_length"]
        self.n_rollout_threads = config["n_rollout_threads"]
        self.n_eval_rollout_threads = config["n_eval_rollout_threads"]
        self.hidden_size = config["hidden_size"]
        self.use_render = config["use_render"]
        self.save_interval = config["save_interval"]
        self.use_eval = config["use_eval"]
        self.eval_interval = config["eval_interval"]
        self.eval_episodes = config["eval_episodes"]
        self.log_interval = config["log_interval"]
        self.seed = cfg.get("seed", 0)
        self.model_dir = model_dir
        self.batch_size = config["batch_size"]
        self.warm_up = True
        self.num_agents = self.envs.num_agents
        self.device = self.envs.rl_device
        self.run_dir = config["run_dir"]
        self.log_dir = str(self.run_dir + '/' + self.env_name + '/' + self.algorithm_name + '/logs_seed{}'.format(self.seed))
        os.makedirs(self.log_dir, exist_ok=True)
        self.writter = SummaryWriter(self.log_dir)
        self.save_dir = str(self.run_dir + '/' + self.env_name + '/' + self.algorithm_name + '/models_seed{}'.format(self.seed))
        os.makedirs(self.save_dir, exist_ok=True)

        self.policy = [Policy(config, self.envs.observation_space[a], self.envs.share_observation_space[a], self.envs.action_space[a],
                              self.envs.action_space, device=self.device) for a in range(self.num_agents)]
        if self.model_dir != "":
            self.restore()
        self.trainer = TrainAlgo(config, self.policy, self.num_agents, device=self.device, use_target_critic=config.get("use_target_critic", False),
                                 fused=config.get("fused", True))
        self.buffer = []
        for a in range(self.num_agents):                # one joint-action ring for all agents (the reference stores N copies)
            self.buffer.append(ReplayBuffer(config, self.envs.observation_space[a].shape, self.envs.share_observation_space[a].shape,
                                            self.envs.action_space[a].shape, self.envs.action_space, device=self.device,
                                            joint_actions=self.buffer[0].joint_actions if a else None))
        self.updates = 0
        self.last_train_infos = None

    def _stage(self, obs, share_obs):
        """The current observation into the ring rows the next add_transitions fills."""
        for a in range(self.num_agents):
            k = self.buffer[a].slot()
            self.buffer[a].obs[k].copy_(obs[:, a])
            self.buffer[a].share_obs[k].copy_(share_obs[:, a])

    def run(self):
        obs, share_obs, _ = self.envs.reset()
        self._stage(obs, share_obs)
        start = time.time()
        episodes = int(self.num_env_steps) // self.episode_length // self.n_rollout_threads
        train_episode_rewards = torch.zeros(self.n_rollout_threads, dtype=torch.float, device=self.device)
        train_infos = None
        for episode in range(episodes):
            done_sum = torch.zeros((), device=self.device)          # finished episodes' rewards and their number: no host loop, no
            done_count = torch.zeros((), device=self.device)        # synchronisation inside the episode
            for step in range(self.episode_length):
                actions, joint_actions = self.collect(step)
                next_obs, next_share_obs, rewards, dones, infos, _ = self.envs.step(joint_actions)
                dones_env = torch.all(dones.bool(), dim=1)
                train_episode_rewards += torch.mean(rewards, dim=1).flatten()
                done_sum += (train_episode_rewards * dones_env).sum()
                done_count += dones_env.sum()
                train_episode_rewards = train_episode_rewards * (~dones_env)
                self.insert((obs, share_obs, rewards, next_obs, next_share_obs, actions, joint_actions, dones, infos))
                obs = next_obs
                share_obs = next_share_obs
                self._stage(obs, share_obs)
                if self.buffer[0].step > self.batch_size:
                    self.warm_up = False
                if not self.warm_up:
                    train_infos = self.train()
            total_num_steps = (episode + 1) * self.episode_length * self.n_rollout_threads
            if episode % self.save_interval == 0 or episode == episodes - 1:
                self.save()
            if episode % self.log_interval == 0:
                end = time.time()
                print("\nAlgo {} Exp {} updates {}/{} episodes, total num timesteps {}/{}, FPS {}.\n".format(
                    self.algorithm_name, self.experiment_name, episode, episodes, total_num_steps, self.num_env_steps, int(total_num_steps / (end - start))))
                if not self.warm_up:
                    self.log_train(train_infos, total_num_steps)
            if float(done_count) != 0:
                aver_episode_rewards = done_sum / done_count
                print("some episodes done, average rewards: ", aver_episode_rewards)
                self.writter.add_scalars("train_episode_rewards", {"aver_rewards": aver_episode_rewards}, total_num_steps)
            if episode % self.eval_interval == 0 and self.use_eval:
                self.eval(total_num_steps)

    def collect(self, step):
        self.trainer.prep_rollout()
        slots = [b.slot() for b in self.buffer]
        return self.trainer.act_all([b.obs[k] for b, k in zip(self.buffer, slots)], deterministic=False,
                                    act_slots=[b.actions[k] for b, k in zip(self.buffer, slots)], joint_slot=self.buffer[0].joint_actions[slots[0]])

    def insert(self, data):
        obs, share_obs, rewards, next_obs, next_share_obs, actions, joint_actions, dones, infos = data
        for a in range(self.num_agents):
            k = self.buffer[a].slot()                   # obs, share_obs (staged), actions and joint_actions (the head kernel) are in place
            self.buffer[a].add_transitions(self.buffer[a].obs[k], self.buffer[a].share_obs[k], actions[a], joint_actions, rewards[:, a], next_obs[:, a],
                                           next_share_obs[:, a], dones[:, a])

    def train(self):
        train_infos = self.trainer.train(self.buffer)
        self.updates += 1
        self.last_train_infos = train_infos
        return train_infos

    def save(self):
        for a in range(self.num_agents):
            torch.save(self.trainer.policy[a].actor.state_dict(), str(self.save_dir) + "/actor_agent" + str(a) + ".pt")
            torch.save(self.trainer.policy[a].critic.state_dict(), str(self.save_dir) + "/critic_agent" + str(a) + ".pt")

    def restore(self):
        for a in range(self.num_agents):
            self.policy[a].actor.load_state_dict(torch.load(str(self.model_dir) + '/actor_agent' + str(a) + '.pt'))
            self.policy[a].critic.load_state_dict(torch.load(str(self.model_dir) + '/critic_agent' + str(a) + '.pt'))

    def log_train(self, train_infos, total_num_steps):
        for a in range(self.num_agents):
            for k, v in train_infos[a].items():
                agent_k = "agent%i/" % a + k
                self.writter.add_scalars(agent_k, {agent_k: v}, total_num_steps)

    def log_env(self, env_infos, total_num_steps):
        for k, v in env_infos.items():
            self.writter.add_scalars(k, {k: torch.mean(v)}, total_num_steps)

    @torch.no_grad()
    def eval(self, total_num_steps):
        eval_episode = 0
        episode_sum = torch.zeros(self.n_eval_rollout_threads, device=self.device)
        finished = []
        eval_obs, eval_share_obs, _ = self.eval_envs.reset()
        while True:
            self.trainer.prep_rollout()
            _, eval_joint = self.trainer.act_all([eval_obs[:, a] for a in range(self.num_agents)], deterministic=True)
            eval_obs, eval_share_obs, eval_rewards, eval_dones, eval_infos, _ = self.eval_envs.step(eval_joint)
            episode_sum += eval_rewards.sum(dim=(1, 2))
            eval_dones_env = torch.all(eval_dones.bool(), dim=1)
            n = int(eval_dones_env.sum())
            if n:
                eval_episode += n
                finished.append(episode_sum[eval_dones_env])
                episode_sum = episode_sum * (~eval_dones_env)
            if eval_episode >= self.eval_episodes:
                eval_episode_rewards = torch.cat(finished, dim=-1)
                eval_env_infos = {'eval_average_episode_rewards': torch.mean(eval_episode_rewards), 'eval_max_episode_rewards': torch.max(eval_episode_rewards)}
                print(eval_env_infos)
                self.log_env(eval_env_infos, total_num_steps)
                print("eval_average_episode_rewards is {}.".format(torch.mean(eval_episode_rewards)))
                break

"""Runner of the on-policy multi-agent algorithms (agents/algorithms/marl/runner.py): `Runner(vec_env, config, model_dir="")` for
algorithm_name mappo, happo and hatrpo, with the reference's methods `run`, `warmup`, `collect`, `insert`, `compute`, `train`, `save`,
`restore`, `eval`, `log_train` over this package's policies (policy.py), trainers (trainer.py, hatrpo.py) and buffers.

Repairs, limited to what cannot execute in the reference:
  * `run` called `self.trainer.policy.lr_decay` on the LIST of trainers (use_linear_lr_decay: True raises there): every trainer's policy
    decays;
  * the first `log_train` took `np.mean` of a device tensor; it is shadowed by the second definition, which is the one Python keeps and
    the one here;
  * `insert` indexed with `dones == True` on whatever dtype the env returns: the masks are formed from `dones.bool()`.
What changes besides:
  * the per-env Python loop over `dones_env` in `run` (one host synchronisation per env and step) is
    `SharedRolloutBuffers.finished_episode_rewards`: masked tensor arithmetic with the same mean over the finished episodes;
  * `collect` and `compute` go through GroupedPolicyInference (one grouped pass over all agents instead of a loop over them; the sampled
    actions come from this build's counter-based noise stream, policy_inference.py);
  * tensorboard is optional (a writer that does nothing when it is not installed);
  * use_single_network (a `policy.model` that no policy class of the reference's on-policy set defines) raises.

`train()` is the reference's sequential update (runner.py:266-316): the agents in the order of one `torch.randperm(num_agents)`, drawn
first; per agent `buffer.update_factor(factor)`, `trainer.train(buffer)`, factor *= exp(sum_dims(new_logp - old_logp)) over all T x N
stored rows, `buffer.after_update()`.  The two log-probability passes per agent:
  * feed-forward policies (`config["fused_factor"]`, absent in the reference's configs, default True): ONE grouped
    `GroupedPolicyInference.evaluate_actions` over all agents for the old log-probabilities before the loop -- an actor does not change
    until its own update, so this equals the per-agent calls -- and per agent one `evaluate_actions(agents=[k], old_logp=..., factor=...)`
    after its update, whose tail kernel (mms_marl_heads_eval) multiplies the factor in place: 1 + num_agents calls per train();
  * recurrent policies, and everything with `fused_factor: False`: the modules' own `actor.evaluate_actions` before and after the update
    and the product in torch, as the reference does (the sequence evaluation is RNNLayer's).  `fused_factor: True` with a recurrent
    policy raises.
`train_infos` is in UPDATE order, as in the reference (its log_train labels entry i "agent i" all the same).

`config["grouped_update"]` (absent in the reference's configs; default False = the loop above, unchanged; mappo only): MAPPO's surrogate
does not read the factor and each agent has its own policy, buffer and normaliser, so the agents' updates do not depend on each other.
True runs them in lockstep BEFORE the loop -- `MAPPO.train_group` over the trainers and buffers in `order` (trainer.py: the bases in
grouped calls, one mms_marl_ppo_loss_group call per minibatch step, one host read per train()) -- and then walks `order` exactly as
above without the `trainer.train` call: agent a's buffer receives the running factor, the factor takes agent a's ratio through the same
call.  Another agent's update does not change agent a's log-probabilities, so every buffer's factor, `last_factor`, the policies and
`train_infos` (in `order`) equal the loop's.  happo and hatrpo raise (their agents are sequential by definition: each surrogate carries
the factor of the agents updated before it), so do recurrent policies and trainers without `fused_block_update`.

`config["shared_buffers"]` (absent in the reference's configs; default False = one SeparatedReplayBuffer per agent): True runs on one
SharedRolloutBuffers (utils/shared_buffer.py) with `collect_into` / `env_step` / `insert_step` / `values_into`: observations, actions,
log-probabilities and values are read and written in the rollout slots where they lie.  `self.buffer` is then the list of its per-agent
views; the slots' roll-over (`after_update`) runs once after the last agent's update, since the views share their storage.  It needs
use_centralized_V."""
import os
import time

import torch

from .policy_inference import GroupedPolicyInference
from .utils.separated_buffer import SeparatedReplayBuffer
from .utils.shared_buffer import SharedRolloutBuffers

try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:                                       # tensorboard is not installed: nothing is logged
    class SummaryWriter:
        def __init__(self, *args, **kwargs):
            pass

        def __getattr__(self, name):
            return lambda *args, **kwargs: None


def _rows(x):
    return x.reshape(-1, *x.shape[2:])


def _classes(name):
    if name == "mappo":
        from .policy import MAPPO_Policy as Policy
        from .trainer import MAPPO as TrainAlgo
    elif name == "happo":
        from .policy import HAPPO_Policy as Policy
        from .trainer import HAPPO as TrainAlgo
    elif name == "hatrpo":
        from .hatrpo import HATRPO as TrainAlgo
        from .policy import HATRPO_Policy as Policy
    else:
        raise ValueError("Runner: algorithm_name must be mappo, happo or hatrpo, got %r" % (name,))
    return TrainAlgo, Policy


class Runner:
    def __init__(self, vec_env, config, model_dir=""):
        self.envs = vec_env
        self.eval_envs = vec_env
        cfg = vec_env.task.cfg
        self.env_name = cfg["env"].get("env_name", getattr(vec_env.task, "TASK_NAME", "env"))
        self.algorithm_name = config["algorithm_name"]
        self.experiment_name = config["experiment_name"]
        self.use_centralized_V = config["use_centralized_V"]
        self.use_obs_instead_of_state = config["use_obs_instead_of_state"]
        self.num_env_steps = config["num_env_steps"]
        self.episode_length = config["episode_length"]
        self.n_rollout_threads = config["n_rollout_threads"]
        self.n_eval_rollout_threads = config["n_eval_rollout_threads"]
        self.use_linear_lr_decay = config["use_linear_lr_decay"]
        self.hidden_size = config["hidden_size"]
        self.use_render = config["use_render"]
        self.recurrent_N = config["recurrent_N"]
        self.use_single_network = config["use_single_network"]
        self.save_interval = config["save_interval"]
        self.use_eval = config["use_eval"]
        self.eval_interval = config["eval_interval"]
        self.eval_episodes = config["eval_episodes"]
        self.log_interval = config["log_interval"]
        self.seed = cfg.get("seed", 0)
        self.model_dir = model_dir
        self.num_agents = self.envs.num_agents
        self.device = self.envs.rl_device
        if self.use_single_network:
            raise NotImplementedError("Runner: use_single_network is not covered (the policies hold an actor and a critic)")
        TrainAlgo, Policy = _classes(self.algorithm_name)
        self.recurrent = bool(config["use_recurrent_policy"] or config["use_naive_recurrent_policy"])
        self.fused_factor = bool(config.get("fused_factor", not self.recurrent))
        if self.fused_factor and self.recurrent:
            raise NotImplementedError("Runner: fused_factor covers feed-forward policies; recurrent ones evaluate sequences through the modules")
        # opt-in (the reference's config has no such key): MAPPO's agents updated in lockstep through MAPPO.train_group (train below)
        self.grouped_update = bool(config.get("grouped_update", False))
        if self.grouped_update:
            if self.algorithm_name != "mappo":
                raise NotImplementedError("Runner: grouped_update covers mappo; %s updates its agents one after another by definition (each agent's "
                                          "surrogate carries the factor of those updated before it)" % self.algorithm_name)
            if self.recurrent:
                raise NotImplementedError("Runner: grouped_update covers feed-forward policies (a recurrent minibatch is a set of sequences)")
            if not config.get("fused_block_update", False):
                raise NotImplementedError("Runner: grouped_update needs fused_block_update (the grouped step runs the bases through blocks.mlp_base)")
        self.run_dir = config["run_dir"]
        self.log_dir = str(self.run_dir + '/' + self.env_name + '/' + self.algorithm_name + '/logs_seed{}'.format(self.seed))
        os.makedirs(self.log_dir, exist_ok=True)
        self.writter = SummaryWriter(self.log_dir)
        self.save_dir = str(self.run_dir + '/' + self.env_name + '/' + self.algorithm_name + '/models_seed{}'.format(self.seed))
        os.makedirs(self.save_dir, exist_ok=True)

        share_space = lambda a: self.envs.share_observation_space[a] if self.use_centralized_V else self.envs.observation_space[a]
        self.policy = [Policy(config, self.envs.observation_space[a], share_space(a), self.envs.action_space[a], device=self.device)
                       for a in range(self.num_agents)]
        if self.model_dir != "":
            self.restore()
        self.trainer = [TrainAlgo(config, self.policy[a], device=self.device) for a in range(self.num_agents)]
        self.shared = None
        if config.get("shared_buffers", False):
            if not self.use_centralized_V:
                raise NotImplementedError("Runner: shared_buffers stores the centralised observation once; it needs use_centralized_V")
            self.shared = SharedRolloutBuffers(config, self.envs, self.device)
            self.buffer = self.shared.agents
        else:
            self.buffer = [SeparatedReplayBuffer(config, self.envs.observation_space[a], share_space(a), self.envs.action_space[a], self.device)
                           for a in range(self.num_agents)]
        self.grouped = GroupedPolicyInference.from_trainers(self.trainer, seed=int(self.seed))

    # -- the loop -----------------------------------------------------------------------------------------------------------------
    def run(self):
        self.warmup()
        start = time.time()
        episodes = int(self.num_env_steps) // self.episode_length // self.n_rollout_threads
        train_episode_rewards = torch.zeros(self.n_rollout_threads, device=self.device)
        finished = SharedRolloutBuffers.finished_episode_rewards
        for episode in range(episodes):
            if self.use_linear_lr_decay:
                for trainer in self.trainer:
                    trainer.policy.lr_decay(episode, episodes)
            done_sum = torch.zeros((), device=self.device)          # finished episodes' rewards and their number: no host loop, no
            done_count = torch.zeros((), device=self.device)        # synchronisation inside the episode
            for step in range(self.episode_length):
                values, actions, action_log_probs, rnn_states, rnn_states_critic = self.collect(step)
                if self.shared is not None:
                    rewards, dones = self.shared.env_step(actions)
                    obs = share_obs = infos = None                   # (the engine wrote the next observation slot in place)
                    total, count = finished(self.shared, train_episode_rewards, rewards.flatten(), dones)
                else:
                    obs, share_obs, rewards, dones, infos, _ = self.envs.step(actions)
                    total, count = finished(None, train_episode_rewards, torch.mean(rewards, dim=1).flatten(), torch.all(dones.bool(), dim=1))
                done_sum += total
                done_count += count
                self.insert((obs, share_obs, rewards, dones, infos, values, actions, action_log_probs, rnn_states, rnn_states_critic))
            self.compute()
            train_infos = self.train()
            total_num_steps = (episode + 1) * self.episode_length * self.n_rollout_threads
            if episode % self.save_interval == 0 or episode == episodes - 1:
                self.save()
            if episode % self.log_interval == 0:
                end = time.time()
                print("\nAlgo {} Exp {} updates {}/{} episodes, total num timesteps {}/{}, FPS {}.\n".format(
                    self.algorithm_name, self.experiment_name, episode, episodes, total_num_steps, self.num_env_steps, int(total_num_steps / (end - start))))
                self.log_train(train_infos, total_num_steps)
            if float(done_count) != 0:                               # (the one host read per episode)
                aver_episode_rewards = done_sum / done_count
                print("some episodes done, average rewards: ", aver_episode_rewards)
                self.writter.add_scalars("train_episode_rewards", {"aver_rewards": aver_episode_rewards}, total_num_steps)
            if episode % self.eval_interval == 0 and self.use_eval:
                self.eval(total_num_steps)

    def warmup(self):
        if self.shared is not None:
            self.shared.warmup()
            return
        obs, share_obs, _ = self.envs.reset()
        if not self.use_centralized_V:
            share_obs = obs
        for a in range(self.num_agents):
            self.buffer[a].share_obs[0].copy_(share_obs[:, a])
            self.buffer[a].obs[0].copy_(obs[:, a])

    @torch.no_grad()
    def collect(self, step):
        """(values [N, agents, 1], per-agent action and log-prob lists, rnn_states, rnn_states_critic [N, agents, ...]) from one grouped
        pass.  shared_buffers: everything is written into slot `step` of the shared storage (and the new recurrent states into slot
        step + 1); the second value is then the [N, agents, act_dim] action slot itself, the third the log-prob slot."""
        for trainer in self.trainer:
            trainer.prep_rollout()
        if self.shared is None:
            return self.grouped.collect(self.buffer, step)
        sh, s = self.shared, self.shared.step
        self.grouped.collect_into(sh)
        nxt = s + 1 if self.recurrent else s
        return sh.value_preds[s], sh.actions[s], sh.action_log_probs[s], sh.rnn_states[nxt], sh.rnn_states_critic[nxt]

    def insert(self, data):
        obs, share_obs, rewards, dones, infos, values, actions, action_log_probs, rnn_states, rnn_states_critic = data
        if self.shared is not None:                                  # (what collect_into wrote in place is recognised by its address)
            self.shared.insert_step(rewards, dones, values, actions, action_log_probs)
            return
        dones = dones.bool()
        dones_env = torch.all(dones, dim=1)
        rnn_states[dones_env] = 0.0
        rnn_states_critic[dones_env] = 0.0
        masks = torch.ones(self.n_rollout_threads, self.num_agents, 1, device=self.device)
        masks[dones_env] = 0.0
        active_masks = torch.ones(self.n_rollout_threads, self.num_agents, 1, device=self.device)
        active_masks[dones] = 0.0
        active_masks[dones_env] = 1.0
        if not self.use_centralized_V:
            share_obs = obs
        for a in range(self.num_agents):
            self.buffer[a].insert(share_obs[:, a], obs[:, a], rnn_states[:, a], rnn_states_critic[:, a], actions[a], action_log_probs[a],
                                  values[:, a], rewards[:, a], masks[:, a], None, active_masks[:, a], None)

    @torch.no_grad()
    def compute(self):
        for trainer in self.trainer:
            trainer.prep_rollout()
        norms = [trainer.value_normalizer for trainer in self.trainer]
        if self.shared is not None:
            nxt = torch.zeros(self.n_rollout_threads, self.num_agents, device=self.device)
            self.grouped.values_into(self.shared, nxt)
            self.shared.compute_returns(nxt, norms)
            return
        kw = {}
        if self.recurrent:
            kw = dict(rnn_states_critic=[b.rnn_states_critic[-1] for b in self.buffer], masks=[b.masks[-1] for b in self.buffer])
        values = self.grouped.get_values([b.share_obs[-1] for b in self.buffer], **kw)
        for a in range(self.num_agents):
            self.buffer[a].compute_returns(values[a].detach(), norms[a])

    # -- the update ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _module_logp(self, a):
        """Agent a's per-dimension log-probabilities of its stored actions over all T x N rows from the module itself (runner.py:282-310)"""
        b = self.buffer[a]
        return self.trainer[a].policy.actor.evaluate_actions(_rows(b.obs[:-1]), _rows(b.rnn_states[0:1]), _rows(b.actions), _rows(b.masks[:-1]), None,
                                                              _rows(b.active_masks[:-1]))[0].detach()

    def train(self):
        order = torch.randperm(self.num_agents)                      # drawn first, as the reference draws it
        T, N = self.episode_length, self.n_rollout_threads
        factor = torch.ones(T, N, 1, device=self.device)
        train_infos = []
        if self.fused_factor:
            obs, acts = [_rows(b.obs[:-1]) for b in self.buffer], [_rows(b.actions) for b in self.buffer]
            old = [t.clone() for t in self.grouped.evaluate_actions(obs, acts)]
        group_infos = None
        if self.grouped_update:
            # every agent's update at once (no agent's update reads another's policy, buffer or factor), then the loop below as ever:
            # agent a's log-probabilities before and after its own update are what they are in the sequential order
            ids = [int(a) for a in order]
            for a in ids:
                self.trainer[a].prep_training()
            if not self.fused_factor:
                old_module = {a: self._module_logp(a) for a in ids}
            group_infos = dict(zip(ids, type(self.trainer[0]).train_group([self.trainer[a] for a in ids], [self.buffer[a] for a in ids])))
        for agent_id in order:
            a = int(agent_id)
            self.trainer[a].prep_training()
            self.buffer[a].update_factor(factor)
            if not self.fused_factor:
                old_logp = old_module[a] if self.grouped_update else self._module_logp(a)
            train_info = group_infos[a] if self.grouped_update else self.trainer[a].train(self.buffer[a])
            if self.fused_factor:
                self.grouped.evaluate_actions([obs[a]], [acts[a]], agents=[a], old_logp=[old[a]], factor=factor.view(-1, 1))
            else:
                new_logp = self._module_logp(a)
                factor = factor * torch.exp((new_logp - old_logp).reshape(T, N, -1).sum(dim=-1, keepdim=True))
            train_infos.append(train_info)
            if self.shared is None:
                self.buffer[a].after_update()
        if self.shared is not None:
            self.shared.after_update()
        self.last_factor = factor
        return train_infos

    # -- checkpoints, logs, evaluation ----------------------------------------------------------------------------------------------
    def save(self):
        for a in range(self.num_agents):
            torch.save(self.trainer[a].policy.actor.state_dict(), str(self.save_dir) + "/actor_agent" + str(a) + ".pt")
            torch.save(self.trainer[a].policy.critic.state_dict(), str(self.save_dir) + "/critic_agent" + str(a) + ".pt")

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
        n = self.n_eval_rollout_threads
        eval_episode = 0
        episode_sum = torch.zeros(n, device=self.device)
        finished = []
        eval_obs, eval_share_obs, _ = self.eval_envs.reset()
        eval_rnn_states = torch.zeros(n, self.num_agents, self.recurrent_N, self.hidden_size, device=self.device)
        eval_masks = torch.ones(n, self.num_agents, 1, device=self.device)
        while True:
            eval_actions = []
            for a in range(self.num_agents):
                self.trainer[a].prep_rollout()
                action, state = self.trainer[a].policy.act(eval_obs[:, a], eval_rnn_states[:, a], eval_masks[:, a], deterministic=True)
                eval_rnn_states[:, a] = state
                eval_actions.append(action)
            eval_obs, eval_share_obs, eval_rewards, eval_dones, eval_infos, _ = self.eval_envs.step(eval_actions)
            episode_sum += eval_rewards.sum(dim=(1, 2))
            eval_dones_env = torch.all(eval_dones.bool(), dim=1)
            eval_rnn_states[eval_dones_env] = 0.0
            eval_masks = torch.ones(n, self.num_agents, 1, device=self.device)
            eval_masks[eval_dones_env] = 0.0
            count = int(eval_dones_env.sum())
            if count:
                eval_episode += count
                finished.append(episode_sum[eval_dones_env])
                episode_sum = episode_sum * (~eval_dones_env)
            if eval_episode >= self.eval_episodes:
                eval_episode_rewards = torch.cat(finished, dim=-1)
                eval_env_infos = {'eval_average_episode_rewards': torch.mean(eval_episode_rewards), 'eval_max_episode_rewards': torch.max(eval_episode_rewards)}
                print(eval_env_infos)
                self.log_env(eval_env_infos, total_num_steps)
                print("eval_average_episode_rewards is {}.".format(torch.mean(eval_episode_rewards)))
                break

"""DDPG, the learner (agents/algorithms/rl/ddpg/ddpg.py), and everything TD3 shares with it (td3/td3.py is this file plus twin critics
and `policy_delay`): the reference's constructor, attributes, `learn` config keys and methods (`run`, `update`, `compute_loss_q`,
`compute_loss_pi`, `log`, `save`, `load`, `test`) over this package's MLPActorCritic and ReplayBuffer, so `process_sarl`'s DDPG / TD3
branches train without the reference tree.  The loop, the log and the checkpoint methods are off_policy.OffPolicyLearner's, shared
with SAC; the update is written here once for both learners.

The default route is the reference's arithmetic statement for statement, including what its code actually does:
  * the body of the minibatch loop only gathers (ddpg.py:283-297, td3.py:286-300), so each epoch takes ONE optimisation step, on the
    LAST of the `nminibatches` index lists, which are drawn once per `update()`; the discarded gathers are not repeated here;
  * TD3 counts `learn_ep` inside that loop, so at the step it equals the number of lists: the policy step runs iff
    `nminibatches % policy_delay == 0`, in every epoch or in none (then the mean surrogate loss is 0); DDPG always takes it;
  * both means are still divided by `noptepochs * nminibatches`;
  * `self.q_params` is a generator (DDPG: `q.parameters()`) or an `itertools.chain` (TD3) that `Adam(...)` exhausts, so the freeze /
    unfreeze loops around the policy step iterate nothing: `loss_pi.backward()` deposits gradients into the critic it runs through;
  * `clip_grad_norm_(self.actor_critic.parameters(), ...)` runs in both steps over EVERY parameter and rewrites stale gradients in place;
  * DDPG smooths its target action as TD3 does (ddpg.py:359-365);
  * polyak runs over all parameters, `pi` included, after every step -- also after a Q step without a policy step;
  * `warm_up` ends when `storage.step > batch_size`; rewards are not scaled; the log directory gets no seed suffix.

New `learn` keys, all defaulting to the above:
  * `fused_update` (False).  True: the modules are built with `fused_grad=True`; the target action is `actor_critic_targ.pi.smoothed`
    (mms_det_heads_act: the last layer, the noise and both clamps in one launch) and the backup `actor_critic_targ.q_backup`
    (mms_q_heads_backup); the losses are `MLPActorCritic.q_loss` / `pi_loss` (mms_q_heads_loss; the actor's head with a gradient is
    mms_det_heads_act / mms_det_heads_grad, written into the critic's [o | a] block); both optimizers are `FusedAdam`s called as
    `clip_and_step(max_norm, also_norm=<the other networks' parameters>, targets=..., polyak=...)`, with the clip coefficient applied
    to the stored gradients on the device from the returned norm, as SAC._fused_minibatch does.  The running losses add up on the device
    and are read once per `update()`; nothing inside a step reads the device from the host.  The smoothing noise is the target
    actor's counter stream (module.py), keyed apart from the online actor's exploration noise.
  * `freeze_q` (False).  True: `self.q_params` is a list, so the freeze loops do what the reference's comments say.
  * `layers` ("fp32"), handed to MLPActorCritic.

`eps_source` (attribute, None): a callable(shape) returning the standard normals of the next target policy smoothing -- a recorded run
replayed (tests/golden/{td3,ddpg}_update.npz).  Where the env exposes this package's engine, `run` binds its observation output to the
ring row the next `add_transitions` fills (OffPolicyLearner.run)."""
from copy import deepcopy

import torch
import torch.nn as nn
from torch.optim import Adam

from ....optim import FusedAdam
from ....spaces import Space
from ..off_policy import OffPolicyLearner, SummaryWriter
from .module import MLPActorCritic
from .storage import ReplayBuffer


class DDPG(OffPolicyLearner):
    ActorCritic = MLPActorCritic

    def __init__(self, vec_env, cfg_train, device='cpu', sampler='random', log_dir='run', is_testing=False, print_log=True, apply_reset=False,
                 asymmetric=False):
        for name in ("observation_space", "state_space", "action_space"):
            if not isinstance(getattr(vec_env, name), Space):
                raise TypeError("vec_env.%s must be a gym Space" % name)
        self.observation_space = vec_env.observation_space
        self.action_space = vec_env.action_space
        self.state_space = vec_env.state_space
        self.act_limit = vec_env.action_space.high[0]
        self.device = device
        self.asymmetric = asymmetric
        learn_cfg = cfg_train["learn"]
        self.learning_rate = learn_cfg["learning_rate"]

        self.num_transitions_per_env = learn_cfg["nsteps"]
        self.num_learning_epochs = learn_cfg["noptepochs"]
        self.num_mini_batches = learn_cfg["nminibatches"]
        self.gamma = learn_cfg["gamma"]
        self.polyak = learn_cfg["polyak"]
        self.max_grad_norm = learn_cfg.get("max_grad_norm", 2.0)
        self._init_delay(learn_cfg)
        self.target_noise = learn_cfg["target_noise"]
        self.act_noise = learn_cfg["act_noise"]
        self.noise_clip = learn_cfg["noise_clip"]
        self.use_clipped_value_loss = learn_cfg.get("use_clipped_value_loss", False)
        self.replay_size = learn_cfg["replay_size"]
        self.batch_size = learn_cfg["batch_size"]
        self.fused_update = bool(learn_cfg.get("fused_update", False))
        self.freeze_q = bool(learn_cfg.get("freeze_q", False))
        self.layers = learn_cfg.get("layers", "fp32")

        self.vec_env = vec_env
        ac_kwargs = dict(hidden_sizes=[learn_cfg["hidden_nodes"]] * learn_cfg["hidden_layer"], layers=self.layers, fused_grad=self.fused_update)
        self.actor_critic = self.ActorCritic(vec_env.observation_space, vec_env.action_space, self.act_noise, self.device, **ac_kwargs).to(self.device)
        self.actor_critic_targ = deepcopy(self.actor_critic)
        if self.fused_update:               # the copy's smoothing noise and the online actor's exploration noise: two streams
            self.actor_critic_targ.pi.seed = (self.actor_critic.pi.seed + 0x9E3779B97F4A7C15) % 2 ** 62
        self.storage = ReplayBuffer(vec_env.num_envs, self.replay_size, self.batch_size, self.num_transitions_per_env, self.observation_space.shape,
                                    self.state_space.shape, self.action_space.shape, self.device, sampler)
        # the target networks move by polyak averaging only
        for p in self.actor_critic_targ.parameters():
            p.requires_grad = False

        # ddpg.py:83, td3.py:86: a generator / a chain, which the optimizer's constructor exhausts; freeze_q keeps a list
        self.q_params = self._q_params()
        if self.freeze_q:
            self.q_params = list(self.q_params)
        optimizer = FusedAdam if self.fused_update else Adam
        self.pi_optimizer = optimizer(self.actor_critic.pi.parameters(), lr=self.learning_rate)
        self.q_optimizer = optimizer(self.q_params, lr=self.learning_rate)

        self.reward_scale = learn_cfg["reward_scale"]
        self.warm_up = True
        self.eps_source = None

        # Log
        self.log_dir = log_dir
        self.print_log = print_log
        self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
        self.tot_timesteps = 0
        self.tot_time = 0
        self.is_testing = is_testing
        self.current_learning_iteration = 0
        self.apply_reset = apply_reset

    # ---- what TD3 changes ----------------------------------------------------------------------------------------------------------

    def _init_delay(self, learn_cfg):
        pass

    def _q_params(self):
        return self.actor_critic.q.parameters()

    def _policy_due(self, learn_ep):
        return True

    # ---- the loop, the log and the checkpoints are OffPolicyLearner's, but for -------------------------------------------------------
    scales_rewards = False                  # (ddpg.py / td3.py keep `reward_scale` and never apply it)

    def _act(self, obs, explore):
        # ddpg.py:132, 155: the testing loop calls act(obs), whose default is deterministic; the rollout passes deterministic=False
        return self.actor_critic.act(obs, deterministic=False) if explore else self.actor_critic.act(obs)

    def _warm_up_over(self):
        return self.storage.step > self.batch_size

    # ---- the update ----------------------------------------------------------------------------------------------------------------

    def update(self):
        mean_value_loss = 0
        mean_surrogate_loss = 0
        batch = self.storage.mini_batch_generator(self.num_mini_batches)          # drawn once, reused by every epoch
        step = self._fused_minibatch if self.fused_update else self._minibatch
        for epoch in range(self.num_learning_epochs):
            learn_ep = len(batch)                                                  # the gather loop's count when it ends
            data = self._gather(batch[-1])                                         # ... and the only list it leaves behind
            loss_q, loss_pi = step(data, self._policy_due(learn_ep))
            mean_value_loss = mean_value_loss + loss_q
            mean_surrogate_loss = mean_surrogate_loss + loss_pi
        num_updates = self.num_learning_epochs * self.num_mini_batches
        if self.fused_update:                   # the one host read of the update
            mean_value_loss, mean_surrogate_loss = torch.stack([torch.as_tensor(v, dtype=torch.float32, device=self.device)
                                                                for v in (mean_value_loss, mean_surrogate_loss)]).tolist()
        return mean_value_loss / num_updates, mean_surrogate_loss / num_updates

    def _minibatch(self, data, policy_step):
        """One step of the default route (ddpg.py:305-342, td3.py:307-345); returns the two losses as host numbers."""
        self.q_optimizer.zero_grad()
        loss_q = self.compute_loss_q(data)
        loss_q.backward()
        nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
        self.q_optimizer.step()
        value_loss = loss_q.item()

        surrogate_loss = 0
        if policy_step:
            # (a generator / a chain: nothing; freeze_q: the critics take no gradient during the policy step)
            for p in self.q_params:
                p.requires_grad = False
            self.pi_optimizer.zero_grad()
            loss_pi = self.compute_loss_pi(data)
            loss_pi.backward()
            nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
            self.pi_optimizer.step()
            surrogate_loss = loss_pi.item()
            for p in self.q_params:
                p.requires_grad = True

        with torch.no_grad():
            for p, p_targ in zip(self.actor_critic.parameters(), self.actor_critic_targ.parameters()):
                p_targ.data.mul_(self.polyak)
                p_targ.data.add_((1 - self.polyak) * p.data)
        return value_loss, surrogate_loss

    def _fused_minibatch(self, data, policy_step):
        """One step of the fused route; returns the two losses as 0-d device tensors (0 for a skipped policy step).  No host read."""
        ac, targ = self.actor_critic, self.actor_critic_targ
        q_params = [p for q in ac._critics() for p in q.parameters()]
        q_targets = [p for q in targ._critics() for p in q.parameters()]
        pi_params, pi_targets = list(ac.pi.parameters()), list(targ.pi.parameters())

        self.q_optimizer.zero_grad()
        loss_q = self.compute_loss_q(data)
        loss_q.backward()
        norm = self.q_optimizer.clip_and_step(self.max_grad_norm, also_norm=pi_params, targets=q_targets, polyak=self.polyak)
        self._rescale(q_params, norm)           # they meet grad(L_pi) in the policy step (freeze_q: they enter its norm as they are)

        if not policy_step:                     # the actor still moves its target copy: the polyak loop runs over all parameters
            with torch.no_grad():
                self._rescale(pi_params, norm)  # (stale actor gradients, where there are any: the Q step's clip rewrites them too)
                torch._foreach_mul_([t.data for t in pi_targets], self.polyak)
                torch._foreach_add_([t.data for t in pi_targets], torch._foreach_mul([p.data for p in pi_params], 1 - self.polyak))
            return loss_q.detach(), 0
        for p in self.q_params:
            p.requires_grad = False
        self.pi_optimizer.zero_grad()
        loss_pi = self.compute_loss_pi(data)
        loss_pi.backward()
        norm = self.pi_optimizer.clip_and_step(self.max_grad_norm, also_norm=q_params, targets=pi_targets, polyak=self.polyak)
        self._rescale(pi_params, norm)          # the stale actor gradients of the next Q step's norm
        for p in self.q_params:
            p.requires_grad = True
        return loss_q.detach(), loss_pi.detach()

    def _smoothing_eps(self, o2):
        if self.eps_source is None:
            return None
        return self.eps_source(tuple(o2.shape[:-1]) + tuple(self.action_space.shape))

    def compute_loss_q(self, data):
        o, a, r, o2, d = data['obs'], data['act'], data['r'], data['obs2'], data['done']
        targ = self.actor_critic_targ
        if self.fused_update:
            with torch.no_grad():
                a2 = targ.pi.smoothed(o2, self.target_noise, self.noise_clip, eps=self._smoothing_eps(o2))
                backup = targ.q_backup(o2, a2, r, d, self.gamma)
            return self.actor_critic.q_loss(o, a, backup)
        qs = [q(o, a) for q in self.actor_critic._critics()]
        with torch.no_grad():
            pi_targ = targ.pi(o2)
            # target policy smoothing
            eps = self._smoothing_eps(o2)
            epsilon = (torch.randn_like(pi_targ) if eps is None else eps) * self.target_noise
            epsilon = torch.clamp(epsilon, -self.noise_clip, self.noise_clip)
            a2 = pi_targ + epsilon
            a2 = torch.clamp(a2, -self.act_limit, self.act_limit)
            q_pi_targ = targ._critics()[0](o2, a2)
            for q in targ._critics()[1:]:
                q_pi_targ = torch.min(q_pi_targ, q(o2, a2))
            backup = r + self.gamma * (1 - d) * q_pi_targ
        loss_q = ((qs[0] - backup) ** 2).mean()
        for q in qs[1:]:
            loss_q = loss_q + ((q - backup) ** 2).mean()
        return loss_q

    def compute_loss_pi(self, data):
        o = data['obs']
        if self.fused_update:
            return self.actor_critic.pi_loss(o)
        q_pi = self.actor_critic._critics()[0](o, self.actor_critic.pi(o))        # the first critic only (td3.py:385)
        return -q_pi.mean()

"""SAC, the learner (agents/algorithms/rl/sac/sac.py): the reference's constructor, attributes, `learn` config keys and methods
(`run`, `update`, `compute_loss_q`, `compute_loss_pi`, `log`, `save`, `load`, `test`) over this package's MLPActorCritic and
ReplayBuffer, so `process_sarl`'s SAC branch trains without the reference tree.

The default route is the reference's arithmetic statement for statement, including what its code actually does:
  * `self.q_params` is an `itertools.chain` that `Adam(...)` exhausts (sac.py:85-88), so the freeze / unfreeze loops around the policy
    step (sac.py:336-348) iterate nothing: `loss_pi.backward()` deposits gradients into the critics' parameters;
  * `clip_grad_norm_(self.actor_critic.parameters(), ...)` runs in both steps over EVERY parameter and rewrites gradients in place:
    the Q step's norm includes the stale actor gradients of the previous policy step (already scaled by that step's coefficient; None
    on the very first step), the policy step's norm is over c_q grad(L_q) + grad(L_pi) on the critics plus the actor's gradients;
  * the `batch` list of index lists is drawn once per `update()` and reused by every epoch;
  * polyak runs over all parameters, `pi` included, after both steps;
  * `warm_up` ends when `storage.step >= batch_size`, and `update()` runs inside the rollout loop after every env step from then on;
  * `rews *= reward_scale` is in place; `load` takes the iteration from the file name.

New `learn` keys, all defaulting to the above:
  * `fused_update` (False).  True: the actor is built with `fused_grad=True`; the Bellman backup comes from
    `actor_critic_targ.q_backup` (mms_q_heads_backup); both losses come from `MLPActorCritic.q_loss` / `pi_loss` (mms_q_heads_loss: the
    critics' last layers, the loss and their backward in one pass); both optimizers are `FusedAdam`s called as `clip_and_step(max_norm,
    also_norm=<the other networks' parameters>, targets=..., polyak=...)`.  FusedAdam does not rewrite gradients, so this route applies
    the clip coefficient to the stored gradients itself, on the device, from the returned norm -- which reproduces both effects of the
    clip bullet above.  The two running losses add up on the device and are read once per `update()`; nothing inside a minibatch reads
    the device from the host.  The sampled actions come from the actor's counter-based noise stream (module.py), not torch's generator.
  * `freeze_q` (False).  True: `self.q_params` is a list, so the freeze loops do what sac.py's comments say; the critics' weight
    gradients of loss_pi are not computed (dw / db NULL in the fused head).  Everything else is unchanged.
  * `layers` ("fp32"), handed to MLPActorCritic.

`eps_source` (attribute, None): a callable(shape) returning the standard normals of the next rsample -- a recorded run replayed through
the default route (tests/golden/sac_update.npz).  Where the env exposes this package's engine and nothing rewrites its observations,
`run` (off_policy.py, shared with DDPG and TD3) binds the engine's observation output to the ring row the next `add_transitions` fills (ReplayBuffer.slot()), so the step
kernel writes next_observations in place.  tensorboard is optional."""
import itertools
from copy import deepcopy

import torch
import torch.nn as nn
from torch.optim import Adam

from ....optim import FusedAdam
from ....spaces import Space
from ..off_policy import OffPolicyLearner, SummaryWriter
from .module import MLPActorCritic
from .storage import ReplayBuffer

class SAC(OffPolicyLearner):
    def __init__(self, vec_env, cfg_train, device='cpu', sampler='random', log_dir='run', is_testing=False, print_log=True, apply_reset=False,
                 asymmetric=False):
        for name in ("observation_space", "state_space", "action_space"):
            if not isinstance(getattr(vec_env, name), Space):
                raise TypeError("vec_env.%s must be a gym Space" % name)
        self.observation_space = vec_env.observation_space
        self.action_space = vec_env.action_space
        self.state_space = vec_env.state_space
        learn_cfg = cfg_train["learn"]
        self.device = device
        self.asymmetric = asymmetric
        self.learning_rate = learn_cfg["learning_rate"]
        self.replay_size = learn_cfg["replay_size"]
        self.batch_size = learn_cfg["batch_size"]
        self.num_transitions_per_env = learn_cfg["nsteps"]
        self.fused_update = bool(learn_cfg.get("fused_update", False))
        self.freeze_q = bool(learn_cfg.get("freeze_q", False))
        self.layers = learn_cfg.get("layers", "fp32")

        # SAC components
        self.vec_env = vec_env
        ac_kwargs = dict(hidden_sizes=[learn_cfg["hidden_nodes"]] * learn_cfg["hidden_layer"], layers=self.layers, fused_grad=self.fused_update)
        self.actor_critic = MLPActorCritic(vec_env.observation_space, vec_env.action_space, **ac_kwargs).to(self.device)
        print(self.actor_critic)
        self.actor_critic_targ = deepcopy(self.actor_critic)
        self.storage = ReplayBuffer(vec_env.num_envs, self.replay_size, self.batch_size, self.num_transitions_per_env, self.observation_space.shape,
                                    self.state_space.shape, self.action_space.shape, self.device, sampler)
        # the target networks move by polyak averaging only
        for p in self.actor_critic_targ.parameters():
            p.requires_grad = False

        # sac.py:85-88: a chain, which the optimizer's constructor exhausts; freeze_q keeps a list
        self.q_params = itertools.chain(self.actor_critic.q1.parameters(), self.actor_critic.q2.parameters())
        if self.freeze_q:
            self.q_params = list(self.q_params)
        optimizer = FusedAdam if self.fused_update else Adam
        self.pi_optimizer = optimizer(self.actor_critic.pi.parameters(), lr=self.learning_rate)
        self.q_optimizer = optimizer(self.q_params, lr=self.learning_rate)

        # SAC parameters
        self.num_learning_epochs = learn_cfg["noptepochs"]
        self.num_mini_batches = learn_cfg["nminibatches"]
        self.entropy_coef = learn_cfg["ent_coef"]
        self.gamma = learn_cfg["gamma"]
        self.polyak = learn_cfg["polyak"]
        self.max_grad_norm = learn_cfg.get("max_grad_norm", 2.0)
        self.use_clipped_value_loss = learn_cfg.get("use_clipped_value_loss", False)
        self.reward_scale = learn_cfg["reward_scale"]
        self.warm_up = True
        self.eps_source = None

        # Log
        log_dir = log_dir + "_seed{}".format(self.vec_env.task.cfg["seed"])
        self.log_dir = log_dir
        self.print_log = print_log
        self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
        self.tot_timesteps = 0
        self.tot_time = 0
        self.is_testing = is_testing
        self.current_learning_iteration = 0
        self.apply_reset = apply_reset

    # ---- the update ----------------------------------------------------------------------------------------------------------------

    def update(self):
        mean_value_loss = 0
        mean_surrogate_loss = 0
        batch = self.storage.mini_batch_generator(self.num_mini_batches)          # drawn once, reused by every epoch
        step = self._fused_minibatch if self.fused_update else self._minibatch
        for epoch in range(self.num_learning_epochs):
            for indices in batch:
                loss_q, loss_pi = step(self._gather(indices))
                mean_value_loss = mean_value_loss + loss_q
                mean_surrogate_loss = mean_surrogate_loss + loss_pi
        num_updates = self.num_learning_epochs * self.num_mini_batches
        if self.fused_update:                   # the one host read of the update
            mean_value_loss, mean_surrogate_loss = torch.stack([mean_value_loss, mean_surrogate_loss]).tolist()
        return mean_value_loss / num_updates, mean_surrogate_loss / num_updates

    def _minibatch(self, data):
        """One minibatch of the default route (sac.py:325-359); returns the two losses as host numbers."""
        self.q_optimizer.zero_grad()
        loss_q = self.compute_loss_q(data)
        loss_q.backward()
        nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
        self.q_optimizer.step()
        value_loss = loss_q.item()

        # (a chain: nothing; freeze_q: the critics take no gradient during the policy step)
        for p in self.q_params:
            p.requires_grad = False
        self.pi_optimizer.zero_grad()
        loss_pi = self.compute_loss_pi(data)
        loss_pi.backward()
        nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
        self.pi_optimizer.step()
        for p in self.q_params:
            p.requires_grad = True
        surrogate_loss = loss_pi.item()

        with torch.no_grad():
            for p, p_targ in zip(self.actor_critic.parameters(), self.actor_critic_targ.parameters()):
                p_targ.data.mul_(self.polyak)
                p_targ.data.add_((1 - self.polyak) * p.data)
        return value_loss, surrogate_loss

    def _fused_minibatch(self, data):
        """One minibatch of the fused route; returns the two losses as 0-d device tensors.  No host read."""
        ac, targ = self.actor_critic, self.actor_critic_targ
        q_params = list(ac.q1.parameters()) + list(ac.q2.parameters())
        q_targets = list(targ.q1.parameters()) + list(targ.q2.parameters())
        pi_params = list(ac.pi.parameters())

        self.q_optimizer.zero_grad()
        loss_q = self.compute_loss_q(data)
        loss_q.backward()
        norm = self.q_optimizer.clip_and_step(self.max_grad_norm, also_norm=pi_params, targets=q_targets, polyak=self.polyak)
        self._rescale(q_params, norm)           # they meet grad(L_pi) in the policy step (freeze_q: they enter its norm as they are)

        for p in self.q_params:
            p.requires_grad = False
        self.pi_optimizer.zero_grad()
        loss_pi = self.compute_loss_pi(data)
        loss_pi.backward()
        norm = self.pi_optimizer.clip_and_step(self.max_grad_norm, also_norm=q_params, targets=list(targ.pi.parameters()), polyak=self.polyak)
        self._rescale(pi_params, norm)          # the stale actor gradients of the next Q step's norm
        for p in self.q_params:
            p.requires_grad = True
        return loss_q.detach(), loss_pi.detach()

    def _pi(self, o):
        if self.eps_source is None:
            return self.actor_critic.pi(o)
        return self.actor_critic.pi(o, eps=self.eps_source(tuple(o.shape[:-1]) + tuple(self.action_space.shape)))

    def compute_loss_q(self, data):
        o, a, r, o2, d = data['obs'], data['act'], data['r'], data['obs2'], data['done']
        if self.fused_update:
            with torch.no_grad():
                a2, logp_a2 = self._pi(o2)       # target actions come from the CURRENT policy
                backup = self.actor_critic_targ.q_backup(o2, a2, r, d, self.gamma, self.entropy_coef, logp_a2)
            return self.actor_critic.q_loss(o, a, backup)
        q1 = self.actor_critic.q1(o, a)
        q2 = self.actor_critic.q2(o, a)
        with torch.no_grad():
            a2, logp_a2 = self._pi(o2)
            q1_pi_targ = self.actor_critic_targ.q1(o2, a2)
            q2_pi_targ = self.actor_critic_targ.q2(o2, a2)
            q_pi_targ = torch.min(q1_pi_targ, q2_pi_targ)
            backup = r + self.gamma * (1 - d) * (q_pi_targ - self.entropy_coef * logp_a2)
        loss_q1 = ((q1 - backup) ** 2).mean()
        loss_q2 = ((q2 - backup) ** 2).mean()
        return loss_q1 + loss_q2

    def compute_loss_pi(self, data):
        o = data['obs']
        if self.fused_update and self.eps_source is None:
            return self.actor_critic.pi_loss(o, self.entropy_coef)
        pi, logp_pi = self._pi(o)
        q1_pi = self.actor_critic.q1(o, pi)
        q2_pi = self.actor_critic.q2(o, pi)
        q_pi = torch.min(q1_pi, q2_pi)
        return (self.entropy_coef * logp_pi - q_pi).mean()

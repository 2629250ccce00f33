"""PPO, the learner (agents/algorithms/rl/ppo/ppo.py): the reference's constructor, attributes, `learn` config keys and methods (`run`,
`update`, `log`, `save`, `load`, `test`) over this package's ActorCritic and RolloutStorage, so `process_sarl`'s PPO branch trains
without the reference tree.  The loop, the log and the checkpoint methods are on_policy.OnPolicyLearner's, shared with TRPO.

The default route of `update()` is ppo.py:243-317 statement for statement: `evaluate` on the gathered rows, the adaptive-KL schedule
with its comparison on the host, the clipped surrogate, the (clipped) value loss, the entropy term, `clip_grad_norm_` over all
parameters and Adam, one `.item()` per loss and minibatch.

New `learn` key `fused_update` (False).  True: the optimizer is a `FusedAdam`; a minibatch is `ActorCritic.ppo_loss` (mms_ppo_loss:
the KL, the loss and its gradients with respect to the networks' outputs in one launch over the storage's fields, read where they lie
through the index vector), the schedule's ONE read of kl, `backward()` and `FusedAdam.clip_and_step(max_grad_norm)` (mms_param_step:
the norm, the clip and Adam in two launches; the stored gradients are not rewritten, and nothing reads them again).  The two running
losses add up on the device and are read once per `update()`.  `_fused_loss` alone -- the gather, both networks and the loss head --
launches device work only and can be captured in a graph; the schedule's read follows it.

`trace` (attribute, None): a list that receives one dict per minibatch -- the loss and its two terms, kl (where the schedule reads it), the norm
before clipping and the step size -- for tests that replay a recorded update."""
import torch
import torch.nn as nn
import torch.optim as optim

from ....optim import FusedAdam
from ..on_policy import OnPolicyLearner
from .module import ActorCritic
from .storage import RolloutStorage


class PPO(OnPolicyLearner):
    def __init__(self, vec_env, cfg_train, device='cpu', sampler='sequential', log_dir='run', is_testing=False, print_log=True, apply_reset=False,
                 asymmetric=False):
        learn_cfg = self._init_common(vec_env, cfg_train, device, sampler, log_dir, is_testing, print_log, apply_reset, asymmetric, ActorCritic,
                                      RolloutStorage)
        self.desired_kl = learn_cfg.get("desired_kl", None)
        self.fused_update = bool(learn_cfg.get("fused_update", False))
        optimizer = FusedAdam if self.fused_update else optim.Adam
        self.optimizer = optimizer(self.actor_critic.parameters(), lr=self.learning_rate)

        # PPO parameters
        self.clip_param = learn_cfg["cliprange"]
        self.num_learning_epochs = learn_cfg["noptepochs"]
        self.num_mini_batches = learn_cfg["nminibatches"]
        self.value_loss_coef = learn_cfg.get("value_loss_coef", 2.0)
        self.entropy_coef = learn_cfg["ent_coef"]
        self.gamma = learn_cfg["gamma"]
        self.lam = learn_cfg["lam"]
        self.max_grad_norm = learn_cfg.get("max_grad_norm", 2.0)
        self.use_clipped_value_loss = learn_cfg.get("use_clipped_value_loss", False)
        self.trace = None
        self._init_log(log_dir, print_log, is_testing, apply_reset)

    # ---- the update ----------------------------------------------------------------------------------------------------------------

    def update(self):
        mean_value_loss = 0
        mean_surrogate_loss = 0
        batch = self.storage.mini_batch_generator(self.num_mini_batches)
        step = self._fused_minibatch if self.fused_update else self._minibatch
        for epoch in range(self.num_learning_epochs):
            for indices in batch:
                value_loss, surrogate_loss = step(indices)
                mean_value_loss = mean_value_loss + value_loss
                mean_surrogate_loss = mean_surrogate_loss + surrogate_loss
        num_updates = self.num_learning_epochs * self.num_mini_batches
        if self.fused_update:                   # the one host read of the two sums
            mean_value_loss, mean_surrogate_loss = torch.stack([torch.as_tensor(v, dtype=torch.float32, device=self.device)
                                                                for v in (mean_value_loss, mean_surrogate_loss)]).tolist()
        return mean_value_loss / num_updates, mean_surrogate_loss / num_updates

    def _adapt_step_size(self, kl_mean):
        """ppo.py:277-283: the adaptive schedule from the minibatch's mean KL (a 0-d tensor: the comparisons read it on the host)."""
        if kl_mean > self.desired_kl * 2.0:
            self.step_size = max(1e-5, self.step_size / 1.5)
        elif kl_mean < self.desired_kl / 2.0 and kl_mean > 0.0:
            self.step_size = min(1e-2, self.step_size * 1.5)
        for param_group in self.optimizer.param_groups:
            param_group['lr'] = self.step_size

    def _minibatch(self, indices):
        """One step of the default route (ppo.py:253-311); returns the two losses as host numbers."""
        b = self._gather(indices)
        actions_log_prob_batch, entropy_batch, value_batch, mu_batch, sigma_batch = self.actor_critic.evaluate(b['obs'], b['states'], b['actions'])

        kl_mean = None
        if self.desired_kl != None and self.schedule == 'adaptive':         # noqa: E711
            kl_mean = torch.mean(self._kl(sigma_batch, mu_batch, b))
            self._adapt_step_size(kl_mean)

        ratio = torch.exp(actions_log_prob_batch - torch.squeeze(b['old_logp']))
        surrogate = -torch.squeeze(b['adv']) * ratio
        surrogate_clipped = -torch.squeeze(b['adv']) * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
        surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
        value_loss = self._value_loss(value_batch, b)
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy_batch.mean()

        self.optimizer.zero_grad()
        loss.backward()
        norm = nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
        self.optimizer.step()
        if self.trace is not None:
            self.trace.append(dict(loss=loss.detach(), value_loss=value_loss.detach(), surrogate_loss=surrogate_loss.detach(), norm=norm.detach(), step_size=self.step_size,
                                   kl=None if kl_mean is None else kl_mean.detach()))
        return value_loss.item(), surrogate_loss.item()

    def _fused_loss(self, indices):
        """The gather of the observations, both networks and mms_ppo_loss: (loss, info).  Device work only."""
        s = self.storage
        obs = s.observations.view(-1, *s.observations.size()[2:])[indices]
        states = s.states.view(-1, *s.states.size()[2:])[indices] if self.asymmetric else None
        return self.actor_critic.ppo_loss(obs, states, s, indices, self.clip_param, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)

    def _fused_minibatch(self, indices):
        """One step of the fused route; returns the two losses as 0-d device tensors."""
        if not torch.is_tensor(indices):
            indices = torch.as_tensor(indices, dtype=torch.int64, device=self.device)
        loss, info = self._fused_loss(indices)
        if self.desired_kl != None and self.schedule == 'adaptive':         # noqa: E711
            self._adapt_step_size(info["kl"])                               # the schedule's read, where the reference has it
        self.optimizer.zero_grad()
        loss.backward()
        norm = self.optimizer.clip_and_step(self.max_grad_norm)
        if self.trace is not None:
            self.trace.append(dict(loss=loss.detach(), value_loss=info["value_loss"], surrogate_loss=info["surrogate"], norm=norm, step_size=self.step_size,
                                   kl=info["kl"]))
        return info["value_loss"], info["surrogate"]

"""MAPPO and HAPPO trainers with the update's loss head and its gradients in one call (loss.marl_ppo_loss / mms_marl_ppo_loss).

Drop-ins for the reference's trainers (agents/algorithms/marl/mappo_trainer.py: MAPPO, happo_trainer.py: HAPPO): the constructor
`(config, policy, device)`, the attributes (`policy`, `value_normalizer`, `clip_param`, ...), `ppo_update(sample, update_actor=True)`,
`train(buffer, update_actor=True)`, `prep_training`, `prep_rollout`, the returned tuples and the `train_info` keys are theirs, so a
runner that imports these classes in place of the reference's trains unchanged.

The policy is taken as it is: `policy.actor`, `.critic`, `.actor_optimizer`, `.critic_optimizer`, with the module attributes that
GroupedPolicyInference relies on (`.base.feature_norm`, `.base.mlp.fc1 / fc2`, `.act.action_out.{fc_mean, log_std, std_x_coef,
std_y_coef}`, `.v_out`).  An update runs actor.base -> fc_mean and critic.base -> v_out in torch, forms std from log_std, calls
marl_ppo_loss, does ONE backward() of the objective (the reference's two backward() calls reach disjoint parameter sets), clips the two
gradient norms separately and steps both optimizers.  Action spaces other than Box raise in the constructor; nothing falls back
silently.

Recurrent policies (use_recurrent_policy / use_naive_recurrent_policy) are accepted when `policy.actor.rnn` and `policy.critic.rnn` are
the reference's RNNLayer (`.rnn`, an nn.GRU, and `.norm`; agents/algorithms/utils/rnn.py:7-80); a policy without one raises.  An update
then runs `actor.rnn(features, rnn_states, masks)` and `critic.rnn(...)` -- the module's own forward, with its sequence branch
(rnn.py:30-77) and torch's backward through time -- between the bases and the heads, on the rows and the one state per sequence that
`recurrent_generator` (or `naive_recurrent_generator`) yields; `train` picks the generator as mappo_trainer.py:211-216 does and
the loss stays marl_ppo_loss on the gathered fields.  The rollout's side of it is GroupedPolicyInference (mms_gru_group).  The
generator hands the rows over as the reference's does (generators.py: chunk-major), and RNNLayer reads them as it does there.

`config["fused_rnn_update"]` (absent in the reference's configs; default False = the paragraph above, unchanged): the update runs
base -> rnn_seq.gru_sequence -> rnn.norm -> head instead -- the GRU of the actor and of the critic in grouped calls, the gate
arithmetic and its backward in HIP (mms_gru_gates_group, mms_gru_gates_grad_group), every product on the library, the mask applied at
every step, which for the buffers' 0 / 1 masks is RNNLayer's function without its host read of the masks and its one nn.GRU call per
piece (rnn_seq.py).  With update_actor=False the actor runs alone under no_grad.  The constructor raises NotImplementedError for
what gru_sequence refuses: a hidden size that is not a multiple of 4 or above 1024, an actor and a critic of unequal GRU shape, a
policy that is not recurrent.

`config["fused_block_update"]` (absent in the reference's configs; default False = unchanged): every MLPBase.forward of an update --
on the feed-forward route, the RNNLayer route and the fused_rnn_update route alike -- runs through blocks.mlp_base instead: per block
level one library product per network and ONE grouped call for the ELU, the LayerNorm and the rows' statistics
(mms_elu_ln_group), their backward with the bias, gamma and beta gradients in one call as well (mms_elu_ln_grad_group), two [M, H]
tensors less saved per block.  With update_actor=True the actor and the critic share the grouped calls; with update_actor=False
the actor runs alone under no_grad.  The constructor raises NotImplementedError for what mlp_base refuses (blocks.check_blocks): a block
that is not Linear with bias + ELU(alpha=1) + affine LayerNorm, differing eps, a hidden width that is not a multiple of 4 or above
1024, non-fp32 parameters, an actor and a critic of unequal width or depth.

`config["block_products"]` (absent in the reference's configs; "library" = the paragraph above, unchanged, or "f16x2"): who forms the
forward products z = x W^T of those blocks.  "f16x2" sends them to the two-plane fp16 layer kernel of the collect paths
(mms_linear_group_act_split16), all networks of a level in one launch, with mms_elu_ln_planes16_group leaving each level's output as
the next level's operand planes (blocks.py); the backward and what is saved stay as they are.  It applies on all three routes, since
all of them go through mlp_base.  It needs fused_block_update (NotImplementedError without it), a hidden width that is a multiple of
128 (NotImplementedError in the constructor) and minibatches whose row count is a multiple of 128 (NotImplementedError at the call,
naming M); any other value raises ValueError.  HATRPO does not read the key.

`config["fused_head_update"]` (absent in the reference's configs; default False = unchanged): the three places that form mu, std and the
values -- the feed-forward and RNNLayer routes of `_update`, `_fused_rnn_forward` and `train_group` -- run fc_mean, the std expression and
v_out through heads.update_heads instead: ONE mms_marl_heads_fwd_group call for the heads of a step and ONE mms_marl_heads_grad_group
call for their backward (df, dW, db, dlog_std; sums in double in a fixed order), in place of two addmm, three element-wise launches and,
backward, four products, two column sums and the std expression's backward per agent.  The recurrent routes hand over the output of
rnn.norm.  With update_actor=False the actor's features are formed under no_grad and its head is left out of the backward call.  The
constructor raises NotImplementedError for what update_heads refuses (heads.check_heads): more than 16 actions, a hidden width that is
not a multiple of 4 or above 1024, non-fp32 parameters, a head without a bias.  HATRPO does not read the key.

`MAPPO.train_group(trainers, buffers)` (no counterpart in the reference; what Runner's `grouped_update` calls): train() of several MAPPO
trainers in lockstep, one loss.marl_ppo_loss_group call per minibatch step for all of them and the bases of all in grouped mlp_base
calls; the permutations are drawn in the order of the loop over `trainer.train(buffer)` and every network runs through the same
functions, so it leaves what that loop leaves.  It needs fused_block_update and one configuration and shape for all trainers.

`ppo_update` takes the reference's gathered tuple.  `train` draws the permutation exactly as feed_forward_generator does
(torch.randperm(batch), the same slices), gathers only the network inputs (share_obs, obs) and the returns the normaliser's batch
moments need, and hands the index vector and the buffer's own tensors to the loss: under the same torch seed it equals a loop of
ppo_update over buffer.feed_forward_generator bit for bit.

The reference is mirrored as it runs:
  * MAPPO.cal_value_loss forms the errors in its `use_valuenorm` branch and then overwrites them in the `else` of `if self._use_popart`:
    with ValueNorm the normaliser is updated, but the targets are the raw returns.  Here too.
  * HAPPO's loss looks at `use_popart` only (no ValueNorm).
  * With PopArt, cal_value_loss calls the normaliser's forward twice on the same returns (once per error), so its statistics take each
    minibatch in twice.  Here too; the entry takes one (mean, var), the statistics after both updates -- what the reference's unclipped
    error is formed with.  This is a deviation from the reference wherever the clipped error is the selected one: the reference forms
    it with the statistics BETWEEN the two updates.  The second update moves the debiased mean by
    (1 - beta) (batch mean - mean) / debiasing term, the mean of squares likewise: nothing on a fresh normaliser (its first update
    already gives the batch's own moments; every test of this path starts there, so none sees the deviation), about
    (batch mean - mean) / (n + 2) after n earlier updates while n << 1 / (1 - beta) = 1e5 -- with returns that drift between rollouts
    this is well above fp32 rounding in the first rollouts of a run -- and 1e-5 (batch mean - mean) on a settled one.  It touches the
    clipped error's target only, by that shift over sqrt(var), and thereby which of the two losses a row near a tie selects.
  * Both advantage preparations of train() are the reference's, in torch: returns minus (denormalised) value predictions, normalised by
    their mean and std over the whole buffer.
  * `imp_weights`, the last element of ppo_update's tuple, is the [M, 1] tensor of ratios in the reference, of which train() takes
    .mean(); here it is that mean, a device scalar (its .mean() is itself)."""
import contextlib
import math

import torch
import torch.nn as nn

from ...optim import FusedAdam
from .loss import marl_ppo_loss, marl_ppo_loss_group
from .blocks import MAX_GROUPS, check_blocks, mlp_base
from .heads import check_heads, update_heads
from .rnn_seq import check_grus, gru_sequence
from .utils.valuenorm import ValueNorm


def _rows(x):
    return x.reshape(-1, *x.shape[2:])


def _base(base, x):
    """MLPBase.forward (agents/algorithms/utils/mlp.py:59-66, 31-35) from the module's attributes."""
    if getattr(base, "_use_feature_normalization", hasattr(base, "feature_norm")):
        x = base.feature_norm(x)
    x = base.mlp.fc1(x)
    for layer in base.mlp.fc2:
        x = layer(x)
    return x


def _grad_if(flag):
    """The context of an actor's forward: as it is where the actor is updated, no_grad where it is not"""
    return contextlib.nullcontext() if flag else torch.no_grad()


def _is_rnn_layer(layer):
    return isinstance(getattr(layer, "rnn", None), nn.GRU) and isinstance(getattr(layer, "norm", None), nn.LayerNorm)


def get_grad_norm(params):
    """agents/utils/util.py:8-15 (get_gard_norm)."""
    total = 0.0
    for p in params:
        if p.grad is not None:
            total += p.grad.norm() ** 2
    return math.sqrt(total)


class _Trainer:
    _has_valuenorm = False          # MAPPO reads config["use_valuenorm"]; HAPPO does not
    _has_factor = False

    def __init__(self, config, policy, device=torch.device("cpu")):
        self.device = device
        self.tpdv = dict(dtype=torch.float32, device=device)
        self.policy = policy
        self.clip_param = config["clip_param"]
        self.ppo_epoch = config["ppo_epoch"]
        self.num_mini_batch = config["num_mini_batch"]
        self.data_chunk_length = config["data_chunk_length"]
        self.value_loss_coef = config["value_loss_coef"]
        self.entropy_coef = config["entropy_coef"]
        self.max_grad_norm = config["max_grad_norm"]
        self.huber_delta = config["huber_delta"]
        self._use_valuenorm = bool(config["use_valuenorm"]) if self._has_valuenorm else False
        self._use_recurrent_policy = config["use_recurrent_policy"]
        self._use_naive_recurrent = config["use_naive_recurrent_policy"]
        self._use_max_grad_norm = config["use_max_grad_norm"]
        self._use_clipped_value_loss = config["use_clipped_value_loss"]
        self._use_huber_loss = config["use_huber_loss"]
        self._use_popart = config["use_popart"]
        self._use_value_active_masks = config["use_value_active_masks"]
        self._use_policy_active_masks = config["use_policy_active_masks"]
        name = type(self).__name__
        assert not (self._use_popart and self._use_valuenorm), "self._use_popart and self._use_valuenorm can not be set True simultaneously"
        self._recurrent = bool(self._use_recurrent_policy or self._use_naive_recurrent)
        if self._recurrent and not (_is_rnn_layer(getattr(policy.actor, "rnn", None)) and _is_rnn_layer(getattr(policy.critic, "rnn", None))):
            raise NotImplementedError("%s: use_recurrent_policy / use_naive_recurrent_policy need policy.actor.rnn and policy.critic.rnn "
                                      "(RNNLayer: .rnn = nn.GRU, .norm = nn.LayerNorm)" % name)
        # opt-in (the reference's config has no such key): the recurrent update's GRU through rnn_seq.gru_sequence (module docstring)
        self._fused_rnn_update = bool(config.get("fused_rnn_update", False))
        if self._fused_rnn_update:
            if not self._recurrent:
                raise NotImplementedError("%s: fused_rnn_update needs use_recurrent_policy or use_naive_recurrent_policy" % name)
            check_grus([policy.actor.rnn.rnn, policy.critic.rnn.rnn], "%s: fused_rnn_update" % name)
        # opt-in (likewise): the bases' ELU + LayerNorm blocks through blocks.mlp_base (module docstring)
        self._fused_block_update = bool(config.get("fused_block_update", False))
        self._block_products = config.get("block_products", "library")
        if self._fused_block_update or self._block_products != "library":
            check_blocks([getattr(policy.actor, "base", None), getattr(policy.critic, "base", None)], "%s: fused_block_update" % name, self._block_products)
        if self._block_products != "library" and not self._fused_block_update:
            raise NotImplementedError("%s: block_products=%r needs fused_block_update" % (name, self._block_products))
        head = getattr(getattr(policy.actor, "act", None), "action_out", None)
        if head is None or not (hasattr(head, "fc_mean") and hasattr(head, "log_std")):
            raise NotImplementedError("%s: only Box action spaces (ACTLayer.action_out = DiagGaussian) are covered" % name)
        # opt-in (likewise): fc_mean, the std expression and v_out through heads.update_heads (module docstring)
        self._fused_head_update = bool(config.get("fused_head_update", False))
        if self._fused_head_update:
            check_heads([policy.actor], [policy.critic], "%s: fused_head_update" % name)
        self.value_normalizer = ValueNorm(1, device=self.device) if (self._use_popart or self._use_valuenorm) else None
        self.loss_fn = marl_ppo_loss            # (a benchmark swaps in marl_ppo_loss_torch)

    # -- one update -------------------------------------------------------------------------------------------------------------
    def _update(self, share_obs, obs, returns_rows, fields, indices, update_actor, rnn=None):
        """rnn: None, or (rnn_states, rnn_states_critic, masks) of a recurrent generator's sample"""
        actor, critic = self.policy.actor, self.policy.critic
        head = actor.act.action_out
        base = self._bases(share_obs, obs, update_actor)
        if rnn is None:
            features = lambda net, x, states: base(net, x)
        elif self._fused_rnn_update:
            return self._update_tail(*self._fused_rnn_forward(share_obs, obs, rnn, update_actor, base), returns_rows, fields, indices)
        else:
            features = lambda net, x, states: net.rnn(base(net, x), states, rnn[2])[0]             # actor_critic.py:64-65, 164-165
        if self._fused_head_update:
            fc = features(critic, share_obs, None if rnn is None else rnn[1])
            with _grad_if(update_actor):
                fa = features(actor, obs, None if rnn is None else rnn[0])
            return self._update_tail(*self._fused_heads(fa, fc, update_actor), returns_rows, fields, indices)
        values = critic.v_out(features(critic, share_obs, None if rnn is None else rnn[1]))
        if update_actor:
            mu = head.fc_mean(features(actor, obs, None if rnn is None else rnn[0]))
            std = torch.sigmoid(head.log_std / head.std_x_coef) * head.std_y_coef
        else:
            with torch.no_grad():
                mu = head.fc_mean(features(actor, obs, None if rnn is None else rnn[0]))
                std = torch.sigmoid(head.log_std / head.std_x_coef) * head.std_y_coef
        return self._update_tail(mu, std, values, returns_rows, fields, indices)

    def _bases(self, share_obs, obs, update_actor):
        """base(net, x): MLPBase.forward of the actor (on obs) or the critic (on share_obs).  Without fused_block_update the module's own
        layers where the caller asks for them; with it mlp_base up front: both networks in grouped calls, or the critic alone and
        the actor under no_grad when it is not updated"""
        if not self._fused_block_update:
            return lambda net, x: _base(net.base, x)
        actor, critic = self.policy.actor, self.policy.critic
        if update_actor:
            fa, fc = mlp_base([obs, share_obs], [actor.base, critic.base], self._block_products)
        else:
            fc, = mlp_base([share_obs], [critic.base], self._block_products)
            with torch.no_grad():
                fa, = mlp_base([obs], [actor.base], self._block_products)
        return lambda net, x: fa if net is actor else fc

    def _fused_heads(self, fa, fc, update_actor):
        """(mu, std, values) of this policy's two heads on the actor's features fa and the critic's fc through heads.update_heads"""
        mus, stds, values = update_heads([fa], [fc], [self.policy.actor], [self.policy.critic], update_actor)
        return mus[0], stds[0], values[0]

    def _fused_rnn_forward(self, share_obs, obs, rnn, update_actor, base):
        """(mu, std, values) with base -> gru_sequence -> rnn.norm -> head: the networks that need gradients in one grouped call, the actor
        alone under no_grad when it is not updated"""
        actor, critic = self.policy.actor, self.policy.critic
        head = actor.act.action_out
        if update_actor:
            (ya, _), (yc, _) = gru_sequence([base(actor, obs), base(critic, share_obs)], [rnn[0], rnn[1]], rnn[2], [actor.rnn.rnn, critic.rnn.rnn])
        else:
            (yc, _), = gru_sequence([base(critic, share_obs)], [rnn[1]], rnn[2], [critic.rnn.rnn])
            with torch.no_grad():
                (ya, _), = gru_sequence([base(actor, obs)], [rnn[0]], rnn[2], [actor.rnn.rnn])
        with _grad_if(update_actor):
            fa = actor.rnn.norm(ya)
            if not self._fused_head_update:
                mu = head.fc_mean(fa)
                std = torch.sigmoid(head.log_std / head.std_x_coef) * head.std_y_coef
        if self._fused_head_update:
            return self._fused_heads(fa, critic.rnn.norm(yc), update_actor)
        return mu, std, critic.v_out(critic.rnn.norm(yc))

    def _update_tail(self, mu, std, values, returns_rows, fields, indices):
        """The normaliser, the loss, one backward, the clips and the steps of one update"""
        norm = self._update_normalizer(returns_rows)
        objective, info = self.loss_fn(mu, std, values, *fields, clip_param=self.clip_param, value_loss_coef=self.value_loss_coef,
                                       entropy_coef=self.entropy_coef, huber_delta=self.huber_delta, use_huber_loss=self._use_huber_loss,
                                       use_clipped_value_loss=self._use_clipped_value_loss, use_policy_active_masks=self._use_policy_active_masks,
                                       use_value_active_masks=self._use_value_active_masks, norm_mean=norm[0], norm_var=norm[1], indices=indices)
        self.policy.actor_optimizer.zero_grad()
        self.policy.critic_optimizer.zero_grad()
        objective.backward()
        actor_grad_norm, critic_grad_norm = self._clip_and_step()
        return info["value_loss"], critic_grad_norm, info["policy_loss"], info["dist_entropy"], actor_grad_norm, info["ratio"]

    def _clip_and_step(self, grad_norm=get_grad_norm):
        """The two clips and the two steps behind a backward; returns (actor_grad_norm, critic_grad_norm).  grad_norm: what measures the
        norm where nothing clips (train_group passes the same sum without the host read)"""
        actor, critic = self.policy.actor, self.policy.critic
        if isinstance(self.policy.actor_optimizer, FusedAdam) and isinstance(self.policy.critic_optimizer, FusedAdam):
            # clip + step as one mms_param_step per network (optim.py; each optimizer holds its network's parameters, as the policies
            # build them); max_norm None: the norm is still computed and reported, nothing is clipped
            max_norm = self.max_grad_norm if self._use_max_grad_norm else None
            actor_grad_norm = self.policy.actor_optimizer.clip_and_step(max_norm)
            critic_grad_norm = self.policy.critic_optimizer.clip_and_step(max_norm)
            return actor_grad_norm, critic_grad_norm
        if self._use_max_grad_norm:
            actor_grad_norm = nn.utils.clip_grad_norm_(actor.parameters(), self.max_grad_norm)
            critic_grad_norm = nn.utils.clip_grad_norm_(critic.parameters(), self.max_grad_norm)
        else:
            actor_grad_norm = grad_norm(actor.parameters())
            critic_grad_norm = grad_norm(critic.parameters())
        self.policy.actor_optimizer.step()
        self.policy.critic_optimizer.step()
        return actor_grad_norm, critic_grad_norm

    def _update_normalizer(self, returns_rows):
        """The normaliser's updates of one minibatch; returns the (mean, variance) the loss normalises the targets with, or (None, None)"""
        norm = (None, None)
        if self._use_valuenorm:
            self.value_normalizer.update(returns_rows)                 # ... and the targets stay raw (module docstring)
        if self._use_popart:
            self.value_normalizer.update(returns_rows)
            self.value_normalizer.update(returns_rows)
            norm = self.value_normalizer.running_mean_var()
        return norm

    def _advantages(self, buffer):
        """train()'s normalised advantages of a buffer, [T, N, 1] contiguous"""
        if self.value_normalizer is not None:
            advantages = buffer.returns[:-1] - self.value_normalizer.denormalize(buffer.value_preds[:-1])
        else:
            advantages = buffer.returns[:-1] - buffer.value_preds[:-1]
        advantages_copy = advantages.clone()
        mean_advantages = torch.mean(advantages_copy)
        std_advantages = torch.std(advantages_copy)
        return ((advantages - mean_advantages) / (std_advantages + 1e-5)).contiguous()

    def ppo_update(self, sample, update_actor=True):
        """One update from the generators' gathered tuple; returns (value_loss, critic_grad_norm, policy_loss, dist_entropy,
        actor_grad_norm, imp_weights) -- imp_weights: the mean ratio (module docstring)."""
        share_obs, obs, rnn_states, rnn_states_critic, actions, value_preds, returns, masks, active_masks, old_logp, adv = sample[:11]
        cast = lambda x: torch.as_tensor(x).to(**self.tpdv)
        factor = cast(sample[12]) if self._has_factor else None
        fields = (cast(actions), cast(old_logp), cast(adv), cast(value_preds), cast(returns), cast(active_masks), factor)
        rnn = (cast(rnn_states), cast(rnn_states_critic), cast(masks)) if self._recurrent else None
        return self._update(cast(share_obs), cast(obs), fields[4], fields, None, update_actor, rnn)

    def train(self, buffer, update_actor=True):
        """The reference's train(): ppo_epoch passes over num_mini_batch random minibatches of the buffer; returns train_info."""
        advantages = self._advantages(buffer)
        train_info = {k: 0 for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio")}
        if self._recurrent:                                            # mappo_trainer.py:210-227 with the recurrent generators
            for _ in range(self.ppo_epoch):
                if self._use_recurrent_policy:
                    generator = buffer.recurrent_generator(advantages, self.num_mini_batch, self.data_chunk_length)
                else:
                    generator = buffer.naive_recurrent_generator(advantages, self.num_mini_batch)
                for sample in generator:
                    value_loss, critic_grad_norm, policy_loss, dist_entropy, actor_grad_norm, imp_weights = self.ppo_update(sample, update_actor)
                    train_info["value_loss"] += value_loss.item()
                    train_info["policy_loss"] += policy_loss.item()
                    train_info["dist_entropy"] += dist_entropy.item()
                    train_info["actor_grad_norm"] += actor_grad_norm
                    train_info["critic_grad_norm"] += critic_grad_norm
                    train_info["ratio"] += imp_weights.mean()
            for k in train_info.keys():
                train_info[k] /= self.ppo_epoch * self.num_mini_batch
            return train_info
        T, N = buffer.rewards.shape[0:2]
        batch = T * N
        assert batch >= self.num_mini_batch, ("PPO requires the number of processes (%d) * number of steps (%d) = %d to be greater than or "
                                              "equal to the number of PPO mini batches (%d)." % (N, T, batch, self.num_mini_batch))
        mini_batch_size = batch // self.num_mini_batch
        fields = (buffer.actions, buffer.action_log_probs, advantages, buffer.value_preds, buffer.returns, buffer.active_masks,
                  buffer.factor if self._has_factor else None)
        share_rows, obs_rows, return_rows = _rows(buffer.share_obs[:-1]), _rows(buffer.obs[:-1]), _rows(buffer.returns[:-1])
        for _ in range(self.ppo_epoch):
            perm = torch.randperm(batch)                               # feed_forward_generator's draw and slices (generators.py)
            for b in range(self.num_mini_batch):
                idx = perm[b * mini_batch_size:(b + 1) * mini_batch_size].to(buffer.rewards.device)
                value_loss, critic_grad_norm, policy_loss, dist_entropy, actor_grad_norm, imp_weights = self._update(
                    share_rows[idx], obs_rows[idx], return_rows[idx], fields, idx, update_actor)
                train_info["value_loss"] += value_loss.item()
                train_info["policy_loss"] += policy_loss.item()
                train_info["dist_entropy"] += dist_entropy.item()
                train_info["actor_grad_norm"] += actor_grad_norm
                train_info["critic_grad_norm"] += critic_grad_norm
                train_info["ratio"] += imp_weights.mean()
        num_updates = self.ppo_epoch * self.num_mini_batch
        for k in train_info.keys():
            train_info[k] /= num_updates
        return train_info

    def prep_training(self):
        self.policy.actor.train()
        self.policy.critic.train()

    def prep_rollout(self):
        self.policy.actor.eval()
        self.policy.critic.eval()


def _grad_norm_on_device(params):
    """get_grad_norm without its host read: the same sum, its root in double on the device (math.sqrt takes the sum as a double too)"""
    total = 0.0
    for p in params:
        if p.grad is not None:
            total += p.grad.norm() ** 2
    return torch.sqrt(total.double()) if torch.is_tensor(total) else total


_GROUP_KEYS = ("clip_param", "ppo_epoch", "num_mini_batch", "value_loss_coef", "entropy_coef", "max_grad_norm", "huber_delta", "_use_valuenorm",
               "_use_popart", "_use_max_grad_norm", "_use_clipped_value_loss", "_use_huber_loss", "_use_value_active_masks", "_use_policy_active_masks",
               "_block_products", "_fused_head_update")


def _check_group(trainers, buffers):
    """What MAPPO.train_group takes (its docstring), or NotImplementedError; nothing is changed"""
    who = "MAPPO.train_group"
    if not trainers or len(trainers) != len(buffers):
        raise ValueError("%s: one buffer per trainer, at least one" % who)
    first = trainers[0]
    shapes = None
    for t, b in zip(trainers, buffers):
        if type(t) is not MAPPO:
            raise NotImplementedError("%s: MAPPO trainers only (HAPPO's and HATRPO's agents are sequential: each surrogate carries the factor of those "
                                      "updated before it), got %s" % (who, type(t).__name__))
        if t._recurrent:
            raise NotImplementedError("%s: feed-forward policies only (a recurrent minibatch is a set of sequences, not of rows)" % who)
        if not t._fused_block_update:
            raise NotImplementedError("%s: every trainer needs fused_block_update (the grouped step runs the bases through blocks.mlp_base)" % who)
        if t.loss_fn is not marl_ppo_loss:
            raise NotImplementedError("%s: a trainer's loss_fn was replaced; the grouped step evaluates loss.marl_ppo_loss_group" % who)
        for k in _GROUP_KEYS:
            if getattr(t, k) != getattr(first, k):
                raise NotImplementedError("%s: one configuration for all trainers; %s differs (%r, %r)" % (who, k.lstrip("_"), getattr(first, k), getattr(t, k)))
        actor, critic = t.policy.actor, t.policy.critic
        sig = (check_blocks([actor.base, critic.base], who, t._block_products), actor.base.mlp.fc1[0].in_features, critic.base.mlp.fc1[0].in_features,
               tuple(b.actions.shape), tuple(b.obs.shape), tuple(b.share_obs.shape), b.rewards.device, t.device)
        if shapes is None:
            shapes = sig
        elif sig != shapes:
            raise NotImplementedError("%s: one set of shapes for all trainers (hidden width, blocks, observation widths, actions, T, N, device): %r against %r"
                                      % (who, shapes, sig))
    T, N = buffers[0].rewards.shape[0:2]
    if T * N < first.num_mini_batch:
        raise NotImplementedError("%s: fewer rows (%d) than minibatches (%d)" % (who, T * N, first.num_mini_batch))


def _train_group(trainers, buffers, update_actor):
    trainers, buffers = list(trainers), list(buffers)
    _check_group(trainers, buffers)
    first, G = trainers[0], len(trainers)
    T, N = buffers[0].rewards.shape[0:2]
    batch = T * N
    mini_batch_size = batch // first.num_mini_batch
    device = buffers[0].rewards.device
    advantages = [t._advantages(b) for t, b in zip(trainers, buffers)]
    # the sequential loop's draws, in its order: trainer by trainer, one permutation per epoch
    perms = [[torch.randperm(batch) for _ in range(first.ppo_epoch)] for _ in trainers]
    fields = [(b.actions, b.action_log_probs, adv, b.value_preds, b.returns, b.active_masks, None) for b, adv in zip(buffers, advantages)]
    rows = [(_rows(b.share_obs[:-1]), _rows(b.obs[:-1]), _rows(b.returns[:-1])) for b in buffers]
    actors, critics = [t.policy.actor for t in trainers], [t.policy.critic for t in trainers]
    heads = [a.act.action_out for a in actors]
    products = first._block_products

    def bases(xs, nets):
        out = []
        for i in range(0, len(nets), MAX_GROUPS):                     # (mlp_base takes 32 networks per call)
            out += mlp_base(xs[i:i + MAX_GROUPS], [n.base for n in nets[i:i + MAX_GROUPS]], products)
        return out

    def actor_outputs(fa):
        return ([h.fc_mean(f) for h, f in zip(heads, fa)], [torch.sigmoid(h.log_std / h.std_x_coef) * h.std_y_coef for h in heads])

    sums = None                                                         # per key a [G] accumulator on the device
    for e in range(first.ppo_epoch):
        for b in range(first.num_mini_batch):
            idx = [p[e][b * mini_batch_size:(b + 1) * mini_batch_size].to(device) for p in perms]
            share = [r[0][i] for r, i in zip(rows, idx)]
            obs = [r[1][i] for r, i in zip(rows, idx)]
            if update_actor:                                            # actor and critic of an agent side by side, as _bases pairs them
                both = bases([x for pair in zip(obs, share) for x in pair], [n for pair in zip(actors, critics) for n in pair])
                fa, fc = both[0::2], both[1::2]
            else:
                fc = bases(share, critics)
                with torch.no_grad():
                    fa = bases(obs, actors)
            if first._fused_head_update:                                # all 2 G heads in one call (chunks of 32), their backward in one as well
                mus, stds, values = update_heads(fa, fc, actors, critics, update_actor)
            else:
                with _grad_if(update_actor):
                    mus, stds = actor_outputs(fa)
                values = [c.v_out(f) for c, f in zip(critics, fc)]
            norms = [t._update_normalizer(r[2][i]) for t, r, i in zip(trainers, rows, idx)]
            objectives, info = marl_ppo_loss_group(mus, stds, values, fields, clip_param=first.clip_param, value_loss_coef=first.value_loss_coef,
                                                   entropy_coef=first.entropy_coef, huber_delta=first.huber_delta, use_huber_loss=first._use_huber_loss,
                                                   use_clipped_value_loss=first._use_clipped_value_loss,
                                                   use_policy_active_masks=first._use_policy_active_masks, use_value_active_masks=first._use_value_active_masks,
                                                   norms=norms if first._use_popart else None, indices=idx)
            for t in trainers:
                t.policy.actor_optimizer.zero_grad()
                t.policy.critic_optimizer.zero_grad()
            torch.stack(objectives).sum().backward()                    # (every objective receives the gradient 1, as objective.backward() gives it)
            steps = [t._clip_and_step(_grad_norm_on_device) for t in trainers]
            # (clip_grad_norm_ over parameters without a gradient returns a host zero: update_actor=False)
            as_row = lambda xs: torch.stack([x.to(device) if torch.is_tensor(x) else torch.tensor(x, dtype=torch.float64, device=device) for x in xs])
            # train()'s sums: the three .item() values add as Python floats (doubles), the norms and the ratio in the type they come in
            step = {"value_loss": info["value_loss"].double(), "policy_loss": info["policy_loss"].double(), "dist_entropy": info["dist_entropy"].double(),
                    "actor_grad_norm": as_row([s[0] for s in steps]), "critic_grad_norm": as_row([s[1] for s in steps]), "ratio": info["ratio"]}
            sums = step if sums is None else {k: sums[k] + v for k, v in step.items()}
    num_updates = first.ppo_epoch * first.num_mini_batch
    keys = ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio")
    table = torch.stack([(sums[k] / num_updates).double() for k in keys]).cpu()          # the one host read
    return [{k: float(table[j, g]) for j, k in enumerate(keys)} for g in range(G)]


class MAPPO(_Trainer):
    """agents/algorithms/marl/mappo_trainer.py: MAPPO (module docstring)."""
    _has_valuenorm = True

    @staticmethod
    def train_group(trainers, buffers, update_actor=True):
        """train() of several MAPPO trainers in lockstep: MAPPO's agents do not depend on each other (no factor in the surrogate), so one
        (epoch, minibatch) step of all of them is the bases in grouped calls of up to 32 networks, ONE loss.marl_ppo_loss_group call,
        one backward of the objectives' sum and each policy's own clips and steps; the gathers, feature_norm, the two heads (with
        fused_head_update: all 2 G of them in one heads.update_heads call) and the normalisers stay per agent.  Returns the
        train_info dictionaries in the trainers' order, their values train()'s under float();
        the statistics add up on the device and are read once, behind the last step.
        The permutations are drawn as the loop `for t, b: t.train(b)` draws them (trainer by trainer, one per epoch), so every agent sees
        the minibatches it would have seen there and torch's generator ends in the same state; every network runs through the same
        functions on the same values, so parameters, optimizer states and normalisers end as that loop leaves them.
        Taken: feed-forward policies, fused_block_update on, one configuration (scalars, flags, block_products) and one set of shapes
        for all trainers.  Anything else raises NotImplementedError before anything is drawn or changed."""
        return _train_group(trainers, buffers, update_actor)


class HAPPO(_Trainer):
    """agents/algorithms/marl/happo_trainer.py: HAPPO: the surrogate carries the buffer's factor; PopArt or no normaliser."""
    _has_factor = True

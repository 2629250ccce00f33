"""HATRPO trainer (agents/algorithms/marl/hatrpo_trainer.py: HATRPO) with the KL's Fisher-vector product on this build's kernels.

A drop-in for the reference's class: the constructor `(config, policy, device)`, the attributes (`kl_threshold`, `ls_step`,
`accept_ratio`, `clip_param`, `value_normalizer`, ...), `trpo_update(sample, update_actor=True)` with its 7-tuple
`(value_loss, critic_grad_norm, kl, loss_improve, expected_improve, dist_entropy, ratio)`, `train(buffer, update_actor=True)` with
the reference's `train_info` keys, `prep_training` and `prep_rollout`.  The policy is taken as the MAPPO / HAPPO trainers take it
(trainer.py): `policy.actor`, `.critic`, `.critic_optimizer` and the module attributes GroupedPolicyInference relies on.

The reference is mirrored as it runs:
  * the critic updates first; its value loss is marl_ppo_loss's value terms, looking at `use_popart` only (as HAPPO; with PopArt the
    normaliser takes each minibatch in twice, trainer.py's docstring);
  * the surrogate is mean(ratio factor adv), or its policy-mask variant, and it is maximised;
  * conjugate gradient: 10 steps, residual_tol 1e-10, damping 0.1 p; step_size = 1 / sqrt(shs / kl_threshold);
  * the line search halves `fraction` and `expected_improve`, accepts on the reference's three-part test, restores the old parameters
    and prints the reference's message when no try is accepted; parameters are written through `.data.copy_`, which moves no version
    counter (GroupedPolicyInference refreshes at step 0 of every rollout for that reason);
  * `loss_improve`, `kl`, `ratio` and `dist_entropy` are those of the last line-search try; `update_actor` is accepted and not looked
    at, as in the reference.
What is different: no second Actor is constructed -- the old policy is the saved (mu_old, std_old) pair, which is all the KL reads.

`fvp` selects how a Fisher-vector product is formed:
  "autograd"  the reference's expression (hatrpo_trainer.py:170-179): the KL between the actor and itself, `autograd.grad` with
              create_graph, then `autograd.grad` of the gradient's dot product with p -- two forwards, a backward and a double backward
              per product, thirteen times per minibatch.  The yardstick, and the path for whatever the kernels do not take.
  "fisher"    the same product in closed form.  The reference always passes new_actor = old_actor = actor, so mu_old - mu is exactly
              zero, the KL's Hessian is exactly the Fisher matrix
                  H p = J^T diag(1 / (M std_j^2)) J p   over every parameter that feeds mu
                      + 2 ((1 - sigmoid(log_std / x_coef)) / x_coef)^2 p   on log_std, per action dimension
              (J: the Jacobian of mu; the curvature term multiplies dKL/dmu = 0 and the mu - log_std block multiplies mu - mu_old = 0),
              and one product is mms_ln_mlp_jvp (J p, scaled by 1 / (M std^2) on the way out) followed by mms_ln_mlp_grad (J^T of it),
              over the activations of ONE forward per minibatch that the actor gradient and all 12 products share.  It raises in the
              constructor for what the entries do not take (recurrent policies, no feature_norm, a block that is not
              Linear + ELU + LayerNorm, action spaces other than Box); nothing falls back silently.

The default is `DEFAULT_FVP`, decided by measurement (tools/bench_hatrpo_update.py, profiles/hatrpo_update_bench.jsonl; one agent,
46 -> 512 x 3 -> 8, one MI355X, medians with the spread of seven repeats): see the figures next to it below.

The [M, A] tail (log-probability, ratio, surrogate, the line search's KL) is torch in both modes."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib
from ...optim import FusedAdam
from .loss import HALF_LOG_2PI, _p, _workspace, marl_ppo_loss
from .trainer import _base, get_grad_norm
from .utils.valuenorm import ValueNorm

# Measured on one MI355X (profiles/hatrpo_update_bench.jsonl; medians, min - max of the repeats in brackets), 32768 rows:
#   one Fisher-vector product   autograd 11.52 ms [11.47 - 11.60]   fisher 6.86 ms [6.79 - 6.90]    (1.68 x)
#   one whole trpo_update       autograd 134.1 ms [133.9 - 134.2]   fisher 85.1 ms [85.0 - 85.2]    (1.58 x)
# and 640 rows: 3.32 against 1.02 ms per product, 40.1 against 14.9 ms per update.  "fisher" is faster than "autograd" by far more than
# the spread of either series, so it is the default.  What the saving is made of: the same algebra in plain torch ops (the tool's
# `fisher-torch` series) takes 4.18 ms per product and 52.9 ms per update at 32768 rows, 1.12 and 15.8 ms at 640 -- the algebra saves
# 2.5 - 2.8 x, and at 32768 rows the split-operand kernels give 0.6 x of that back against the library GEMMs (as TRPO's fused_grad
# did, rl/trpo/module.py); at 640 rows they are level with torch (1.1 x).
DEFAULT_FVP = "fisher"


_ptrs = _lib.ptr_array


class _ActorMap:
    """The actor's modules in the entries' order -- levels (LayerNorms) 0..L, Linear layers 1..L+1 (the last is fc_mean) -- and the slot
    of every parameter in `actor.parameters()`, the order of every flat vector here (log_std comes before fc_mean's weight)."""

    def __init__(self, actor):
        base, head = actor.base, actor.act.action_out
        if not getattr(base, "_use_feature_normalization", hasattr(base, "feature_norm")) or not hasattr(base, "feature_norm"):
            raise NotImplementedError("HATRPO(fvp='fisher'): the actor has no feature_norm (use_feature_normalization is off)")
        blocks = [base.mlp.fc1] + list(base.mlp.fc2)
        for b in blocks:
            if not (isinstance(b, nn.Sequential) and len(b) == 3 and isinstance(b[0], nn.Linear) and isinstance(b[1], nn.ELU) and b[1].alpha == 1.0
                    and isinstance(b[2], nn.LayerNorm) and b[0].bias is not None):
                raise NotImplementedError("HATRPO(fvp='fisher'): every hidden block must be Linear + ELU + LayerNorm")
        self.lns = [base.feature_norm] + [b[2] for b in blocks]
        self.lins = [b[0] for b in blocks] + [head.fc_mean]
        self.head = head
        if any(ln.weight is None or ln.bias is None or ln.eps != self.lns[0].eps or len(ln.normalized_shape) != 1 for ln in self.lns):
            raise NotImplementedError("HATRPO(fvp='fisher'): the LayerNorms must be affine over the last dimension with one eps")
        self.eps = float(self.lns[0].eps)
        self.dims = [self.lins[0].in_features] + [lin.out_features for lin in self.lins]
        self.blocks = len(blocks)
        if self.blocks > 7 or max(self.dims[:-1]) > 4096 or self.dims[-1] > 128:                 # include/mms.h: MMS_LN_MLP_MAX_*
            raise NotImplementedError("HATRPO(fvp='fisher'): at most 7 hidden blocks, widths up to 4096 and 128 actions")
        slots = {id(head.log_std): ("s", 0)}
        for l, ln in enumerate(self.lns):
            slots[id(ln.weight)], slots[id(ln.bias)] = ("g", l), ("t", l)
        for l, lin in enumerate(self.lins):
            slots[id(lin.weight)], slots[id(lin.bias)] = ("w", l), ("c", l)
        self.params = list(actor.parameters())
        if any(id(q) not in slots or q.dtype != torch.float32 for q in self.params) or len(self.params) != len(slots):
            raise NotImplementedError("HATRPO(fvp='fisher'): the actor has parameters besides feature_norm, the hidden blocks, fc_mean and log_std")
        self.order = [slots[id(q)] for q in self.params]
        self.numels = [q.numel() for q in self.params]
        self.total = sum(self.numels)

    def split(self, flat):
        """{kind: [tensor per level / layer]} views of a flat vector in actor.parameters() order."""
        out = {"g": [None] * len(self.lns), "t": [None] * len(self.lns), "w": [None] * len(self.lins), "c": [None] * len(self.lins), "s": [None]}
        for (kind, l), q, part in zip(self.order, self.params, flat.split(self.numels)):
            out[kind][l] = part.view(q.shape)
        return out

    def forward(self, x):
        """(mu, [h_1..h_L]): the actor's mean and the ELU outputs in front of every LayerNorm; no graph."""
        with torch.no_grad():
            hs = []
            u = F.layer_norm(x, (x.shape[-1],), self.lns[0].weight, self.lns[0].bias, self.eps)
            for lin, ln in zip(self.lins[:-1], self.lns[1:]):
                h = F.elu(F.linear(u, lin.weight, lin.bias))
                hs.append(h)
                u = F.layer_norm(h, (h.shape[-1],), ln.weight, ln.bias, self.eps)
            return F.linear(u, self.lins[-1].weight, self.lins[-1].bias), hs


class LnMlpState:
    """One forward's saved state (x, h_l) with the two entries over it: `grad(g)` = J^T g and `jvp(p)` = J p (include/mms.h)."""

    def __init__(self, amap, x, hs):
        self.amap, self.x, self.hs = amap, x.contiguous(), [h.contiguous() for h in hs]
        self.M = x.shape[0]
        self.lib, self.idx, self.stream = _lib.for_device(x.device)
        self.dims = (ctypes.c_int32 * len(amap.dims))(*amap.dims)
        self.ln_g, self.ln_t = [ln.weight.data for ln in amap.lns], [ln.bias.data for ln in amap.lns]
        self.w = [lin.weight.data for lin in amap.lins]
        need = 0
        for fn, n in ((self.lib.mms_ln_mlp_grad, 10), (self.lib.mms_ln_mlp_jvp, 11)):
            nbytes = ctypes.c_int64(-1)
            _lib.check(fn(self.idx, amap.blocks, self.M, self.dims, amap.eps, *([None] * n), None, ctypes.byref(nbytes), self.stream), None,
                       "ln_mlp size query", self.lib)
            need = max(need, nbytes.value)
        self.ws_bytes = need

    def _head(self):
        return (self.idx, self.amap.blocks, self.M, self.dims, self.amap.eps, _p(self.x), _ptrs(self.hs), _ptrs(self.ln_g), _ptrs(self.ln_t), _ptrs(self.w))

    def _ws(self):
        return ctypes.c_void_p(_workspace(self.ws_bytes, self.x.device)), ctypes.byref(ctypes.c_int64(self.ws_bytes))

    def grad(self, g):
        """J^T g as a flat vector in actor.parameters() order; log_std's slot is zero (mu does not depend on it)."""
        out = torch.zeros(self.amap.total, device=g.device)
        d = self.amap.split(out)
        g = g.contiguous()
        _lib.check(self.lib.mms_ln_mlp_grad(*self._head(), _p(g), _ptrs(d["g"]), _ptrs(d["t"]), _ptrs(d["w"]), _ptrs(d["c"]), *self._ws(), self.stream),
                   None, "mms_ln_mlp_grad", self.lib)
        return out

    def jvp(self, p, col_scale=None):
        """J p [M, A] for a flat direction p in actor.parameters() order, column j times col_scale[j]."""
        v = self.amap.split(p.contiguous())
        rmu = torch.empty(self.M, self.amap.dims[-1], device=p.device)
        _lib.check(self.lib.mms_ln_mlp_jvp(*self._head(), _ptrs(v["g"]), _ptrs(v["t"]), _ptrs(v["w"]), _ptrs(v["c"]), _p(col_scale), _p(rmu), *self._ws(),
                                           self.stream), None, "mms_ln_mlp_jvp", self.lib)
        return rmu


def gaussian_kl(mu_old, std_old, mu, std):
    """hatrpo_trainer.py:137-148: D(pi_old || pi_new) per row, [M, 1]."""
    kl = torch.log(std) - torch.log(std_old) + (std_old.pow(2) + (mu_old - mu).pow(2)) / (2.0 * std.pow(2)) - 0.5
    return kl.sum(1, keepdim=True)


class HATRPO:
    """agents/algorithms/marl/hatrpo_trainer.py: HATRPO (module docstring)."""

    def __init__(self, config, policy, device=torch.device("cpu"), *, fvp=None):
        self.device = device
        self.tpdv = dict(dtype=torch.float32, device=device)
        self.policy = policy
        self.kl_threshold = config["kl_threshold"]
        self.ls_step = config["ls_step"]
        self.accept_ratio = config["accept_ratio"]
        self.clip_param = config["clip_param"]
        self.num_mini_batch = config["num_mini_batch"]
        self.data_chunk_length = config["data_chunk_length"]
        self.value_loss_coef = config["value_loss_coef"]
        self.entropy_coef = config["entropy_coef"]
        self.max_grad_norm = config["max_grad_norm"]
        self.huber_delta = config["huber_delta"]
        self._use_recurrent_policy = config["use_recurrent_policy"]
        self._use_naive_recurrent = config["use_naive_recurrent_policy"]
        self._use_max_grad_norm = config["use_max_grad_norm"]
        self._use_clipped_value_loss = config["use_clipped_value_loss"]
        self._use_huber_loss = config["use_huber_loss"]
        self._use_popart = config["use_popart"]
        self._use_value_active_masks = config["use_value_active_masks"]
        self._use_policy_active_masks = config["use_policy_active_masks"]
        self.fvp = DEFAULT_FVP if fvp is None else fvp
        if self.fvp not in ("fisher", "autograd"):
            raise ValueError("HATRPO: fvp must be 'fisher' or 'autograd', not %r" % (fvp,))
        if self._use_recurrent_policy or self._use_naive_recurrent:
            raise NotImplementedError("HATRPO: recurrent policies are not covered (use_recurrent_policy / use_naive_recurrent_policy)")
        head = getattr(getattr(policy.actor, "act", None), "action_out", None)
        if head is None or not (hasattr(head, "fc_mean") and hasattr(head, "log_std")):
            raise NotImplementedError("HATRPO: only Box action spaces (ACTLayer.action_out = DiagGaussian) are covered")
        self._map = _ActorMap(policy.actor) if self.fvp == "fisher" else None
        self.value_normalizer = ValueNorm(1, device=self.device) if self._use_popart else None
        self.last = {}                  # the last trpo_update's step_dir, full_step, loss_grad, tries and accepted (for tests and logs)

    # -- the [M, A] tail, in torch ---------------------------------------------------------------------------------------------------
    def _std(self, log_std=None):
        head = self.policy.actor.act.action_out
        return torch.sigmoid((head.log_std if log_std is None else log_std) / head.std_x_coef) * head.std_y_coef

    def _mean(self, obs):
        actor = self.policy.actor
        return actor.act.action_out.fc_mean(_base(actor.base, obs))

    def _surrogate(self, mu, std, actions, old_logp, adv, factor, masks):
        logp = -((actions - mu) ** 2) / (2 * std ** 2) - std.log() - HALF_LOG_2PI                  # FixedNormal.log_probs
        ratio = torch.exp((logp - old_logp).sum(dim=-1, keepdim=True))
        surr = torch.sum(ratio * factor * adv, dim=-1, keepdim=True)
        if self._use_policy_active_masks:
            return (surr * masks).sum() / masks.sum(), ratio
        return surr.mean(), ratio

    def _entropy(self, std, masks, rows):
        ent = 0.5 + HALF_LOG_2PI + std.log()                                                        # Normal.entropy, [A]
        if self._use_policy_active_masks:                                                           # act.py:218 against :220
            return (ent.expand(rows, -1) * masks).sum() / masks.sum()
        return ent.mean()

    # -- Fisher-vector products ------------------------------------------------------------------------------------------------------
    def _flat(self, grads):
        return torch.cat([g.contiguous().view(-1) for g in grads if g is not None])

    def _fvp_autograd(self, obs, p):
        """hatrpo_trainer.py:170-179 with new_actor = old_actor = actor."""
        params = list(self.policy.actor.parameters())
        mu, std = self._mean(obs), self._std()
        with torch.no_grad():
            mu_old, std_old = self._mean(obs), self._std()
        kl = gaussian_kl(mu_old, std_old, mu, std).mean()
        kl_grad = self._flat(torch.autograd.grad(kl, params, create_graph=True, allow_unused=True))
        hp = torch.autograd.grad((kl_grad * p).sum(), params, allow_unused=True)
        return self._flat(hp).data + 0.1 * p

    def _fvp_fisher(self, state, col_scale, s_curv, p):
        hp = state.grad(state.jvp(p, col_scale))
        s_at = self._map.order.index(("s", 0))
        off = sum(self._map.numels[:s_at])
        n = self._map.numels[s_at]
        hp[off:off + n] = s_curv * p[off:off + n]
        return hp + 0.1 * p

    def conjugate_gradient(self, fvp, b, nsteps, residual_tol=1e-10):
        """hatrpo_trainer.py:152-168."""
        x = torch.zeros(b.size()).to(device=self.device)
        r = b.clone()
        p = b.clone()
        rdotr = torch.dot(r, r)
        for _ in range(nsteps):
            _Avp = fvp(p)
            alpha = rdotr / torch.dot(p, _Avp)
            x += alpha * p
            r -= alpha * _Avp
            new_rdotr = torch.dot(r, r)
            betta = new_rdotr / rdotr
            p = r + betta * p
            rdotr = new_rdotr
            if rdotr < residual_tol:
                break
        return x

    def flat_params(self, model):
        return torch.cat([q.data.view(-1) for q in model.parameters()])

    def update_model(self, model, new_params):
        index = 0
        for q in model.parameters():
            n = q.numel()
            q.data.copy_(new_params[index:index + n].view(q.size()))
            index += n

    # -- one update ------------------------------------------------------------------------------------------------------------------
    def trpo_update(self, sample, update_actor=True):
        share_obs, obs, _, _, actions, value_preds, returns, _, active_masks, old_logp, adv = sample[:11]
        cast = lambda x: torch.as_tensor(x).to(**self.tpdv)
        share_obs, obs, actions, value_preds, returns, active_masks, old_logp, adv, factor = (
            cast(t) for t in (share_obs, obs, actions, value_preds, returns, active_masks, old_logp, adv, sample[12]))
        actor, critic = self.policy.actor, self.policy.critic
        head = actor.act.action_out
        M = obs.shape[0]

        # the one forward of the minibatch
        if self.fvp == "fisher":
            obs = obs.contiguous()
            mu_old, hs = self._map.forward(obs)
            state = LnMlpState(self._map, obs, hs)
        else:
            with torch.no_grad():
                mu_old = self._mean(obs)
        std_old = self._std().detach()

        # critic update
        values = critic.v_out(_base(critic.base, share_obs))
        norm = (None, None)
        if self._use_popart:
            self.value_normalizer.update(returns)
            self.value_normalizer.update(returns)
            norm = self.value_normalizer.running_mean_var()
        objective, info = marl_ppo_loss(mu_old, std_old, values, actions, old_logp, adv, value_preds, returns, active_masks, factor,
                                        clip_param=self.clip_param, value_loss_coef=self.value_loss_coef, entropy_coef=self.entropy_coef,
                                        huber_delta=self.huber_delta, use_huber_loss=self._use_huber_loss,
                                        use_clipped_value_loss=self._use_clipped_value_loss, use_policy_active_masks=self._use_policy_active_masks,
                                        use_value_active_masks=self._use_value_active_masks, norm_mean=norm[0], norm_var=norm[1])
        value_loss = info["value_loss"]
        self.policy.critic_optimizer.zero_grad()
        objective.backward()                                           # mu and std carry no graph: value_loss_coef value_loss alone
        if isinstance(self.policy.critic_optimizer, FusedAdam):        # clip + step as one mms_param_step (optim.py); None: the norm only
            critic_grad_norm = self.policy.critic_optimizer.clip_and_step(self.max_grad_norm if self._use_max_grad_norm else None)
        else:
            if self._use_max_grad_norm:
                critic_grad_norm = nn.utils.clip_grad_norm_(critic.parameters(), self.max_grad_norm)
            else:
                critic_grad_norm = get_grad_norm(critic.parameters())
            self.policy.critic_optimizer.step()

        # actor update: the surrogate's gradient
        tail = (actions, old_logp, adv, factor, active_masks)
        if self.fvp == "fisher":
            mu_leaf, ls_leaf = mu_old.detach().requires_grad_(True), head.log_std.detach().clone().requires_grad_(True)
            loss, _ = self._surrogate(mu_leaf, self._std(ls_leaf), *tail)
            g_mu, g_ls = torch.autograd.grad(loss, (mu_leaf, ls_leaf))
            loss_grad = state.grad(g_mu)
            s_at = self._map.order.index(("s", 0))
            off = sum(self._map.numels[:s_at])
            loss_grad[off:off + g_ls.numel()] = g_ls
            col_scale = (1.0 / (M * std_old ** 2)).contiguous()
            dlog = (1.0 - torch.sigmoid(head.log_std.detach() / head.std_x_coef)) / head.std_x_coef
            s_curv = 2.0 * dlog ** 2
            fvp = lambda p: self._fvp_fisher(state, col_scale, s_curv, p)
        else:
            loss, _ = self._surrogate(self._mean(obs), self._std(), *tail)
            loss_grad = self._flat(torch.autograd.grad(loss, list(actor.parameters()), allow_unused=True)).data
            fvp = lambda p: self._fvp_autograd(obs, p)

        step_dir = self.conjugate_gradient(fvp, loss_grad, nsteps=10)
        loss = loss.data.cpu().numpy()
        params = self.flat_params(actor)
        shs = 0.5 * (step_dir * fvp(step_dir)).sum(0, keepdim=True)
        step_size = 1 / torch.sqrt(shs / self.kl_threshold)[0]
        full_step = step_size * step_dir
        expected_improve = (loss_grad * full_step).sum(0, keepdim=True).data.cpu().numpy()

        # backtracking line search
        flag = False
        fraction = 1
        tries = 0
        for _ in range(self.ls_step):
            tries += 1
            self.update_model(actor, params + fraction * full_step)
            with torch.no_grad():
                mu, std = self._mean(obs), self._std()
                new_loss, ratio = self._surrogate(mu, std, *tail)
                kl = gaussian_kl(mu_old, std_old, mu, std).mean()
                dist_entropy = self._entropy(std, active_masks, M)
            loss_improve = new_loss.data.cpu().numpy() - loss
            if kl < self.kl_threshold and (loss_improve / expected_improve) > self.accept_ratio and loss_improve.item() > 0:
                flag = True
                break
            expected_improve *= 0.5
            fraction *= 0.5
        if not flag:
            self.update_model(actor, params)
            print('policy update does not impove the surrogate')
        self.last = {"step_dir": step_dir, "full_step": full_step, "loss_grad": loss_grad, "tries": tries, "accepted": flag}
        return value_loss, critic_grad_norm, kl, loss_improve, expected_improve, dist_entropy, ratio

    def train(self, buffer, update_actor=True):
        """hatrpo_trainer.py:321-375."""
        if self._use_popart:
            advantages = buffer.returns[:-1] - self.value_normalizer.denormalize(buffer.value_preds[:-1])
        else:
            advantages = buffer.returns[:-1] - buffer.value_preds[:-1]
        advantages_copy = advantages.clone()
        mean_advantages = torch.mean(advantages_copy)
        std_advantages = torch.std(advantages_copy)
        advantages = (advantages - mean_advantages) / (std_advantages + 1e-5)
        train_info = {k: 0 for k in ("value_loss", "kl", "dist_entropy", "loss_improve", "expected_improve", "critic_grad_norm", "ratio")}
        for sample in buffer.feed_forward_generator(advantages, self.num_mini_batch):
            value_loss, critic_grad_norm, kl, loss_improve, expected_improve, dist_entropy, imp_weights = self.trpo_update(sample, update_actor)
            train_info["value_loss"] += value_loss.item()
            train_info["kl"] += kl
            train_info["loss_improve"] += loss_improve.item()
            train_info["expected_improve"] += expected_improve
            train_info["dist_entropy"] += dist_entropy.item()
            train_info["critic_grad_norm"] += critic_grad_norm
            train_info["ratio"] += imp_weights.mean()
        for k in train_info.keys():
            train_info[k] /= self.num_mini_batch
        return train_info

    def prep_training(self):
        self.policy.actor.train()
        self.policy.critic.train()

    def prep_rollout(self):
        self.policy.actor.eval()
        self.policy.critic.eval()

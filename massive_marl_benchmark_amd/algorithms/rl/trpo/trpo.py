"""TRPO, the learner (agents/algorithms/rl/trpo/trpo.py): the reference's constructor, attributes, `learn` config keys and methods
(`run`, `update`, `conjugate_gradient`, `line_search`, `kl_hessian_times_vector`, `set_pi_flat_params`, `get_pi_flat_params`,
`get_aloss_logp`, `log`, `save`, `load`, `test`) over this package's ActorCritic and RolloutStorage, so `process_sarl`'s TRPO branch
trains without the reference tree.  The loop, the log and the checkpoint methods are on_policy.OnPolicyLearner's, shared with PPO.

The default route of `update()` is trpo.py:258-351 statement for statement, including what its code actually does:
  * the step is taken with respect to `actor.parameters()` only: `log_std` is not among them (asserted here) and gets no gradient
    anywhere in the update, so it leaves the update as it entered;
  * `line_search` calls `fnew, olp = evaluate_policy(olp)`: every trial is measured against the PREVIOUS evaluation's
    log-probabilities, not the stored ones;
  * three further `evaluate` calls per minibatch at parameters whose result is known (`a_old_loss`, `f0`, `a_new_loss`), each with the
    critic, whose value is thrown away;
  * the critic step runs with the actor frozen: `clip_grad_norm_` over the critic, Adam over whatever has a gradient;
  * "linear search fail" keeps `x0`.

New `learn` keys, all defaulting to the above:
  * `fused_update` (False).  True: one forward per minibatch; `mms_trpo_heads` (heads.py) gives a_loss, kl, logp, gsur and gkl from its
    mu; the surrogate gradient is J^T gsur; the line search's trials are actor-only forwards without a graph
    (`ActorCritic.mean_nograd`) followed by the head's out + logp call, with the `olp` chain kept exactly (the previous trial's logp
    goes in as a dense old_logp); evaluations the reference repeats at unchanged parameters are not run again -- `a_old_loss` and `f0`
    are the first call's a_loss (the reference's three evaluations at x0 run the same code on the same bits: so do their results),
    `a_new_loss` is one head-only call on the accepted trial's mu (the x0 one after a failure) against the stored old_logp; the
    critic step is `FusedAdam.clip_and_step` (only the critic's tensors have a gradient).  The host reads the line search needs stay;
    the two running losses are read once, at the end of `update()`.
  * `fvp` ("autograd"): "autograd" is the reference's expression (a create_graph gradient and a double backward per product).
    "direct" builds the module with fused_grad=True, raises if the actor does not qualify for the kernels, and evaluates
        H v = J^T ((J v) / (exp(l)^2 M)) + sum_rows gkl . (d2 mu / d theta2) v + damping v
    as mms_mlp_grad_rop along v (with g = gkl and the d, e of ONE mms_mlp_grad(gkl, save) per minibatch), mms_trpo_heads for
    gn = (J v) / (exp(l)^2 M), and mms_mlp_grad(gn): two chains, no autograd graph, in the flat layout of `actor.parameters()`.
    That is the exact product of the reference's KL because log_std is not differentiated.  Independent of `fused_update`.
    Measured at the shipped shape: 5.63 ms per product against 5.24 ms for torch autograd on the plain module
    and 7.76 ms for autograd over the kernels -- it closes most of that gap, not all of it, so it is off by default.

`trace` (attribute, None): a list that receives one dict per minibatch -- the line search's decision, its number of trials and every
trial's margin (f0 - fnew) - alpha expected_improve, every v . Av, the value loss, the critic's norm before clipping, and the new
surrogate loss -- for tests that replay a recorded update."""
import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from ....optim import FusedAdam
from ..on_policy import OnPolicyLearner
from .heads import StoredRows, trpo_heads
from .module import ActorCritic, grad_flat, grad_saved, rop_flat
from .storage import RolloutStorage


class TRPO(OnPolicyLearner):
    logs_fps = True

    def __init__(self, vec_env, cfg_train, device='cpu', sampler='sequential', log_dir='run', is_testing=False, print_log=True, apply_reset=False,
                 asymmetric=False):
        learn = cfg_train["learn"]
        self.fused_update = bool(learn.get("fused_update", False))
        self.fvp = learn.get("fvp", "autograd")
        if self.fvp not in ("autograd", "direct"):
            raise ValueError("learn.fvp must be 'autograd' or 'direct', not %r" % (self.fvp,))
        learn_cfg = self._init_common(vec_env, cfg_train, device, sampler, log_dir, is_testing, print_log, apply_reset, asymmetric, ActorCritic,
                                      RolloutStorage, fused_grad=self.fvp == "direct")
        optimizer = FusedAdam if self.fused_update else optim.Adam
        self.optimizer = optimizer(self.actor_critic.parameters(), lr=self.learning_rate)
        # the policy step is over actor.parameters(): log_std must not be differentiated silently
        assert all(p is not self.actor_critic.log_std for p in self.actor_critic.actor.parameters())
        if self.fvp == "direct":
            probe = torch.zeros(1, self.observation_space.shape[0], device=self.device)
            if not self.actor_critic._grad_path_qualifies(probe):
                raise ValueError("learn.fvp = 'direct' needs an actor the kernels take: fp32 Linear / ELU layers with biases, 2..8 layers, input "
                                 "widths multiples of 4")

        # TRPO parameters
        self.clip_param = learn_cfg["cliprange"]
        self.num_learning_epochs = learn_cfg["noptepochs"]
        self.num_mini_batches = learn_cfg["nminibatches"]
        self.damping = learn_cfg["damping"]
        self.cg_nsteps = learn_cfg["cg_nsteps"]
        self.max_kl = learn_cfg["max_kl"]
        self.max_num_backtrack = learn_cfg["max_num_backtrack"]
        self.accept_ratio = learn_cfg["accept_ratio"]
        self.step_fraction = learn_cfg["step_fraction"]
        self.gamma = learn_cfg["gamma"]
        self.lam = learn_cfg["lam"]
        self.max_grad_norm = learn_cfg.get("max_grad_norm", 2.0)
        self.use_clipped_value_loss = learn_cfg.get("use_clipped_value_loss", False)
        self.trace = None
        self._rec = None                    # the minibatch's trace entry while it is being filled
        self._direct = None                 # (net, gkl, d, e) of the minibatch's direct curvature products
        self._init_log(log_dir, print_log, is_testing, apply_reset)

    # ---- the update ----------------------------------------------------------------------------------------------------------------

    def update(self):
        mean_value_loss = 0
        mean_surrogate_loss = 0
        batch = self.storage.mini_batch_generator(self.num_mini_batches)
        step = self._fused_minibatch if self.fused_update else self._minibatch
        for epoch in range(self.num_learning_epochs):
            for indices in batch:
                self._rec = dict(vAv=[], margins=[]) if self.trace is not None else None
                value_loss, surrogate_loss = step(indices)
                self._direct = None
                if self._rec is not None:
                    self.trace.append(self._rec)
                mean_value_loss = mean_value_loss + value_loss
                mean_surrogate_loss = mean_surrogate_loss + surrogate_loss
        num_updates = self.num_learning_epochs * self.num_mini_batches
        if self.fused_update:                   # the one host read of the two sums
            mean_value_loss, mean_surrogate_loss = torch.stack([torch.as_tensor(v, dtype=torch.float32, device=self.device)
                                                                for v in (mean_value_loss, mean_surrogate_loss)]).tolist()
        return mean_value_loss / num_updates, mean_surrogate_loss / num_updates

    def _policy_step(self, flat_g, Av, evaluate_policy, old_logp):
        """trpo.py:302-315 behind the gradient: the search direction, the largest step along it, the line search, the new parameters."""
        step_dir = self.conjugate_gradient(Av, -flat_g, nsteps=self.cg_nsteps)
        sAs = (step_dir * Av(step_dir)).sum(0)
        beta = torch.sqrt(2 * self.max_kl / sAs)
        full_step = (beta * step_dir).data
        success, new_params = self.line_search(evaluate_policy, full_step, old_logp, flat_g, max_num_backtrack=self.max_num_backtrack,
                                               accept_ratio=self.accept_ratio, step_fraction=self.step_fraction)
        self.set_pi_flat_params(new_params)
        return success

    def _minibatch(self, indices):
        """One minibatch of the default route (trpo.py:268-345); returns the two losses as host numbers."""
        b = self._gather(indices)
        obs_batch, states_batch, actions_batch, advantages_batch, old_actions_log_prob_batch = b['obs'], b['states'], b['actions'], b['adv'], b['old_logp']
        actor = self.actor_critic.actor
        actions_log_prob_batch, entropy_batch, value_batch, mu_batch, sigma_batch = self.actor_critic.evaluate(obs_batch, states_batch, actions_batch)

        # 1. the search direction, by conjugate gradient
        a_loss = -torch.squeeze(advantages_batch) * torch.exp(actions_log_prob_batch - torch.squeeze(old_actions_log_prob_batch))
        a_loss = a_loss.mean()
        g = torch.autograd.grad(a_loss, actor.parameters(), retain_graph=True)
        flat_g = torch.cat([grad.view(-1) for grad in g]).detach()
        kl = torch.mean(self._kl(sigma_batch, mu_batch, b).unsqueeze(-1))
        if self.fvp == "direct":
            self._prepare_direct(obs_batch, indices)
        Av = lambda v: self.kl_hessian_times_vector(v, kl)

        # 2., 3. the largest step along it and the line search
        evaluate_policy = lambda x: self.get_aloss_logp(obs_batch, states_batch, actions_batch, advantages_batch, old_actions_log_prob_batch=x)
        a_old_loss, old_logp = evaluate_policy(old_actions_log_prob_batch)
        self._policy_step(flat_g, Av, evaluate_policy, old_actions_log_prob_batch)
        a_new_loss, new_logp = evaluate_policy(old_actions_log_prob_batch)
        surrogate_loss = a_new_loss

        # the critic's step, with the actor frozen
        for p in actor.parameters():
            p.requires_grad = False
        value_loss = self._value_loss(value_batch, b)
        self.optimizer.zero_grad()
        value_loss.backward()
        norm = nn.utils.clip_grad_norm_(self.actor_critic.critic.parameters(), self.max_grad_norm)
        self.optimizer.step()
        for p in actor.parameters():
            p.requires_grad = True
        if self._rec is not None:
            self._rec.update(value_loss=value_loss.detach(), norm=norm.detach(), surrogate_loss=surrogate_loss.detach())
        return value_loss.item(), surrogate_loss.item()

    def _prepare_direct(self, obs_batch, indices, saved=None, gkl=None):
        """What every direct curvature product of this minibatch shares: the actor's saved forward, gkl = d kl / d mu and the d_l / e_l of
        ONE mms_mlp_grad(gkl, save)."""
        mu, net = saved if saved is not None else self.actor_critic.mean_saved(obs_batch.contiguous())
        if gkl is None:
            gkl = trpo_heads(self.actor_critic.log_std.detach(), mu=mu, stored=StoredRows(self.storage, indices), want=("gkl",))["gkl"]
        d, e = grad_saved(net, gkl)
        self._direct = (net, gkl, d, e)

    def _fused_minibatch(self, indices):
        """One minibatch of the fused route; returns the two losses as 0-d device tensors."""
        ac, s = self.actor_critic, self.storage
        log_std = ac.log_std.detach()
        if not torch.is_tensor(indices):
            indices = torch.as_tensor(indices, dtype=torch.int64, device=self.device)
        rows = StoredRows(s, indices)
        obs = s.observations.view(-1, *s.observations.size()[2:])[indices]
        states = s.states.view(-1, *s.states.size()[2:])[indices] if self.asymmetric else None

        # the one forward: the actor (with what its derivatives need) and the critic (under autograd, for its own step)
        if self.fvp == "direct":
            mu, net = ac.mean_saved(obs)
            mu_graph = None
        else:
            mu_graph = ac.mean(obs)
            mu = mu_graph.detach().contiguous()
        value_batch = ac.critic(states if self.asymmetric else obs)
        first = trpo_heads(log_std, mu=mu, stored=rows, want=("out", "logp", "gsur", "gkl"))
        params = list(ac.actor.parameters())
        if self.fvp == "direct":
            flat_g = grad_flat(net, first["gsur"])
            self._prepare_direct(obs, indices, saved=(mu, net), gkl=first["gkl"])
            kl = None
        else:
            g = torch.autograd.grad(mu_graph, params, grad_outputs=first["gsur"], retain_graph=True)
            flat_g = torch.cat([grad.reshape(-1) for grad in g]).detach()
            sigma = ac.log_std.repeat(mu.shape[0], 1)
            kl = torch.mean(self._kl(sigma, mu_graph, dict(old_mu=rows.old_mu[indices], old_sigma=rows.old_sigma[indices])))
        Av = lambda v: self.kl_hessian_times_vector(v, kl)

        # the line search's evaluations.  Its first one is f0 at x0 against the stored log-probabilities: the first call's numbers.  Every
        # later one follows a set_pi_flat_params: an actor-only forward and the head's out + logp call against `x`, the previous
        # evaluation's logp as a dense vector.
        state = dict(mu=mu, calls=0)

        def evaluate_policy(x):
            state["calls"] += 1
            if state["calls"] == 1:
                return first["out"][0], first["logp"]
            state["mu"] = ac.mean_nograd(obs)
            res = trpo_heads(log_std, mu=state["mu"], stored=rows, old_logp=x, want=("out", "logp"))
            return res["out"][0], res["logp"]

        success = self._policy_step(flat_g, Av, evaluate_policy, rows.old_logp)
        if not success:
            state["mu"] = mu                    # x0 was put back: its mean is the first forward's
        a_new_loss = trpo_heads(log_std, mu=state["mu"], stored=rows, want=("out",))["out"][0]

        # the critic's step: nothing but the critic has a gradient
        value_loss = self._value_loss(value_batch, dict(target_values=s.values.view(-1, 1)[indices], returns=s.returns.view(-1, 1)[indices]))
        self.optimizer.zero_grad()
        value_loss.backward()
        norm = self.optimizer.clip_and_step(self.max_grad_norm)
        if self._rec is not None:
            self._rec.update(value_loss=value_loss.detach(), norm=norm, surrogate_loss=a_new_loss)
        return value_loss.detach(), a_new_loss

    # ---- the reference's methods -------------------------------------------------------------------------------------------------

    def conjugate_gradient(self, Av, b, nsteps, residual_tol=1e-10):
        """An approximate v with A v = b from `nsteps` conjugate gradient steps (trpo.py:353-382).  Av: a callable v -> A v."""
        x = torch.zeros(b.size(), device=self.device)
        r = b.clone()
        p = b.clone()
        rdotr = torch.dot(r, r)
        for k in range(nsteps):
            av = Av(p)
            alpha = rdotr / torch.dot(p, av)
            x += alpha * p
            r -= alpha * av
            new_rdotr = torch.dot(r, r)
            if new_rdotr < residual_tol:
                break
            beta = new_rdotr / rdotr
            p = r + beta * p
            rdotr = new_rdotr
        return x

    def line_search(self, evaluate_policy, full_step, old_actions_log_prob_batch, grad, max_num_backtrack=10, accept_ratio=0.1, step_fraction=1.0):
        """Backtracking line search (trpo.py:384-415): (whether a point was accepted, the accepted parameters or x0).  evaluate_policy(x)
        returns (loss, log-probabilities) at the current parameters against the log-probabilities x; each trial hands the NEXT one its
        own log-probabilities, as the reference does."""
        x0 = self.get_pi_flat_params()
        f0, olp = evaluate_policy(old_actions_log_prob_batch)
        alpha = step_fraction
        expected_improve = accept_ratio * (-full_step * grad).sum(0, keepdim=True)
        success, found = False, x0
        for count in range(max_num_backtrack):
            xnew = x0 + alpha * full_step
            self.set_pi_flat_params(xnew)
            fnew, olp = evaluate_policy(olp)
            actual_improve = f0 - fnew
            if self._rec is not None:
                self._rec["margins"].append(float((actual_improve - alpha * expected_improve).detach()))
            if actual_improve > 0 and actual_improve > alpha * expected_improve:
                success, found = True, xnew
                break
            alpha *= 0.5
        if not success:
            print("linear search fail")
        if self._rec is not None:
            self._rec.update(success=success, trials=len(self._rec["margins"]))
        return success, found

    def kl_hessian_times_vector(self, v, kl):
        """(H + damping I) v, H the Hessian of the KL over the actor's parameters (trpo.py:417-435), in O(n) time."""
        if self.fvp == "direct":
            net, gkl, d, e = self._direct
            jv, curvature = rop_flat(net, gkl, d, e, v.contiguous())
            gn = trpo_heads(self.actor_critic.log_std.detach(), rmu=jv, want=("gn",))["gn"]
            out = curvature + grad_flat(net, gn) + self.damping * v
        else:
            params = list(self.actor_critic.actor.parameters())
            grad_kl = torch.autograd.grad(kl, params, create_graph=True)
            flat_grad_kl = torch.cat([grad.view(-1) for grad in grad_kl])
            grad_kl_v = (flat_grad_kl * v).sum()
            grad_grad_kl_v = torch.autograd.grad(grad_kl_v, params, retain_graph=True)
            out = torch.cat([grad.contiguous().view(-1) for grad in grad_grad_kl_v]).detach() + self.damping * v
        if self._rec is not None:
            self._rec["vAv"].append(float((v * out).sum().detach()))
        return out

    def set_pi_flat_params(self, flat_params):
        """Write the flat vector into the actor's parameters (trpo.py:437-449)."""
        prev_ind = 0
        for param in self.actor_critic.actor.parameters():
            flat_size = int(np.prod(list(param.size())))
            param.data.copy_(flat_params[prev_ind:prev_ind + flat_size].view(param.size()))
            prev_ind += flat_size
        self.old_log_prob = None

    def get_pi_flat_params(self):
        """The actor's parameters as one flat vector (trpo.py:451-462)."""
        return torch.cat([param.data.view(-1) for param in self.actor_critic.actor.parameters()])

    def get_aloss_logp(self, obs_batch, states_batch, actions_batch, advantages_batch, old_actions_log_prob_batch=None):
        """(the surrogate loss against the given log-probabilities, the current log-probabilities) (trpo.py:464-478)."""
        actions_log_prob_batch, entropy_batch, value_batch, mu_batch, sigma_batch = self.actor_critic.evaluate(obs_batch, states_batch, actions_batch)
        a_loss = -torch.squeeze(advantages_batch) * torch.exp(actions_log_prob_batch - torch.squeeze(old_actions_log_prob_batch))
        a_loss = a_loss.mean()
        return a_loss, actions_log_prob_batch

"""MADDPG (agents/algorithms/marl/maddpg/module.py): `Actor`, `Critic`, `MADDPG_policy` and the learner `MADDPG`, with the
reference's constructors, attribute names, config keys and state_dict keys (`pi.pi.{0,2,..}.*`, `q.q.{0,2,..}.*`).

What the reference's functions compute is kept value for value:
  * the target Q is evaluated with the ONLINE critic `policy[nid].critic.q` (module.py:218), although `critic_targ` exists and is
    polyak-updated;
  * `cal_pi_loss` feeds agent `id`'s observation to EVERY agent's actor (:233);
  * `train` draws one index list from `buffer[0]`, breaks when `learn_ep >= num_learning_epochs`, shares ONE dict between the agents
    and divides it once per agent (:296-348);
  * `mlp()` constructs a throw-away `nn.Linear` per layer (:31): it only matters for the RNG stream at initialisation;
  * the polyak updates happen inside the per-agent loop of `ddpg_update` (:280-292): agent `nid`'s target sees the already updated
    target actors of agents `< nid`.
One keyword is not the reference's: `MADDPG(..., use_target_critic=False)`; True evaluates the target with `critic_targ.q` (the
published algorithm) -- the same path with other parameter pointers.

The no-gradient side leaves torch (`fused=True`, the default; `fused=False`: torch always).  The reference's `ddpg_update` runs, per
agent, all N target actors and all N online actors (N^2 + N(N-1) small MLP passes, three launches per layer, of which one actor's
gradient is used).  Here:
  * collection, `MADDPG.act_all`: the hidden layers of all agents through `mms_linear_group_act`, one launch per layer and chunk of
    32 agents, then one `mms_det_heads_act_group` per chunk that writes each agent's action into its destination (a replay ring row)
    and the joint action row; the exploration noise comes from the device's counter-based stream -- a different stream of normals
    than torch.randn's with the same distribution (as rl/ddpg/module.py documents) -- with the counters in a device tensor, so a
    captured graph draws fresh noise;
  * target actions: ONE grouped pass of all target actors on their own `obs2` at the start of `ddpg_update`, written straight into
    the joint-action columns of a critic-input buffer [M, S + N A]; after agent `id`'s target actor is polyak-updated its columns
    alone are refreshed (groups = 1, agent0 = id): N + (N - 1) actor passes instead of N^2, the reference's ordering intact;
  * Q targets: `share_obs2` is copied into the buffer's left columns, the critic's hidden layers go through `mms_linear_group_act`
    and `mms_q_heads_backup_group` computes the last layer and the Bellman backup: one chain per agent (critic `nid` changes in its
    own iteration, so the reference's ordering admits no grouping across agents), no `torch.cat`, no element-wise launches;
  * `cal_pi_loss`: the N - 1 actors whose gradient the reference computes and throws away run under no_grad as one grouped pass on
    agent `id`'s observation; agent `id`'s own action and the critic stay torch autograd.  The other actors' `.grad` fields
    therefore stay UNTOUCHED here (the reference accumulates into them and never reads them: every actor's optimizer zeroes its
    gradients before its own step).
Widths that are no multiple of 4 (TenAnt's per-agent observation: 46): rows are taken at a pitch rounded up to 4 -- in place where
the tensor already has that pitch (the ReplayBuffer's padded rows and gathers from them), through one `F.pad` otherwise -- and the
first layer's weights get zero-padded copies rebuilt from the parameters on EVERY call: there is no validity rule, whatever rewrote
the parameters since the last call is in the result.

The fused paths are decided before the first launch and otherwise give way to the plain modules: on the CPU without the CPU library,
for activations outside ELU / ReLU / Tanh / Identity, for hidden widths the entries do not take (the last one a multiple of 64, the
others of 4), for parameters that are not dense and 16-byte aligned, for agents of different shapes.  Only the exact-fp32 layer
kernel is used."""
import ctypes
import os
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import _lib
from ....optim import FusedAdam
from .storage import round_up4

_ACT_CODES = {nn.Identity: 0, nn.ELU: 1, nn.ReLU: 2, nn.Tanh: 3}
_MAX_GROUPS = 32         # include/mms.h: MMS_MAX_GROUPS
_Q_MAX_H = 4096          # include/mms.h: MMS_Q_MAX_H
_vp = ctypes.c_void_p


def get_activation(act_name):
    acts = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "crelu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}
    if act_name not in acts:
        print("invalid activation function!")
        return None
    return acts[act_name]()


def mlp(sizes, activation, output_activation=nn.Identity()):
    layers = []
    for j in range(len(sizes) - 1):
        act = activation if j < len(sizes) - 2 else output_activation
        nn.Linear(sizes[j], sizes[j + 1])           # (module.py:31: a layer that is thrown away; kept for the initialisation's RNG stream)
        layers += [nn.Linear(sizes[j], sizes[j + 1]), act]
    return nn.Sequential(*layers)


class MLPActLayer(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit):
        super().__init__()
        self.pi = mlp([obs_dim] + list(hidden_sizes) + [act_dim], activation, nn.Tanh())
        self.act_limit = act_limit

    def forward(self, obs):
        return self.act_limit * self.pi(obs)


class MLPQFunction(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes, activation):
        super().__init__()
        self.q = mlp([obs_dim + act_dim] + list(hidden_sizes) + [1], activation)

    def forward(self, obs, act):
        return self.q(torch.cat([obs, act], dim=-1))


class Actor(nn.Module):
    def __init__(self, observation_space, action_space, hidden_sizes=(256, 256), activation=nn.ReLU, device=torch.device("cuda:0")):
        super().__init__()
        self.pi = MLPActLayer(observation_space.shape[0], action_space.shape[0], hidden_sizes, activation, action_space.high[0])
        self.to(device)

    def act(self, obs):
        return self.pi(obs)


class Critic(nn.Module):
    def __init__(self, share_observation_space, share_action_space, hidden_sizes=(256, 256), activation=nn.ReLU, device=torch.device("cuda:0")):
        super().__init__()
        share_act_dim = sum(space.shape[0] for space in share_action_space)
        self.q = MLPQFunction(share_observation_space.shape[0], share_act_dim, hidden_sizes, activation)
        self.to(device)

    def get_value(self, share_obs, share_acts):
        return self.q(share_obs, share_acts)


class MADDPG_policy:
    def __init__(self, config, obs_space, cent_obs_space, act_space, cent_act_space, device=torch.device("cpu")):
        self.device = device
        self.lr = config["learning_rate"]
        self.hidden_size = config["hidden_size"]
        self.activation = get_activation(config["activation"])
        self.act_noise = config["act_noise"]
        self.obs_space = obs_space
        self.share_obs_space = cent_obs_space
        self.act_space = act_space
        self.share_act_space = cent_act_space
        self.act_limit = act_space.high[0]
        self.actor = Actor(self.obs_space, self.act_space, self.hidden_size, self.activation, self.device)
        self.critic = Critic(self.share_obs_space, self.share_act_space, self.hidden_size, self.activation, self.device)
        self.actor_targ = deepcopy(self.actor)
        self.critic_targ = deepcopy(self.critic)
        # config "fused_step" (not the reference's; default False): FusedAdam (optim.py), whose clip_and_step MADDPG.ddpg_update then calls
        Adam = FusedAdam if config.get("fused_step", False) else torch.optim.Adam
        self.actor_optimizer = Adam(self.actor.pi.parameters(), lr=self.lr)
        self.critic_optimizer = Adam(self.critic.q.parameters(), lr=self.lr)

    def get_actions(self, obs, deterministic=False):
        return self.actor.act(obs).detach()

    def get_values(self, cent_obs, cent_acts):
        """(The reference calls the Critic module, which has no forward, and unpacks a 1-tuple from a tensor: repaired.)"""
        return self.critic.get_value(cent_obs, cent_acts)

    def act(self, obs, deterministic=False):
        actions = self.actor.act(obs)
        if not deterministic:
            actions = torch.clamp(actions + self.act_noise * torch.randn(actions.shape).to(self.device), -self.act_limit, self.act_limit)
        return actions.detach()


# ---- the launches ----------------------------------------------------------------------------------------------------------------

def _table(ts):
    return (_vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _library(dev):
    """(library, device argument, stream) for `dev`, or None where there is no library to run on (the CPU without the CPU build)."""
    dev = torch.device(dev)
    if dev.type == "cuda" or (dev.type == "cpu" and os.path.exists(_lib.LIB_CPU_PATH)):
        return _lib.for_device(dev)
    return None


def _qualify(seqs, kind, dev):
    """The networks `seqs` (nn.Sequential of Linear / activation pairs, all of one shape) as lists of modules if the entries take
    them, else None.  kind "actor": Linear(H, A <= 128) + Tanh at the end; "critic": Linear(H, 1) + Identity."""
    nets = [list(s) for s in seqs]
    n0 = nets[0]
    if len(n0) < 4 or len(n0) % 2:
        return None
    for m in nets:
        if len(m) != len(n0):
            return None
        for i in range(0, len(m), 2):
            lin, fn, lin0, fn0 = m[i], m[i + 1], n0[i], n0[i + 1]
            if not isinstance(lin, nn.Linear) or not isinstance(lin0, nn.Linear) or lin.bias is None or type(fn) is not type(fn0):
                return None
            if (lin.in_features, lin.out_features) != (lin0.in_features, lin0.out_features):
                return None
            for t in (lin.weight, lin.bias):
                if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.data_ptr() % 4:
                    return None
            if lin.weight.data_ptr() % 16:
                return None
            if i == len(m) - 2:
                if lin.in_features % 64:
                    return None
                if kind == "actor" and (type(fn) is not nn.Tanh or not 1 <= lin.out_features <= 128):
                    return None
                if kind == "critic" and (type(fn) is not nn.Identity or lin.out_features != 1 or lin.in_features > _Q_MAX_H):
                    return None
            else:
                if type(fn) not in _ACT_CODES or (isinstance(fn, nn.ELU) and fn.alpha != 1.0) or (i > 0 and lin.in_features % 4):
                    return None
    return nets


def _rows4(x):
    """x [..., K] as dense fp32 rows [M, round_up4(K)].  In place where x already lies at that pitch (a view [..., :K] of padded rows:
    the ReplayBuffer's, and gathers from them; the zero-padded weights multiply the padding, which therefore only has to be finite
    and is zero there), else one F.pad."""
    K = x.shape[-1]
    Kp = round_up4(K)
    M = x.shape[:-1].numel()
    if Kp == K:
        x = x.reshape(M, K).contiguous()
        return x if x.data_ptr() % 16 == 0 else x.clone()
    want, pitch = True, Kp
    for size, stride in zip(reversed(x.shape[:-1]), reversed(x.stride()[:-1])):
        want = want and (size == 1 or stride == pitch)
        pitch *= size
    room = x.untyped_storage().nbytes() // 4 - x.storage_offset()
    if want and x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and room >= M * Kp and M > 0:
        return x.as_strided((M, Kp), (Kp, 1))
    return F.pad(x.reshape(M, K), (0, Kp - K))


def _hidden(lib3, nets, xs, M):
    """The hidden Linear + activation pairs of `nets` (equal shapes) on xs[g] [M, Kp]: one mms_linear_group_act per layer and chunk
    of 32 networks.  Returns the last hidden activations per network."""
    L, idx, stream = lib3
    G = len(nets)
    cur = list(xs)
    for l in range(len(nets[0]) // 2 - 1):
        lins = [m[2 * l] for m in nets]
        N, K, Kx = lins[0].out_features, lins[0].in_features, cur[0].shape[1]
        ws = [lin.weight.detach() for lin in lins]
        if Kx != K:                                   # padded rows: zero-padded weights, rebuilt from the parameters on every call
            ws = list(F.pad(torch.stack(ws), (0, Kx - K)).unbind(0))
        bs = [lin.bias.detach() for lin in lins]
        y = list(torch.empty(G, M, N, device=cur[0].device).unbind(0))
        act = _ACT_CODES[type(nets[0][2 * l + 1])]
        for c in range(0, G, _MAX_GROUPS):
            s = slice(c, min(G, c + _MAX_GROUPS))
            _lib.check(L.mms_linear_group_act(idx, len(ws[s]), M, N, Kx, _table(cur[s]), _table(ws[s]), _table(bs[s]), _table(y[s]), act, None, None, None,
                                              stream), None, "mms_linear_group_act", L)
        cur = y
    return cur


def _heads(lib3, nets, hs, M, limits, agent_ids, joint, joint_col0, act_out=None, sigma=0.0, seed=0, counters=None):
    """The actors' last layers through mms_det_heads_act_group: network g is agent agent_ids[g]; runs of consecutive agents (at most 32)
    share a launch (launch i draws with counters[i], a row of an int64 [launches, M] tensor: the entry advances the counters it is
    given once per call).  joint (or None): a tensor whose rows take agent a's action at columns joint_col0 + a A; act_out (or None): one
    [M, A] destination per network, all at the same row pitch."""
    L, idx, stream = lib3
    last = [m[-2] for m in nets]
    A, H = last[0].out_features, last[0].in_features
    g = launch = 0
    while g < len(nets):
        e = g + 1
        while e < len(nets) and e - g < _MAX_GROUPS and agent_ids[e] == agent_ids[e - 1] + 1:
            e += 1
        n = e - g
        _lib.check(L.mms_det_heads_act_group(idx, n, M, H, A, agent_ids[g], _table(hs[g:e]), _table([l.weight.detach() for l in last[g:e]]),
                                             _table([l.bias.detach() for l in last[g:e]]), (ctypes.c_float * n)(*[float(v) for v in limits[g:e]]), float(sigma),
                                             seed, None if counters is None else _vp(counters[launch].data_ptr()), 0, None if act_out is None else _table(act_out[g:e]),
                                             0 if act_out is None else act_out[g].stride(0), None if joint is None else _vp(joint.data_ptr() + 4 * joint_col0),
                                             0 if joint is None else joint.stride(0), stream), None, "mms_det_heads_act_group", L)
        g = e
        launch += 1


class MADDPG():
    def __init__(self, config, policy, num_agents, device=torch.device("cpu"), use_target_critic=False, fused=True):
        self.device = device
        self.num_agents = num_agents
        self.policy = policy
        self.num_learning_epochs = config["num_learning_epochs"]
        self.num_mini_batches = config["num_mini_batch"]
        self.gamma = config["gamma"]
        self.learning_rate = config["learning_rate"]
        self.polyak = config["polyak"]
        self.max_grad_norm = config["max_grad_norm"]
        self.use_target_critic = bool(use_target_critic)     # True: the target Q from critic_targ (the published algorithm)
        self.fused = bool(fused)                             # False: torch always
        self.noise_seed = int(torch.initial_seed()) & 0x7fffffffffffffff
        self._counters = {}                                  # the exploration noise's draw counters per (device, rows): [chunks of 32 agents, rows]

    # ---- what decides the fused paths, before the first launch ----

    def _fused_nets(self, which, kind, dev, agents=None):
        """(library triple, module lists) for the `which` networks ("actor", "actor_targ", "critic", "critic_targ") of `agents`, or None."""
        if not self.fused or torch.device(dev).type not in ("cuda", "cpu"):
            return None
        lib3 = _library(dev)
        if lib3 is None:
            return None
        agents = range(self.num_agents) if agents is None else agents
        seqs = [getattr(self.policy[a], which).pi.pi if kind == "actor" else getattr(self.policy[a], which).q.q for a in agents]
        nets = _qualify(seqs, kind, torch.device(dev)) if seqs else None
        return None if nets is None else (lib3, nets)

    def _target_critic(self, nid):
        return (self.policy[nid].critic_targ if self.use_target_critic else self.policy[nid].critic).q

    @staticmethod
    def _fits(*ts):
        return all(torch.is_tensor(t) and t.dtype == torch.float32 and t.device == ts[0].device and t.dim() >= 2 for t in ts)

    # ---- collection ----

    @torch.no_grad()
    def act_all(self, obs_list, deterministic=False, act_slots=None, joint_slot=None):
        """Every agent's action on its own observation obs_list[a] [M, K]: returns (the list of [M, A] actions, the joint action
        [M, N A] = their concatenation).  act_slots (one [M, A] tensor per agent, e.g. `buffer[a].actions[buffer[a].slot()]`) and
        joint_slot ([M, N A], e.g. the shared `joint_actions[slot]`) are written in place and returned; None: fresh tensors."""
        N = self.num_agents
        dev = obs_list[0].device
        M = obs_list[0].shape[0]
        plan = self._fused_nets("actor", "actor", dev) if self._fits(*obs_list) and all(o.dim() == 2 and o.shape == obs_list[0].shape for o in obs_list) else None
        A = self.policy[0].act_space.shape[0]
        if plan is not None and act_slots is not None:
            ok = all(t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (M, A) and t.stride(1) == 1 and t.stride(0) == act_slots[0].stride(0)
                     for t in act_slots)
            plan = plan if ok else None
        if plan is not None and joint_slot is not None:
            ok = joint_slot.dtype == torch.float32 and joint_slot.device == dev and tuple(joint_slot.shape) == (M, N * A) and joint_slot.stride(1) == 1
            plan = plan if ok else None
        if plan is None or M == 0:
            acts = [self.policy[a].act(obs_list[a], deterministic) for a in range(N)]
            joint = torch.cat(acts, dim=-1)
            if act_slots is not None:
                for dst, src in zip(act_slots, acts):
                    dst.copy_(src)
                acts = list(act_slots)
            if joint_slot is not None:
                joint_slot.copy_(joint)
                joint = joint_slot
            return acts, joint
        lib3, nets = plan
        acts = list(act_slots) if act_slots is not None else list(torch.empty(N, M, A, device=dev).unbind(0))
        joint = joint_slot if joint_slot is not None else torch.empty(M, N * A, device=dev)
        sigma = 0.0 if deterministic else float(self.policy[0].act_noise)
        counters = None
        if sigma > 0.0:
            counters = self._counters.get((str(dev), M))
            if counters is None:
                counters = self._counters[(str(dev), M)] = torch.zeros((N + _MAX_GROUPS - 1) // _MAX_GROUPS, M, dtype=torch.int64, device=dev)
        hs = _hidden(lib3, nets, [_rows4(o) for o in obs_list], M)
        _heads(lib3, nets, hs, M, [self.policy[a].act_limit for a in range(N)], list(range(N)), joint, 0, acts, sigma, self.noise_seed, counters)
        return acts, joint

    # ---- the Q target ----

    @torch.no_grad()
    def _target_inputs(self, data):
        """The critic-input buffer [M, round_up4(S + N A)] with every target actor's action on its own obs2 in the joint-action
        columns (ONE grouped pass), and what refreshes one agent's columns; None where the fused path does not apply."""
        N = self.num_agents
        if not self._fits(*[data[v]["obs2"] for v in range(N)], *[data[v]["sobs2"] for v in range(N)]):
            return None
        dev = data[0]["obs2"].device
        plan = self._fused_nets("actor_targ", "actor", dev)
        if plan is None:
            return None
        lib3, nets = plan
        A, S = nets[0][-2].out_features, data[0]["sobs2"].shape[-1]
        M = data[0]["obs2"].shape[:-1].numel()
        if M == 0 or any(data[v]["obs2"].shape != data[0]["obs2"].shape or data[v]["sobs2"].shape[:-1] != data[0]["obs2"].shape[:-1] for v in range(N)):
            return None
        C = S + N * A
        xin = torch.empty(M, round_up4(C), device=dev)
        if xin.shape[1] > C:
            xin[:, C:].zero_()
        x2 = [_rows4(data[v]["obs2"]) for v in range(N)]
        limits = [self.policy[v].act_limit for v in range(N)]
        _heads(lib3, nets, _hidden(lib3, nets, x2, M), M, limits, list(range(N)), xin, S)
        return {"xin": xin, "x2": x2, "S": S, "C": C, "M": M}

    @torch.no_grad()
    def _refresh_target_action(self, tin, id):
        """Agent id's target actor has changed: its columns of the critic-input buffer alone (groups = 1, agent0 = id)."""
        plan = self._fused_nets("actor_targ", "actor", tin["xin"].device, [id])
        if plan is None:                      # (cannot happen after _target_inputs qualified all of them; the plain module serves)
            a = self.policy[id].actor_targ.pi(tin["x2"][id][:, :self.policy[id].obs_space.shape[0]])
            A = a.shape[-1]
            tin["xin"][:, tin["S"] + id * A:tin["S"] + (id + 1) * A] = a
            return
        lib3, nets = plan
        _heads(lib3, nets, _hidden(lib3, nets, [tin["x2"][id]], tin["M"]), tin["M"], [self.policy[id].act_limit], [id], tin["xin"], tin["S"])

    @torch.no_grad()
    def _backup(self, data, nid, tin):
        """r + gamma (1 - d) Q_nid(sobs2, jact2) (module.py:208-219): the fused chain on the critic-input buffer, or the reference's
        expression in torch."""
        r, d, sobs2 = data[nid]["r"], data[nid]["done"], data[nid]["sobs2"]
        qnet = self._target_critic(nid)
        plan = None
        if tin is not None and r.dtype == torch.float32 and r.numel() == tin["M"] and d.numel() == tin["M"] and r.device == tin["xin"].device == d.device:
            plan = _qualify([qnet.q], "critic", tin["xin"].device)
            if plan is not None and (plan[0][0].in_features != tin["C"] or sobs2.shape[-1] != tin["S"]):
                plan = None
        if plan is None:
            if tin is not None:
                jact2 = tin["xin"][:, tin["S"]:tin["C"]].reshape(*sobs2.shape[:-1], tin["C"] - tin["S"])
            else:
                jact2 = torch.cat([self.policy[v].actor_targ.pi(data[v]["obs2"]) for v in range(self.num_agents)], dim=-1)
            return r + self.gamma * (1 - d) * qnet(sobs2, jact2)
        lib3 = _library(tin["xin"].device)
        L, idx, stream = lib3
        xin, S, M = tin["xin"], tin["S"], tin["M"]
        xin[:, :S].copy_(sobs2.reshape(M, S))
        h = _hidden(lib3, plan, [xin], M)[0]
        d8 = d if d.dtype in (torch.uint8, torch.bool) else d.ne(0)
        d8 = d8.contiguous()
        d8 = d8.view(torch.uint8) if d8.dtype == torch.bool else d8
        rc = r.contiguous()
        backup = torch.empty(r.shape, device=r.device)
        last = plan[0][-2]
        _lib.check(L.mms_q_heads_backup_group(idx, 1, M, h.shape[1], _table([h]), _table([last.weight.detach()]), _table([last.bias.detach()]), None, _table([rc]),
                                              _table([d8]), float(self.gamma), _table([backup]), stream), None, "mms_q_heads_backup_group", L)
        return backup

    def cal_value_loss(self, data, nid, _tin=None):
        q = self.policy[nid].critic.q(data[nid]['sobs'], data[nid]['jact'])
        backup = self._backup(data, nid, self._target_inputs(data) if _tin is None else _tin)
        return ((q - backup) ** 2).mean()

    def cal_pi_loss(self, data, id):
        """-Q_id(sobs, [pi_0(obs_id), .., pi_{N-1}(obs_id)]).mean() (module.py:226-241).  Fused: the N - 1 other actors under no_grad as
        one grouped pass -- their `.grad` fields stay untouched -- and agent id's own action and the critic through autograd."""
        sobs, obs = data[id]['sobs'], data[id]['obs']
        N = self.num_agents
        others = [a for a in range(N) if a != id]
        plan = self._fused_nets("actor", "actor", obs.device, others) if others and self._fits(obs) and not obs.requires_grad else None
        M = obs.shape[:-1].numel()
        if plan is None or M == 0:
            jact = torch.cat([self.policy[pid].actor.pi(obs) for pid in range(N)], dim=-1)
        else:
            lib3, nets = plan
            A = nets[0][-2].out_features
            with torch.no_grad():
                joint = torch.empty(M, N * A, device=obs.device)
                x = _rows4(obs)
                _heads(lib3, nets, _hidden(lib3, nets, [x] * len(nets), M), M, [self.policy[a].act_limit for a in others], others, joint, 0)
            joint = joint.view(*obs.shape[:-1], N * A)
            own = self.policy[id].actor.pi(obs)
            jact = torch.cat([joint[..., :id * A], own, joint[..., (id + 1) * A:]], dim=-1)
        q_pi = self.policy[id].critic.q(sobs, jact)
        return -q_pi.mean()

    def ddpg_update(self, samples):
        """With FusedAdam optimizers on every policy (config "fused_step"): per agent ONE clip_and_step for the critic and one for the
        actor -- clip + Adam + that network's polyak average, one mms_param_step each -- in place of two clips, two steps and the polyak
        loop.  The critic's target is then averaged right behind the critic's step instead of behind the actor's (nothing in between
        reads it); agent id's target actor is refreshed behind its polyak as before."""
        fused_step = all(isinstance(po.critic_optimizer, FusedAdam) and isinstance(po.actor_optimizer, FusedAdam) for po in self.policy)
        value_loss = []
        policy_loss = []
        tin = self._target_inputs(samples)              # every target actor once; None: the reference's per-agent evaluation
        for id in range(self.num_agents):
            self.policy[id].critic_optimizer.zero_grad()
            loss_q = self.cal_value_loss(samples, id, tin) if tin is not None else self.cal_value_loss(samples, id)
            loss_q.backward()
            if fused_step:
                self.policy[id].critic_optimizer.clip_and_step(self.max_grad_norm, targets=self.policy[id].critic_targ.q.parameters(), polyak=self.polyak)
            else:
                nn.utils.clip_grad_norm_(self.policy[id].critic.parameters(), self.max_grad_norm)
                self.policy[id].critic_optimizer.step()
            value_loss.append(loss_q)

            for p in self.policy[id].critic.q.parameters():
                p.requires_grad = False
            self.policy[id].actor_optimizer.zero_grad()
            loss_pi = self.cal_pi_loss(samples, id)
            loss_pi.backward()
            if fused_step:
                self.policy[id].actor_optimizer.clip_and_step(self.max_grad_norm, targets=self.policy[id].actor_targ.pi.parameters(), polyak=self.polyak)
            else:
                nn.utils.clip_grad_norm_(self.policy[id].actor.parameters(), self.max_grad_norm)
                self.policy[id].actor_optimizer.step()
            policy_loss.append(loss_pi)
            for p in self.policy[id].critic.q.parameters():
                p.requires_grad = True

            if not fused_step:
                with torch.no_grad():
                    for p, p_targ in zip(self.policy[id].critic.q.parameters(), self.policy[id].critic_targ.q.parameters()):
                        p_targ.data.mul_(self.polyak)
                        p_targ.data.add_((1 - self.polyak) * p.data)
                    for p, p_targ in zip(self.policy[id].actor.pi.parameters(), self.policy[id].actor_targ.pi.parameters()):
                        p_targ.data.mul_(self.polyak)
                        p_targ.data.add_((1 - self.polyak) * p.data)
            if tin is not None and id + 1 < self.num_agents:
                self._refresh_target_action(tin, id)     # the agents behind see this target actor as updated (the reference's ordering)
        return value_loss, policy_loss

    def train(self, buffer):
        train_infos = []
        train_info = {}
        train_info['value_loss'] = 0
        train_info['policy_loss'] = 0
        batch = buffer[0].mini_batch_generator(self.num_mini_batches)
        learn_ep = 0
        for indices in batch:
            learn_ep += 1
            if learn_ep >= self.num_learning_epochs:
                break
            samples = []
            for id in range(self.num_agents):
                b = buffer[id]
                K = b.obs.shape[-1]
                # gathered at the padded pitch where the buffer has one: the [..., :K] views are what the reference's gathers hold
                obs = b.obs_padded[indices][..., :K] if hasattr(b, "obs_padded") else b.obs[indices]
                obs2 = b.next_observations_padded[indices][..., :K] if hasattr(b, "next_observations_padded") else b.next_observations[indices]
                samples.append({'obs': obs, 'sobs': b.share_obs[indices], 'act': b.actions[indices], 'jact': b.joint_actions[indices], 'r': b.rewards[indices],
                                'obs2': obs2, 'sobs2': b.next_share_obs[indices], 'done': b.dones[indices]})
            value_loss, policy_loss = self.ddpg_update(samples)
            for id in range(self.num_agents):
                train_info['value_loss'] += value_loss[id].item()
                train_info['policy_loss'] += policy_loss[id].item()
                train_infos.append(train_info)
        num_updates = self.num_learning_epochs * self.num_mini_batches
        for id in range(self.num_agents):
            for k in train_infos[id].keys():
                train_infos[id][k] /= num_updates
        return train_infos

    def prep_training(self):
        for id in range(self.num_agents):
            self.policy[id].actor.train()
            self.policy[id].critic.train()

    def prep_rollout(self):
        for id in range(self.num_agents):
            self.policy[id].actor.eval()
            self.policy[id].critic.eval()

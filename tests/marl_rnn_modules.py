"""Test infrastructure: the stand-ins of marl_modules.py with the reference's recurrent layer (agents/algorithms/utils/rnn.py:7-80:
RNNLayer = nn.GRU(hidden, hidden, num_layers=recurrent_N) + nn.LayerNorm, between the base and the head at
agents/algorithms/marl/actor_critic.py:35-36, 64-65, 139-140, 164-165), with its attribute names and state_dict keys, so that the
reference's recurrent state_dicts (tests/golden/marl_rnn_policy.npz) load unchanged, and `torch_forward`, the torch statement of the
single-step forward that the grouped path is compared with.  Not a product path."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import marl_modules as mm


class RNNLayer(nn.Module):
    def __init__(self, hidden, recurrent_N):
        super().__init__()
        self._recurrent_N = recurrent_N
        self.rnn = nn.GRU(hidden, hidden, num_layers=recurrent_N)
        self.norm = nn.LayerNorm(hidden)

    def forward(self, x, hxs, masks):
        """x [rows, hidden], hxs [N, recurrent_N, hidden], masks [rows, 1].  rows == N: one step from hxs * masks.  rows == T * N
        (time-major): the sequence, cut wherever some env's mask is zero -- the state is multiplied by that step's masks at the start of
        every piece (at t = 0 always), inside a piece the GRU runs on."""
        if x.size(0) == hxs.size(0):
            y, h = self.rnn(x.unsqueeze(0), (hxs * masks.view(-1, 1, 1)).transpose(0, 1).contiguous())
            y = y.squeeze(0)
        else:
            N = hxs.size(0)
            T = x.size(0) // N
            xs, m = x.view(T, N, -1), masks.view(T, N)
            cuts = [0] + [t for t in range(1, T) if bool((m[t] == 0).any())] + [T]
            h, ys = hxs.transpose(0, 1), []
            for a, b in zip(cuts[:-1], cuts[1:]):
                y, h = self.rnn(xs[a:b], (h * m[a].view(1, N, 1)).contiguous())
                ys.append(y)
            y = torch.cat(ys).reshape(T * N, -1)
        return self.norm(y), h.transpose(0, 1)


class Actor(mm.Actor):
    def __init__(self, obs_dim, act_dim, hidden=64, layer_N=2, recurrent_N=1):
        super().__init__(obs_dim, act_dim, hidden, layer_N)
        self._use_recurrent_policy, self._recurrent_N = True, recurrent_N
        self.rnn = RNNLayer(hidden, recurrent_N)


class Critic(mm.Critic):
    def __init__(self, share_obs_dim, hidden=64, layer_N=2, recurrent_N=1):
        super().__init__(share_obs_dim, hidden, layer_N)
        self._use_recurrent_policy, self._recurrent_N = True, recurrent_N
        self.rnn = RNNLayer(hidden, recurrent_N)


def torch_forward(actor, critic, obs, share_obs, rnn_states, rnn_states_critic, masks):
    """(mean, std, value, new rnn_states, new rnn_states_critic) of one agent: Actor.forward's distribution parameters and
    Critic.forward's value with the RNNLayer between base and head (single step, or a sequence when the rows say so)."""
    with torch.no_grad():
        hd = actor.act.action_out
        fa, new_a = actor.rnn(mm.base_forward(actor.base, obs), rnn_states, masks)
        fc, new_c = critic.rnn(mm.base_forward(critic.base, share_obs), rnn_states_critic, masks)
        mean = F.linear(fa, hd.fc_mean.weight, hd.fc_mean.bias)
        std = torch.sigmoid(hd.log_std / hd.std_x_coef) * hd.std_y_coef
        value = F.linear(fc, critic.v_out.weight, critic.v_out.bias)
    return mean, std, value, new_a, new_c


def fixture_agents(device="cpu"):
    """[(actor, critic, arrays)] of tests/golden/marl_rnn_policy.npz: the stand-ins with the reference's state_dicts loaded (strict)."""
    import os

    import numpy as np
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marl_rnn_policy.npz"))
    H, layer_N, R = int(fx["hidden"]), int(fx["layer_N"]), int(fx["recurrent_N"])
    out = []
    for i in range(int(fx["agents"])):
        actor, critic = Actor(46, 8, H, layer_N, R), Critic(388, H, layer_N, R)
        for mod, tag in ((actor, "actor"), (critic, "critic")):
            pre = "a%d.%s." % (i, tag)
            mod.load_state_dict({k[len(pre):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(pre)}, strict=True)
        data = {k[len("a%d." % i):]: torch.from_numpy(fx[k]).to(device) for k in fx.files
                if k.startswith("a%d." % i) and not k.startswith("a%d.actor." % i) and not k.startswith("a%d.critic." % i)}
        out.append((actor.to(device), critic.to(device), data))
    return out

"""The networks of the on-policy multi-agent algorithms (MAPPO / HAPPO / HATRPO) as torch modules, with the reference's constructors,
attribute names, config keys and state_dict keys (agents/algorithms/marl/actor_critic.py; utils/mlp.py, rnn.py, act.py,
distributions.py), so that its checkpoints load with strict=True and its Runner-side code finds what it looks for:

    Actor    .base (MLPBase) [.rnn (RNNLayer)] .act (ACTLayer -> .action_out = DiagGaussian: .fc_mean, .log_std, .std_x_coef, .std_y_coef)
    Critic   .base (MLPBase) [.rnn (RNNLayer)] .v_out (Linear(hidden, 1))
    MLPBase  [.feature_norm (LayerNorm)] .mlp.fc1, .mlp.fc2[i] = Sequential(Linear, ELU, LayerNorm)      (use_ReLU picks ELU either way)
    RNNLayer .rnn (nn.GRU, recurrent_N layers) .norm (LayerNorm)

These are the modules the grouped HIP paths read in place (policy_inference.GroupedPolicyInference for the rollout and the factor
passes, trainer.MAPPO / HAPPO and hatrpo.HATRPO for the update); their own forward methods are the torch statement of the same
functions, which `config["fused_factor"] = False` and recurrent policies run in Runner.train.  Written from the behaviour that
tests/golden/marl_policy_fixture.npz and marl_rnn_policy.npz pin (tests/marl_runner_check.py).

Covered: Box action spaces (a diagonal Gaussian whose std is sigmoid(log_std / std_x_coef) * std_y_coef, one value per action
dimension, independent of the state) and flat observations (MLPBase).  Discrete / MultiDiscrete / MultiBinary / mixed action spaces and
image observations (the reference's CNNBase) raise NotImplementedError in the constructor.

FixedNormal.log_probs keeps the PER-DIMENSION log-densities ([M, act_dim]; the reference has the sum commented out,
distributions.py:31-34); everything downstream (the buffers' action_log_probs, the losses' sum over the last dimension, the factor) is
built on that."""
import numpy as np
import torch
import torch.nn as nn


def _tensor(x):
    return torch.from_numpy(x) if isinstance(x, np.ndarray) else x


def _shape_of(space):
    """The shape of an observation space: a Box's, or a plain list's own value"""
    kind = space.__class__.__name__
    if kind == "Box":
        return tuple(space.shape)
    if kind == "list":
        return tuple(space)
    raise NotImplementedError("observation space %s is not covered (Box, or a list holding the shape)" % kind)


def _init_linear(layer, orthogonal, gain):
    (nn.init.orthogonal_ if orthogonal else nn.init.xavier_uniform_)(layer.weight.data, gain=gain)
    nn.init.constant_(layer.bias.data, 0)
    return layer


class MLPLayer(nn.Module):
    def __init__(self, input_dim, hidden_size, layer_N, use_orthogonal, use_ReLU):
        super().__init__()
        self._layer_N = layer_N
        gain = nn.init.calculate_gain("relu" if use_ReLU else "tanh")        # (the activation is ELU for both values of use_ReLU)
        block = lambda k: nn.Sequential(_init_linear(nn.Linear(k, hidden_size), use_orthogonal, gain), nn.ELU(), nn.LayerNorm(hidden_size))
        self.fc1 = block(input_dim)
        self.fc2 = nn.ModuleList([block(hidden_size) for _ in range(layer_N)])

    def forward(self, x):
        x = self.fc1(x)
        for i in range(self._layer_N):
            x = self.fc2[i](x)
        return x


class MLPBase(nn.Module):
    def __init__(self, config, obs_shape, cat_self=True, attn_internal=False):
        super().__init__()
        self._use_feature_normalization = config["use_feature_normalization"]
        self._use_orthogonal = config["use_orthogonal"]
        self._use_ReLU = config["use_ReLU"]
        self._stacked_frames = config["stacked_frames"]
        self._layer_N = config["layer_N"]
        self.hidden_size = config["hidden_size"]
        obs_dim = obs_shape[0]
        if self._use_feature_normalization:
            self.feature_norm = nn.LayerNorm(obs_dim)
        self.mlp = MLPLayer(obs_dim, self.hidden_size, self._layer_N, self._use_orthogonal, self._use_ReLU)

    def forward(self, x):
        if self._use_feature_normalization:
            x = self.feature_norm(x)
        return self.mlp(x)


class RNNLayer(nn.Module):
    """nn.GRU over `recurrent_N` layers + LayerNorm.  forward(x, hxs, masks): x [rows, hidden], hxs [N, recurrent_N, hidden], masks
    [rows, 1].  rows == N is one step from hxs * masks.  rows == T * N (time-major) is a sequence: it is cut at every step at which
    some env's mask is zero; at the start of each piece (always at t = 0) the state is multiplied by that step's masks, inside a piece
    the GRU runs on.  Returns (LayerNorm(outputs) [rows, hidden], the last state [N, recurrent_N, hidden])."""

    def __init__(self, inputs_dim, outputs_dim, recurrent_N, use_orthogonal):
        super().__init__()
        self._recurrent_N = recurrent_N
        self._use_orthogonal = use_orthogonal
        self.rnn = nn.GRU(inputs_dim, outputs_dim, num_layers=recurrent_N)
        for name, param in self.rnn.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                (nn.init.orthogonal_ if use_orthogonal else nn.init.xavier_uniform_)(param)
        self.norm = nn.LayerNorm(outputs_dim)

    def forward(self, x, hxs, masks):
        N = hxs.size(0)
        if x.size(0) == N:
            y, h = self.rnn(x.unsqueeze(0), (hxs * masks.view(N, 1, 1)).transpose(0, 1).contiguous())
            y = y.squeeze(0)
        else:
            T = x.size(0) // N
            xs, m = x.view(T, N, x.size(1)), masks.view(T, N)
            zero_steps = (m[1:] == 0.0).any(dim=-1).nonzero().flatten().cpu().tolist()       # (a host read, as in the reference)
            cuts = [0] + [t + 1 for t in zero_steps] + [T]
            h, pieces = hxs.transpose(0, 1), []
            for a, b in zip(cuts[:-1], cuts[1:]):
                y, h = self.rnn(xs[a:b], (h * m[a].view(1, N, 1)).contiguous())
                pieces.append(y)
            y = torch.cat(pieces, dim=0).reshape(T * N, -1)
        return self.norm(y), h.transpose(0, 1)


class FixedNormal(torch.distributions.Normal):
    def log_probs(self, actions):
        return super().log_prob(actions)                # per dimension: no sum (module docstring)

    def mode(self):
        return self.mean


class DiagGaussian(nn.Module):
    def __init__(self, num_inputs, num_outputs, use_orthogonal=True, gain=0.01, config=None):
        super().__init__()
        if config is None:
            raise ValueError("DiagGaussian: config is required (actor_gain, std_x_coef, std_y_coef)")
        self.std_x_coef = config["std_x_coef"]
        self.std_y_coef = config["std_y_coef"]
        self.fc_mean = _init_linear(nn.Linear(num_inputs, num_outputs), use_orthogonal, config["actor_gain"])
        self.log_std = nn.Parameter(torch.ones(num_outputs) * self.std_x_coef)

    def forward(self, x, available_actions=None):
        return FixedNormal(self.fc_mean(x), torch.sigmoid(self.log_std / self.std_x_coef) * self.std_y_coef)


class ACTLayer(nn.Module):
    def __init__(self, action_space, inputs_dim, use_orthogonal, gain, args=None):
        super().__init__()
        self.mixed_action = self.multi_discrete = False
        self.action_type = action_space.__class__.__name__
        if self.action_type != "Box":
            raise NotImplementedError("ACTLayer: only Box action spaces are covered, got %s" % self.action_type)
        self.action_out = DiagGaussian(inputs_dim, action_space.shape[0], use_orthogonal, gain, args)

    def forward(self, x, available_actions=None, deterministic=False):
        dist = self.action_out(x, available_actions)
        actions = dist.mode() if deterministic else dist.sample()
        return actions, dist.log_probs(actions)

    def _entropy(self, dist, active_masks):
        if active_masks is None:
            return dist.entropy().mean()
        return (dist.entropy() * active_masks).sum() / active_masks.sum()

    def evaluate_actions(self, x, action, available_actions=None, active_masks=None):
        """(per-dimension log-probabilities [M, act_dim], the entropy: its mean, or its active_masks-weighted sum over active_masks.sum())"""
        dist = self.action_out(x, available_actions)
        return dist.log_probs(action), self._entropy(dist, active_masks)

    def evaluate_actions_trpo(self, x, action, available_actions=None, active_masks=None):
        """... and the distribution's mean and std (HATRPO's KL needs them) and None in the place of a Discrete space's logits"""
        dist = self.action_out(x, available_actions)
        return dist.log_probs(action), self._entropy(dist, active_masks), dist.mean, dist.stddev, None


class Actor(nn.Module):
    def __init__(self, config, obs_space, action_space, device=torch.device("cpu")):
        super().__init__()
        self.hidden_size = config["hidden_size"]
        self.config = config
        self._gain = config["gain"]
        self._use_orthogonal = config["use_orthogonal"]
        self._use_policy_active_masks = config["use_policy_active_masks"]
        self._use_naive_recurrent_policy = config["use_naive_recurrent_policy"]
        self._use_recurrent_policy = config["use_recurrent_policy"]
        self._recurrent_N = config["recurrent_N"]
        self.tpdv = dict(dtype=torch.float32, device=device)
        obs_shape = _shape_of(obs_space)
        if len(obs_shape) != 1:
            raise NotImplementedError("Actor: only flat observations (MLPBase) are covered, got shape %r" % (obs_shape,))
        self.base = MLPBase(config, obs_shape)
        if self._use_naive_recurrent_policy or self._use_recurrent_policy:
            self.rnn = RNNLayer(self.hidden_size, self.hidden_size, self._recurrent_N, self._use_orthogonal)
        self.act = ACTLayer(action_space, self.hidden_size, self._use_orthogonal, self._gain, config)
        self.to(device)

    def _features(self, obs, rnn_states, masks):
        obs, rnn_states, masks = (_tensor(t).to(**self.tpdv) for t in (obs, rnn_states, masks))
        features = self.base(obs)
        if self._use_naive_recurrent_policy or self._use_recurrent_policy:
            features, rnn_states = self.rnn(features, rnn_states, masks)
        return features, rnn_states

    def forward(self, obs, rnn_states, masks, available_actions=None, deterministic=False):
        """(actions, per-dimension action_log_probs, rnn_states: the new ones of a recurrent policy, else the argument)"""
        features, rnn_states = self._features(obs, rnn_states, masks)
        actions, action_log_probs = self.act(features, available_actions, deterministic)
        return actions, action_log_probs, rnn_states

    def evaluate_actions(self, obs, rnn_states, action, masks, available_actions=None, active_masks=None):
        """(action_log_probs, dist_entropy), and for config["algorithm_name"] == "hatrpo" (action_log_probs, dist_entropy, action_mu,
        action_std, all_probs = None).  active_masks weighs the entropy only with use_policy_active_masks."""
        features, _ = self._features(obs, rnn_states, masks)
        action = _tensor(action).to(**self.tpdv)
        am = _tensor(active_masks).to(**self.tpdv) if (active_masks is not None and self._use_policy_active_masks) else None
        if self.config["algorithm_name"] == "hatrpo":
            return self.act.evaluate_actions_trpo(features, action, available_actions, active_masks=am)
        return self.act.evaluate_actions(features, action, available_actions, active_masks=am)


class Critic(nn.Module):
    def __init__(self, config, cent_obs_space, device=torch.device("cpu")):
        super().__init__()
        self.hidden_size = config["hidden_size"]
        self._use_orthogonal = config["use_orthogonal"]
        self._use_naive_recurrent_policy = config["use_naive_recurrent_policy"]
        self._use_recurrent_policy = config["use_recurrent_policy"]
        self._recurrent_N = config["recurrent_N"]
        self.tpdv = dict(dtype=torch.float32, device=device)
        cent_obs_shape = _shape_of(cent_obs_space)
        if len(cent_obs_shape) != 1:
            raise NotImplementedError("Critic: only flat observations (MLPBase) are covered, got shape %r" % (cent_obs_shape,))
        self.base = MLPBase(config, cent_obs_shape)
        if self._use_naive_recurrent_policy or self._use_recurrent_policy:
            self.rnn = RNNLayer(self.hidden_size, self.hidden_size, self._recurrent_N, self._use_orthogonal)
        self.v_out = nn.Linear(self.hidden_size, 1)                    # (the reference initialises it with gain 0: the weight starts at zero)
        nn.init.constant_(self.v_out.weight.data, 0)
        nn.init.constant_(self.v_out.bias.data, 0)
        self.to(device)

    def forward(self, cent_obs, rnn_states, masks):
        """(values [M, 1], rnn_states)"""
        cent_obs, rnn_states, masks = (_tensor(t).to(**self.tpdv) for t in (cent_obs, rnn_states, masks))
        features = self.base(cent_obs)
        if self._use_naive_recurrent_policy or self._use_recurrent_policy:
            features, rnn_states = self.rnn(features, rnn_states, masks)
        return self.v_out(features), rnn_states

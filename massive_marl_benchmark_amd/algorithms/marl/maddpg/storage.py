"""ReplayBuffer of MADDPG (agents/algorithms/marl/maddpg/storage.py:5-93): one `[replay_size, num_envs, .]` transition ring per
agent.  Same constructor, fields (`obs`, `share_obs`, `rewards`, `next_observations`, `next_share_obs`, `actions`, `joint_actions`,
`dones`), cursor arithmetic and `random.sample` batches.

What is added:
  * `slot()`: the ring row the next `add_transitions` fills, so that whoever produces a transition (MADDPG.act_all's head kernel for
    `actions` / `joint_actions`, the engine's step kernel for next observations, rewards and dones) can write it in place;
    `add_transitions` recognises such rows by their address and copies only what is not there yet (rl/ddpg/storage.py's rule).
  * `joint_actions=None` (constructor keyword): a `[replay_size, num_envs, joint_act_dim]` tensor to use as this buffer's joint-action
    ring.  The reference stores N identical copies; handing every agent's buffer the same tensor stores one.
  * Padded rows.  `obs` and `next_observations` are views `[..., :K]` of `obs_padded` / `next_observations_padded`, whose row pitch
    is K rounded up to a multiple of 4 with zero padding (the grouped layer kernel takes K % 4 == 0; TenAnt's per-agent observation
    is 46 wide).  Nothing ever writes the padding: every store goes through the public views.

Reference behaviour kept on purpose: on overflow the cursor becomes (replay_size + 1) % replay_size = 1, not 0 (storage.py:49-53), so
row 0 keeps the first transition for ever; `mini_batch_generator` draws ROW indices with Python's `random.sample` (the same stream as
the reference for the same `random.seed`); `get_statistics` takes the mean reward over the WHOLE ring (storage.py:73)."""
import random

import torch


def round_up4(k):
    return (k + 3) // 4 * 4


class ReplayBuffer:
    def __init__(self, config, obs_shape, share_obs_shape, actions_shape, joint_actions_shape, device='cpu', joint_actions=None):
        num_envs = config["n_rollout_threads"]
        num_transitions_per_env = config["replay_size"]
        self.batch_size = config["batch_size"]
        self.device = device
        self.sampler = config["sampler"] if config.get("sampler") is not None else "random"
        joint_act_dim = sum(space.shape[0] for space in joint_actions_shape)
        R, N = num_transitions_per_env, num_envs
        z = lambda *s: torch.zeros(*s, device=self.device)

        def padded(shape):
            if len(shape) != 1:
                t = z(R, N, *shape)
                return t, t
            base = z(R, N, round_up4(shape[0]))
            return base, base[..., :shape[0]]
        self.obs_padded, self.obs = padded(tuple(obs_shape))
        self.share_obs = z(R, N, *share_obs_shape)
        self.rewards = z(R, N, 1)
        self.next_observations_padded, self.next_observations = padded(tuple(obs_shape))
        self.next_share_obs = z(R, N, *share_obs_shape)
        self.actions = z(R, N, *actions_shape)
        if joint_actions is None:
            joint_actions = z(R, N, joint_act_dim)
        elif tuple(joint_actions.shape) != (R, N, joint_act_dim):
            raise ValueError("joint_actions must be [%d, %d, %d], not %s" % (R, N, joint_act_dim, tuple(joint_actions.shape)))
        self.joint_actions = joint_actions
        self.dones = z(R, N, 1).byte()
        self.num_transitions_per_env = R
        self.num_envs = N
        self.fullfill = False
        self.step = 0

    def slot(self):
        """Ring row the next add_transitions writes (storage.py:49-53 applied ahead of time, without moving the cursor)."""
        return self.step if self.step < self.num_transitions_per_env else (self.step + 1) % self.num_transitions_per_env

    def add_transitions(self, observations, share_obs, actions, joint_actions, rewards, next_obs, next_state, dones):
        if self.step >= self.num_transitions_per_env:
            self.step = (self.step + 1) % self.num_transitions_per_env
            self.fullfill = True
        k = self.step

        def put(dst, src):
            in_place = src.data_ptr() == dst.data_ptr() and src.shape == dst.shape and src.stride() == dst.stride() and src.numel() > 0
            if not in_place:
                dst.copy_(src.view(dst.shape) if src.numel() == dst.numel() and src.dim() != dst.dim() else src)
        put(self.obs[k], observations)
        put(self.share_obs[k], share_obs)
        put(self.actions[k], actions)
        put(self.joint_actions[k], joint_actions)
        put(self.rewards[k], rewards.view(-1, 1))
        put(self.next_observations[k], next_obs)
        put(self.next_share_obs[k], next_state)
        put(self.dones[k], dones.view(-1, 1))
        self.step += 1

    def get_statistics(self):
        done = self.dones.clone()
        done[-1] = 1
        flat = done.permute(1, 0, 2).reshape(-1)
        ends = flat.nonzero(as_tuple=False)[:, 0]
        starts = torch.cat((ends.new_tensor([-1]), ends[:-1]))
        return (ends - starts).float().mean(), self.rewards.mean()

    def mini_batch_generator(self, num_mini_batches):
        """storage.py:75-93: num_mini_batches lists of batch_size // num_mini_batches distinct ring rows."""
        size = self.batch_size // num_mini_batches
        rows = range(self.num_transitions_per_env if self.fullfill else self.step)
        return [random.sample(rows, size) for _ in range(num_mini_batches)]

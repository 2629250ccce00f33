"""MLPActorCritic of TD3 (agents/algorithms/rl/td3/module.py): the DDPG one with twin Q networks `q1`, `q2` (:50-51)."""
from ..ddpg.module import MLPActor, MLPActorCritic as _DDPGActorCritic, MLPQFunction, fused_mlp_forward, fused_q_backup, fused_q_forward, mlp, split16_hidden  # noqa: F401


class MLPActorCritic(_DDPGActorCritic):
    def _build_q(self, obs_dim, act_dim, hidden_sizes, activation):
        self.q1 = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, self.layers)
        self.q2 = MLPQFunction(obs_dim, act_dim, hidden_sizes, activation, self.fused_q, self.layers)

    def _critics(self):
        return [self.q1, self.q2]      # q_backup: both in one chain

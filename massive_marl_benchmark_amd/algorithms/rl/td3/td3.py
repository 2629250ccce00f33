"""TD3, the learner (agents/algorithms/rl/td3/td3.py): ddpg.ddpg.DDPG -- the reference's two files differ in nothing else -- with twin
critics (`q1`, `q2`: both in the critic loss and the Bellman backup's min, `q1` alone in the policy loss) and `policy_delay`.  What the
reference's counter actually does with that key, the `learn` keys this package adds and `eps_source` are described there."""
import itertools

from ..ddpg.ddpg import DDPG
from .module import MLPActorCritic


class TD3(DDPG):
    ActorCritic = MLPActorCritic

    def _init_delay(self, learn_cfg):
        self.policy_delay = learn_cfg["policy_delay"]

    def _q_params(self):
        return itertools.chain(self.actor_critic.q1.parameters(), self.actor_critic.q2.parameters())

    def _policy_due(self, learn_ep):
        return learn_ep % self.policy_delay == 0           # td3.py:318, with learn_ep as the gather loop leaves it

"""agents/algorithms/rl/ppo/__init__.py exports RolloutStorage, ActorCritic and PPO: all three live here, the learner in ppo.py."""
from .module import ActorCritic  # noqa: F401
from .ppo import PPO  # noqa: F401
from .storage import RolloutStorage  # noqa: F401

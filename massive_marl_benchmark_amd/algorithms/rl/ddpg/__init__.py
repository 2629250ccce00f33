"""agents/algorithms/rl/ddpg/__init__.py exports ReplayBuffer, MLPActorCritic and DDPG: all three live here, the learner in ddpg.py."""
from .module import MLPActorCritic  # noqa: F401
from .storage import ReplayBuffer  # noqa: F401
from .ddpg import DDPG  # noqa: F401

"""agents/algorithms/rl/td3/__init__.py exports ReplayBuffer, MLPActorCritic and TD3: the learner lives in td3.py."""
from .module import MLPActorCritic  # noqa: F401
from .storage import ReplayBuffer  # noqa: F401
from .td3 import TD3  # noqa: F401

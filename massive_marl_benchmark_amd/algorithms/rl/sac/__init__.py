"""agents/algorithms/rl/sac/__init__.py exports ReplayBuffer, MLPActorCritic and SAC: all three live here, the learner in sac.py."""
from .module import MLPActorCritic  # noqa: F401
from .sac import SAC  # noqa: F401
from .storage import ReplayBuffer  # noqa: F401

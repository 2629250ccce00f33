"""agents/algorithms/rl/sac/__init__.py exports ReplayBuffer, MLPActorCritic and SAC; the learner class stays the reference's."""
from .module import MLPActorCritic  # noqa: F401
from .storage import ReplayBuffer  # noqa: F401

"""agents/algorithms/rl/trpo/__init__.py exports ActorCritic and RolloutStorage; the learner class stays the reference's."""
from .module import ActorCritic  # noqa: F401
from .storage import RolloutStorage  # noqa: F401

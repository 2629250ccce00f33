"""agents/algorithms/rl/trpo/__init__.py exports RolloutStorage, ActorCritic and TRPO: all three live here, the learner in trpo.py."""
from .module import ActorCritic  # noqa: F401
from .storage import RolloutStorage  # noqa: F401
from .trpo import TRPO  # noqa: F401

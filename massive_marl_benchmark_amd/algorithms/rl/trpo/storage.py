"""agents/algorithms/rl/trpo/storage.py is PPO's storage.py: one implementation here."""
from ..ppo.storage import RolloutStorage  # noqa: F401

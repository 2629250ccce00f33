"""MADDPG (agents/algorithms/marl/maddpg): the learner, its per-agent policy, the replay ring and the runner."""
from .module import MADDPG, MADDPG_policy
from .runner import Runner
from .storage import ReplayBuffer

__all__ = ["MADDPG", "MADDPG_policy", "ReplayBuffer", "Runner"]

from .actor_critic import ACTLayer, Actor, Critic, DiagGaussian, MLPBase, RNNLayer  # noqa: F401
from .hatrpo import HATRPO  # noqa: F401
from .policy import HAPPO_Policy, HATRPO_Policy, MAPPO_Policy  # noqa: F401
from .trainer import HAPPO, MAPPO  # noqa: F401

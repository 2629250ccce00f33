from .hatrpo import HATRPO  # noqa: F401
from .trainer import HAPPO, MAPPO  # noqa: F401

"""Time-conditioned layers ``layer(t, x)`` of the ODE nets.  The convolutional layers, ``ResNet`` / ``BasicBlock`` and
``MixtureODELayer`` of the reference are not built ("Continuous normalizing flows")."""
from .container import *  # noqa: F401,F403
from .basic import *  # noqa: F401,F403
from .wrappers import *  # noqa: F401,F403

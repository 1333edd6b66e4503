from .odefunc import *  # noqa: F401,F403
from . import diffeq_layers  # noqa: F401

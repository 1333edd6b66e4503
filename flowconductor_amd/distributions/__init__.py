from flowconductor_amd.distributions.base import Distribution, NoMeanException  # noqa: F401
from flowconductor_amd.distributions.discrete import ConditionalIndependentBernoulli  # noqa: F401
from flowconductor_amd.distributions.normal import (ConditionalDiagonalNormal, DiagonalNormal,  # noqa: F401
                                                     StandardNormal)
from flowconductor_amd.distributions.mixture import MADEMoG  # noqa: F401
from flowconductor_amd.distributions.uniform import LotkaVolterraOscillating, MG1Uniform  # noqa: F401

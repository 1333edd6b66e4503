"""Continuous normalizing flows (flowcon/CNF): ``cnf.CNF`` over ``neural_odes.ODEfunc`` / ``ODEnet``, the package's own
solver ``odeint`` and the ``CNFTransform`` adapter.  ``CompactCNF``, ``CompactTimeVariableCNF``, the convolutional
layers, ``ResNet`` / ``BasicBlock``, ``MixtureODELayer`` and ``squeeze`` of the reference are not built."""
from .cnf import CNF, CNFTransform  # noqa: F401

from flowconductor_amd.transforms.UMNN.MonotonicNormalizer import (  # noqa: F401
    ELUPlus,
    IntegrandNet,
    MonotonicNormalizer,
    cc_weights,
)

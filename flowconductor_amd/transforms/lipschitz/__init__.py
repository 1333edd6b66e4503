from flowconductor_amd.transforms.lipschitz.iresblock import (  # noqa: F401
    ApproxTraceDeterminantEstimator,
    BruteForceDeterminantEstimator,
    DeterminantEstimator,
    iResBlock,
)

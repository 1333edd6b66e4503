from flowconductor_amd.transforms.autoregressive import (  # noqa: F401
    AutoregressiveTransform,
    MaskedAffineAutoregressiveTransform,
    MaskedDeepSigmoidTransform,
    MaskedPiecewiseCubicAutoregressiveTransform,
    MaskedPiecewiseLinearAutoregressiveTransform,
    MaskedPiecewiseQuadraticAutoregressiveTransform,
    MaskedPiecewiseRationalQuadraticAutoregressiveTransform,
    MaskedShiftAutoregressiveTransform,
    MaskedSumOfSigmoidsTransform,
    MaskedUMNNAutoregressiveTransform,
)
from flowconductor_amd.transforms.base import (  # noqa: F401
    CompositeTransform,
    InputOutsideDomain,
    InverseNotAvailable,
    InverseTransform,
    MultiscaleCompositeTransform,
    Transform,
)
from flowconductor_amd.transforms.conditional import (  # noqa: F401
    AffineConditionalTransform,
    ConditionalLUTransform,
    ConditionalOrthogonalTransform,
    ConditionalPiecewiseRationalQuadraticTransform,
    ConditionalPlanarTransform,
    ConditionalRotationTransform,
    ConditionalScaleTransform,
    ConditionalShiftTransform,
    ConditionalSumOfSigmoidsTransform,
    ConditionalSVDTransform,
    ConditionalSylvesterTransform,
    ConditionalTransform,
    ConditionalUMNNTransform,
    PiecewiseLinearConditionalTransform,
)
from flowconductor_amd.transforms.coupling import (  # noqa: F401
    AdditiveCouplingTransform,
    AffineCouplingTransform,
    CouplingTransform,
    PiecewiseCubicCouplingTransform,
    PiecewiseLinearCouplingTransform,
    PiecewiseQuadraticCouplingTransform,
    PiecewiseRationalQuadraticCouplingTransform,
    UMNNCouplingTransform,
)
from flowconductor_amd.transforms.adaptive_sigmoids import DeepSigmoid, SumOfSigmoids  # noqa: F401
from flowconductor_amd.transforms.linear import Linear, NaiveLinear, ScalarScale, ScalarShift  # noqa: F401
from flowconductor_amd.transforms.lu import LULinear  # noqa: F401
from flowconductor_amd.transforms.qr import QRLinear  # noqa: F401
from flowconductor_amd.transforms.svd import SVDLinear  # noqa: F401
from flowconductor_amd.transforms.no_analytic_inv import (  # noqa: F401
    MonotonicTransform,
    PlanarTransform,
    RadialTransform,
    SylvesterTransform,
)
from flowconductor_amd.transforms.nonlinearities import (  # noqa: F401
    CauchyCDF,
    CauchyCDFInverse,
    CompositeCDFTransform,
    Exp,
    ExtendedSoftplus,
    GatedLinearUnit,
    LeakyReLU,
    Logit,
    LogTanh,
    PiecewiseCubicCDF,
    PiecewiseLinearCDF,
    PiecewiseQuadraticCDF,
    PiecewiseRationalQuadraticCDF,
    Sigmoid,
    Softplus,
    Tanh,
)
from flowconductor_amd.transforms.normalization import ActNorm, BatchNorm  # noqa: F401
from flowconductor_amd.transforms.orthogonal import HouseholderSequence, ParametrizedHouseHolder  # noqa: F401
from flowconductor_amd.transforms.permutations import (  # noqa: F401
    FillTriangular,
    Permutation,
    RandomPermutation,
    ReversePermutation,
)
from flowconductor_amd.transforms.standard import (  # noqa: F401
    AffineScalarTransform,
    AffineTransform,
    IdentityTransform,
    PointwiseAffineTransform,
)
from flowconductor_amd.transforms.matrix import (  # noqa: F401
    CholeskyOuterProduct,
    TransformDiagonal,
    TransformDiagonalExponential,
    TransformDiagonalSoftplus,
)
from flowconductor_amd.transforms.conv import OneByOneConvolution  # noqa: F401
from flowconductor_amd.transforms.reshape import SqueezeTransform  # noqa: F401
from flowconductor_amd.transforms.lipschitz import iResBlock  # noqa: F401
from flowconductor_amd.transforms.unitvector import UnitVector  # noqa: F401

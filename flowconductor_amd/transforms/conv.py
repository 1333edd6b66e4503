"""``OneByOneConvolution``: Glow's invertible 1x1 convolution (same class, constructor arguments, parameter and buffer
names as flowcon/transforms/conv.py, so reference checkpoints load with ``strict=True``).

The reference permutes the channels, moves them to rows, runs ``LULinear`` and moves them back: about five passes over
the tensor.  Here the permutation is folded into the kernel matrix -- the columns of ``W = L U`` (forward) or the rows
of ``W^-1`` (inverse, formed in float64 once per parameter version) -- and ``fc_conv1x1`` makes one pass over the NCHW
tensor.  The inverse subtracts the bias before the product.  More than ``ops.CONV1X1_MAX_CHANNELS`` channels take the
reference's composition (permutation + ``LULinear`` on rows + permutation back)."""
import torch

from flowconductor_amd import ops
from flowconductor_amd.transforms.lu import LULinear
from flowconductor_amd.transforms.permutations import RandomPermutation


class OneByOneConvolution(LULinear):
    """``y = W x_perm + b`` at every pixel of ``[B, C, H, W]`` inputs; logabsdet = ``H W sum log diag U`` per image."""

    _HIP_AUTOGRAD = True

    def __init__(self, num_channels, using_cache=False, identity_init=True):
        super().__init__(num_channels, using_cache, identity_init)
        self.permutation = RandomPermutation(num_channels, dim=1)

    def _inverse64(self):
        """``U^-1 L^-1`` in float64 (differentiable with respect to the parameters)."""
        lower, upper = self._create_lower_upper()
        eye = torch.eye(self.features, dtype=torch.float64, device=lower.device)
        l_inv = torch.linalg.solve_triangular(lower.double(), eye, upper=False, unitriangular=True)
        return torch.linalg.solve_triangular(upper.double(), l_inv, upper=True)

    def weight_inverse(self):
        return self._inverse64().to(self.lower_entries.dtype)

    def _fold(self, matrix, inverse):
        """The channel permutation folded into the kernel matrix: columns of W (forward), rows of W^-1 (inverse)."""
        inv = torch.argsort(self.permutation._permutation).to(matrix.device)
        return (matrix[inv, :] if inverse else matrix[:, inv]).contiguous()

    def _folded_nograd(self, inputs, inverse):
        """(kernel matrix, log|det W|) without autograd, memoised per parameter version.  With the cache active the
        LULinear cache is filled as for LULinear, and the memo lives exactly as long as the cached matrix does."""
        cached = None
        if self._cache_active(inputs):
            if inverse:
                self._check_inverse_cache()
                cached = self.cache.inverse
            else:
                self._check_forward_cache()
                cached = self.cache.weight
            key = ("cache", ops.cache_key(self.permutation._permutation), inverse)
        else:
            key = ops.cache_key(self.lower_entries, self.upper_entries, self.unconstrained_upper_diag,
                                self.permutation._permutation, extra=(inverse,))

        @torch.no_grad()
        def fold():
            if inverse:
                source = self._inverse64()
            else:
                lower, upper = self._create_lower_upper()
                source = lower.double() @ upper.double()
            matrix = self._fold(source, inverse).float()
            lad = self.logabsdet() if cached is None else self.cache.logabsdet
            return matrix, lad, cached       # (the entry keeps alive what its key names by id)

        return ops.memo(self, "conv1x1", (key, id(cached)), fold)[:2]

    def _lu_forward_inverse(self, inputs, inverse=False):
        """The reference's composition on rows (conv.py), for channel counts the kernel does not take."""
        b, c, h, w = inputs.shape
        rows = inputs.permute(0, 2, 3, 1).reshape(b * h * w, c)
        outputs, logabsdet = super().inverse(rows) if inverse else super().forward(rows)
        outputs = outputs.reshape(b, h, w, c).permute(0, 3, 1, 2)
        return outputs, logabsdet.reshape(b, h * w).sum(dim=1)

    def _map(self, inputs, inverse):
        b, c, h, w = inputs.shape
        if c > ops.CONV1X1_MAX_CHANNELS:
            if inverse:
                outputs, logabsdet = self._lu_forward_inverse(inputs, inverse=True)
                return self.permutation.inverse(outputs)[0], logabsdet
            return self._lu_forward_inverse(self.permutation(inputs)[0])
        if self._needs_grad(inputs):    # training: the kernel behind an autograd node, the matrix built differentiably
            if inverse:
                outputs = ops.conv1x1(inputs, self._fold(self._inverse64(), True).float(), pre=self.bias)
            else:
                lower, upper = self._create_lower_upper()
                outputs = ops.conv1x1(inputs, self._fold(lower @ upper, False), post=self.bias)
            lad = self.logabsdet() * (h * w)
        else:
            matrix, lad = self._folded_nograd(inputs, inverse)
            if inverse:
                outputs = ops.conv1x1(inputs, matrix, pre=self.bias.detach())
            else:
                outputs = ops.conv1x1(inputs, matrix, post=self.bias.detach())
            lad = lad * (h * w)
        return outputs, self._per_row(-lad if inverse else lad, b)

    def forward(self, inputs, context=None):
        if inputs.dim() != 4:
            raise ValueError("Inputs must be a 4D tensor.")
        return self._map(inputs, inverse=False)

    def inverse(self, inputs, context=None):
        if inputs.dim() != 4:
            raise ValueError("Inputs must be a 4D tensor.")
        return self._map(inputs, inverse=True)

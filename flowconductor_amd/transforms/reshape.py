"""``SqueezeTransform`` (same class, constructor argument, checks and messages as flowcon/transforms/reshape.py): trades
spatial size for channels.  Both directions are the bit-exact ``fc_squeeze`` HIP kernel, each the other's backward.
"""
from flowconductor_amd import ops
from flowconductor_amd.transforms.base import Transform
from flowconductor_amd.utils import typechecks as check


class SqueezeTransform(Transform):
    """``[B, C, H, W] -> [B, C f^2, H/f, W/f]`` in the element order of the reference's
    ``view(B, C, H/f, f, W/f, f).permute(0, 1, 3, 5, 2, 4)``; zero logabsdet.

    The inverse requires ``c >= 4 and c % 4 == 0`` whatever the factor, as the reference does (for f = 3 it therefore
    accepts only channel counts that are multiples of 36; a multiple of 4 that is not a multiple of f^2 fails in the
    reshape with torch's message)."""

    _HIP_AUTOGRAD = True

    def __init__(self, factor=2):
        super().__init__()
        if not check.is_int(factor) or factor <= 1:
            raise ValueError("Factor must be an integer > 1.")
        self.factor = factor

    def get_output_shape(self, c, h, w):
        return (c * self.factor * self.factor, h // self.factor, w // self.factor)

    def forward(self, inputs, context=None):
        if inputs.dim() != 4:
            raise ValueError("Expecting inputs with 4 dimensions")
        batch_size, c, h, w = inputs.size()
        if h % self.factor != 0 or w % self.factor != 0:
            raise ValueError("Input image size not compatible with the factor.")
        return ops.squeeze(inputs, self.factor), inputs.new_zeros(batch_size)

    def inverse(self, inputs, context=None):
        if inputs.dim() != 4:
            raise ValueError("Expecting inputs with 4 dimensions")
        batch_size, c, h, w = inputs.size()
        if c < 4 or c % 4 != 0:
            raise ValueError("Invalid number of channel dimensions.")
        f2 = self.factor ** 2
        if c % f2 != 0:
            shape = [batch_size, c // f2, self.factor, self.factor, h, w]
            raise RuntimeError("shape '%s' is invalid for input of size %d" % (str(shape).replace(" ", ""),
                                                                               inputs.numel()))
        return ops.squeeze(inputs, self.factor, inverse=True), inputs.new_zeros(batch_size)

"""Host-side checks of the SPD-matrix layers (no GPU): constructors, exports, state_dict keys, error bits."""
import numpy as np
import pytest
import torch

from _util import golden
from flowconductor_amd import _hip, ops, transforms


def test_exports():
    from flowconductor_amd.transforms import matrix

    for name in ("CholeskyOuterProduct", "TransformDiagonal", "TransformDiagonalSoftplus",
                 "TransformDiagonalExponential", "FillTriangular"):
        assert hasattr(transforms, name)
    assert transforms.CholeskyOuterProduct is matrix.CholeskyOuterProduct
    from flowconductor_amd.transforms.matrix.diagonal import fancy_exp_transform, fancy_softplus_transform

    assert isinstance(fancy_exp_transform, transforms.CompositeTransform)
    assert isinstance(fancy_softplus_transform, transforms.CompositeTransform)


def test_fill_triangular_constructor():
    for m in (1, 2, 5, 128):
        d = m * (m + 1) // 2
        assert transforms.FillTriangular.calc_matrix_dimension(d) == m
        assert transforms.FillTriangular.calc_n_ltri(m) == d
        t = transforms.FillTriangular(features=d)
        assert (t.features, t.matrix_dim) == (d, m)
        t = transforms.FillTriangular(matrix_dimension=m)
        assert (t.features, t.matrix_dim) == (d, m)
        assert [a.tolist() for a in t.lower_indices] == [a.tolist() for a in np.tril_indices(m)]
    with pytest.raises(ValueError, match="Provide either"):
        transforms.FillTriangular()
    with pytest.raises(ValueError, match="Provide either"):
        transforms.FillTriangular(features=3, matrix_dimension=2)
    with pytest.raises(AssertionError, match="invalid dimension"):
        transforms.FillTriangular.calc_matrix_dimension(4)
    with pytest.raises(AssertionError, match="Dimension must be positive"):
        transforms.FillTriangular.calc_matrix_dimension(0)


def test_parameters_and_default_inner_transform():
    c = transforms.CholeskyOuterProduct(5)
    assert c.checkargs and c.eps == 1e-6 and c.N == 5
    assert c.powers.dtype == torch.int64 and c.powers.tolist() == [[5, 4, 3, 2, 1]]
    assert torch.equal(c.eye, torch.eye(5).unsqueeze(0)) and not c.eye.requires_grad and not c.powers.requires_grad
    a, b = transforms.TransformDiagonal(3), transforms.TransformDiagonal(4)
    assert isinstance(a.diag_transform, transforms.Exp) and a.diag_transform is b.diag_transform
    assert not a.diag_mask.requires_grad and a.diag_mask.shape == (1, 3, 3)
    e = transforms.TransformDiagonalExponential(3, eps=1e-3)
    assert isinstance(e.diag_transform._transforms[0], transforms.Exp)
    assert float(e.diag_transform._transforms[1].shift) == pytest.approx(1e-3)


@pytest.mark.parametrize("m", [1, 3, 4, 17, 53, 64, 128])
def test_state_dict_keys_match_fixtures(m):
    g = golden("spd_m%d" % m)
    for name, mod in (("chol", transforms.CholeskyOuterProduct(m)), ("diag", transforms.TransformDiagonalSoftplus(m))):
        keys = sorted(k.split("::", 2)[2] for k in g.files if k.startswith("sd::%s::" % name))
        assert keys == sorted(mod.state_dict())
        sd = {k.split("::", 2)[2]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::%s::" % name)}
        mod.load_state_dict(sd, strict=True)


def test_error_bits_raise_reference_exceptions():
    cases = [(_hip.ERR_NOT_LOWER_TRIANGULAR, AssertionError, "lower triangular matrices$"),
             (_hip.ERR_DIAGONAL_NONPOSITIVE, AssertionError, "positive diagonal elements"),
             (_hip.ERR_NOT_SYMMETRIC, AssertionError, "not symmetric"),
             (_hip.ERR_NOT_POSITIVE_DEFINITE, AssertionError, "positive semi-definite"),
             (_hip.ERR_CHOLESKY_FAILED, torch.linalg.LinAlgError, "positive-definite")]
    for bit, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops._raise_for(bit)
    assert _hip.ABI_VERSION == 3


def test_step_aside_path_on_cpu_tensors():
    # m > 128 is the reference's torch composition (runs wherever torch does)
    m = 129
    c = transforms.CholeskyOuterProduct(m)
    low = torch.tril(torch.rand(2, m, m)) + torch.eye(m)
    y, lad = c(low)
    ref = low @ low.mT
    assert torch.allclose(y, 0.5 * (ref + ref.mT))
    with pytest.raises(AssertionError, match="lower triangular matrices$"):
        c(low.mT.contiguous())

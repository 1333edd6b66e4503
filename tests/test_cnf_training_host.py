"""Training-mode continuous normalizing flows, host side: the composition's gradients against the reference, the
differentiable net image, the limits, the option and the routing predicate.

Bounds: ``1e-5 max(1, max|expected|) + 4 floor`` with the fixture's recorded ``floor = max|ref32 - ref64|`` (float32), and
``1e-12 max(1, max|expected|)`` for the float64 composition against the float64 reference (the same operations in the
same order up to the BLAS: a few hundred float64 roundings of values of order 10)."""
import pytest
import torch

from flowconductor_amd import ops, options

import _cnf_training_util as U


@pytest.mark.parametrize("name,mode", U.FIXTURES)
def test_composition_meets_the_training_fixtures(name, mode):
    func, g = U.load_train_case(name, mode)
    data = U.fixture_data(g)
    got32, forward, backward = U.evaluate(func, data)
    got64, _, _ = U.evaluate(func, data, dtype=torch.float64)
    assert (forward, backward) == (0, 0)
    keys = [k[:-2] for k in g.files if k.endswith("64") and not k.startswith("sd::")]
    assert set(keys) == set(got32) and len(keys) >= 4
    for key in keys:
        e32, e64 = torch.from_numpy(g[key + "32"]), torch.from_numpy(g[key + "64"])
        bound = 1e-5 * U.scale_of(e32) + 4 * float(g["floor::" + key])
        assert U.worst(got32[key], e32) <= bound, (key, U.worst(got32[key], e32), bound)
        assert U.worst(got64[key], e64) <= 1e-12 * U.scale_of(e64), (key, U.worst(got64[key], e64))


def _hand_unpacked(func, kind, r):
    """``{parameter name: the entries of r that the image takes from it}`` by the layout of include/flowcon_hip.h, and
    the mask of the entries that are no parameter's."""
    out, at = {}, 0
    used = torch.zeros_like(r, dtype=torch.bool)
    for index, layer in enumerate(func.diffeq.layers):
        rows, cols = layer._layer.weight.shape
        width = cols - (kind == "concat")
        op = (rows + 3) & ~3
        vectors = {"b": "_layer.bias"}
        if kind in ("squash",):
            vectors.update(w_g="_hyper.weight", b_g="_hyper.bias")
        if kind == "concatsquash":
            vectors.update(w_g="_hyper_gate.weight", b_g="_hyper_gate.bias", w_b="_hyper_bias.weight")
        if kind == "concat_v2":
            vectors.update(w_b="_hyper_bias.weight")
        prefix = "diffeq.layers.%d." % index
        for slot, tag in enumerate(("b", "w_t", "w_g", "b_g", "w_b")):
            piece = slice(at + slot * op, at + slot * op + rows)
            if tag in vectors:
                shape = dict(func.named_parameters())[prefix + vectors[tag]].shape
                out[prefix + vectors[tag]] = r[piece].reshape(shape)
                used[piece] = True
        wt = r[at + 5 * op:at + (5 + width) * op].reshape(width, op)
        used[at + 5 * op:at + (5 + width) * op] = (torch.arange(op) < rows).repeat(width)
        weight = wt[:, :rows].t()
        if kind == "concat":        # column 0 of the weight multiplies t: the image's w_t
            piece = slice(at + op, at + op + rows)
            weight = torch.cat([r[piece].reshape(rows, 1), weight], dim=1)
            used[piece] = True
        out[prefix + "_layer.weight"] = weight
        at += (5 + width) * op
    assert at == r.numel()
    return out, ~used


@pytest.mark.parametrize("kind", ["ignore", "concat", "concat_v2", "squash", "concatsquash"])
def test_differentiable_image_unpacks_into_the_parameters(kind):
    func = U.make_train_func(3, (5, 6), layer_type=kind, seed=21)
    plan = func._kernel_plan()
    assert plan is not None
    image = func._pack_image(plan, differentiable=True)
    assert image.requires_grad and torch.equal(image.detach(), func._pack_image(plan))
    assert not func._pack_image(plan).requires_grad
    r = torch.randn(image.shape, generator=torch.Generator().manual_seed(22))
    names = [k for k, _ in func.named_parameters()]
    grads = dict(zip(names, torch.autograd.grad((image * r).sum(), [p for _, p in func.named_parameters()],
                                                retain_graph=True)))
    expected, padding = _hand_unpacked(func, kind, r)
    assert set(expected) == set(names) and bool(padding.any())
    for name in names:
        assert torch.equal(grads[name], expected[name]), name
    assert float(image.detach()[padding].abs().max()) == 0.0
    other = torch.where(padding, r + 1.0, r)            # the padding gets no weight
    again = torch.autograd.grad((image * other).sum(), [p for _, p in func.named_parameters()])
    for name, grad in zip(names, again):
        assert torch.equal(grad, grads[name]), name


def test_training_limits_and_the_lanes_rule():
    assert ops.cnf_train_supported(16, (64, 64, 64)) and ops.cnf_train_supported(1, ())
    assert not ops.cnf_train_supported(16, (64, 64, 64, 64)) and ops.cnf_supported(16, (64, 64, 64, 64))
    assert not ops.cnf_train_supported(17, (8,)) and not ops.cnf_train_supported(3, (65,))
    assert not ops.cnf_train_supported(0, ())
    assert ops.cnf_train_lanes(100, 2, True) == 200 and ops.cnf_train_lanes(100, 16, True) == 200
    assert ops.cnf_train_lanes(100, 2, False) == 400 and ops.cnf_train_lanes(100, 16, False) == 3200
    assert ops.cnf_train_lanes(100, 1, False) == 200
    for n, d, hutchinson in ((1, 2, True), (4096, 2, False), (1 << 20, 16, False)):
        assert ops.cnf_train_rows_pay(n, d, hutchinson) == (
            ops.cnf_train_lanes(n, d, hutchinson) <= ops.CNF_TRAIN_MAX_LANES)


def test_option_defaults_to_off_and_takes_three_values():
    assert options.get("cnf_training") is False
    for value in (True, False, "force"):
        with options.override(cnf_training=value):
            assert options.get("cnf_training") == value
    for value in ("on", "auto", 1, None):
        with pytest.raises(ValueError):
            with options.override(cnf_training=value):
                pass
    assert options.get("cnf_training") is False


def test_routing_predicate_is_false_off_the_device_route():
    func = U.make_train_func(3, (8, 8), seed=23)
    y = torch.randn(5, 3)
    zero = torch.zeros(5, 1)
    with options.override(cnf_training="force"):
        assert func._use_training_kernels(0.3, (y, zero)) is None                          # a CPU tensor
        assert func._use_training_kernels(0.3, (y.double(), zero.double())) is None        # float64
        assert func._use_training_kernels(0.3, (y, zero, zero)) is None                    # a regulariser's state
        t = torch.tensor(0.3, requires_grad=True)
        assert func._use_training_kernels(t, (y, zero)) is None                            # d/dt wanted
        before = func.num_evals()
        dy, negdiv = func(0.3, (y.requires_grad_(True), zero))                             # and the call goes through
        assert dy.requires_grad and negdiv.shape == (5, 1) and func.num_evals() == before + 1
    assert func._use_training_kernels(0.3, (y, zero)) is None                              # the option is off

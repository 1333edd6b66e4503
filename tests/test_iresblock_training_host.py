"""iResBlock training off the GPU (options ``iresblock_training``): the float64 restatement of ``fc_iresnet_backward``'s
reverse sweep (tests/_iresblock_training_util.py) against ``torch.autograd`` on the package's float64 composition, the
activations' derivatives against ``torch.autograd.functional``, the differentiable image builder against
``_pack_image``, the option and the ABI entry.

Tolerances: the sweep and autograd evaluate the same float64 expressions in different orders, so they agree to 1e-10
relative to the largest gradient magnitude of the case; the activation derivatives are closed forms against autograd of
closed forms, 1e-12 relative to max(1, |value|); the float32 image is a handful of float32 operations per entry away from
the float32 rounding of the float64 image: 2 ulp."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from flowconductor_amd import _hip, ops, options, transforms
from flowconductor_amd.nn import nets
from flowconductor_amd.nn.nets import activations

import _iresblock_training_util as U
from test_iresblock_host import BLOCKS, CONTEXT, load_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def seeded():
    """The nets that are not loaded from fixtures draw their initial weights and power-method vectors from torch's
    global generator."""
    torch.manual_seed(20261021)


ACT_IDS = {"relu": ops.IRES_ACT_RELU, "tanh": ops.IRES_ACT_TANH, "elu": ops.IRES_ACT_ELU, "swish": ops.IRES_ACT_SWISH,
           "lipswish": ops.IRES_ACT_LIPSWISH, "clipswish": ops.IRES_ACT_CLIPSWISH, "sin": ops.IRES_ACT_SIN,
           "csin": ops.IRES_ACT_CSIN, "leaky_lswish": ops.IRES_ACT_LEAKY_LSWISH}


def test_option_and_abi_entry():
    assert options.get("iresblock_training") is False
    with options.override(iresblock_training=True):
        assert options.get("iresblock_training") is True
    assert options.get("iresblock_training") is False
    for bad in (1, 0, "force", "yes", None):
        with pytest.raises(ValueError):
            with options.override(iresblock_training=bad):
                pass
    with open(os.path.join(ROOT, "include", "flowcon_hip.h")) as f:
        header = f.read()
    for name in ("fc_iresnet_backward", "fc_iresnet_backward_workspace"):
        assert name in _hip.SIGNATURES
        declared = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert declared, name
        assert len(declared.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert "iresblock_training" in ops.IRES_DOUBLE_BACKWARD_MSG
    assert callable(ops.iresnet_backward) and callable(ops.iresnet_autograd)


@pytest.mark.parametrize("name", sorted(ACT_IDS))
def test_activation_derivatives(name):
    """f against the module itself, f' and f'' against autograd of it, the p0 / p1 derivatives against autograd of the
    closed forms, on a grid that stays away from the kink of ReLU / ELU at zero."""
    act = ACT_IDS[name]
    module = U.ACTIVATIONS[name]()
    if isinstance(module, str):
        module = nets.invertible_densenet.ACTIVATION_FNS[module]()
    module = module.double()
    if name == "leaky_lswish":
        with torch.no_grad():
            module.alpha.fill_(-0.4)
    block = transforms.iResBlock(nets.DenseNet(dimension=2, activation_function=module))
    _, p0_fn, p1_fn = transforms.lipschitz.iresblock._kernel_activation(block.nnet.activation)
    scalar = lambda fn: torch.zeros((), dtype=torch.float64) if fn is None else torch.as_tensor(fn(), dtype=torch.float64).reshape(())
    p0, p1 = scalar(p0_fn).detach(), scalar(p1_fn).detach()
    t = torch.cat([torch.linspace(-3.1, -0.05, 17), torch.linspace(0.07, 2.9, 16)]).double()
    jet = U.act_jet(act, t, p0, p1)

    def through_module(v):
        return module(v.view(-1, 1))[:, 0]

    def check(tag, got, want):
        err = float((got - want).abs().max())
        assert err <= 1e-12 * max(1.0, float(want.abs().max())), (name, tag, err)

    with torch.no_grad():
        check("f", jet["f"], through_module(t))
        if act in ops.IRES_CONCAT_ACTS:
            check("f(-t)", U.act_jet(act, -t, p0, p1)["f"], module(t.view(-1, 1))[:, 1])
    check("df", jet["df"], torch.autograd.functional.jacobian(lambda v: through_module(v).sum(), t))
    check("d2f", jet["d2f"], torch.autograd.functional.hessian(lambda v: through_module(v).sum(), t).diagonal())
    for key, slot in (("p0", 0), ("p1", 1)):
        for which in ("f", "df"):
            want = torch.autograd.functional.jacobian(
                lambda p: U.act_jet(act, t, p if slot == 0 else p0, p if slot == 1 else p1)[which],
                p0 if slot == 0 else p1)
            if act in (ops.IRES_ACT_RELU, ops.IRES_ACT_TANH) or (slot == 1 and act != ops.IRES_ACT_LEAKY_LSWISH):
                assert float(jet[which + "_" + key].abs().max()) == 0.0
            else:
                check(which + "_" + key, jet[which + "_" + key], want.reshape(-1))


def sweep_gradients(block64, plan, x, context, gy, gl):
    context = None if context is None else context.detach().clone().requires_grad_(True)
    block64.zero_grad()
    extra, scale = block64._extras(plan, context, differentiable=True)
    image = block64._training_image(plan)
    detach = lambda v: None if v is None else v.detach()
    y, lad, dx, dimage, dextra, dscale = U.reverse_sweep(image.detach(), block64._shape_args(plan), x, gy, gl,
                                                         detach(extra), detach(scale))
    roots = [(image, dimage)] + [(a, b) for a, b in ((extra, dextra), (scale, dscale)) if a is not None]
    torch.autograd.backward([a for a, _ in roots], [b for _, b in roots])
    grads = {"x": dx}
    if context is not None:
        grads["context"] = context.grad.clone()
    for name, p in block64.named_parameters():
        if p.grad is not None:
            grads[name] = p.grad.clone()
    block64.zero_grad()
    return grads, (y, lad)


CASES = [("dense", act, d) for act in sorted(ACT_IDS) for d in (1, 3)] + \
        [(kind, act, d) for kind, act in (("input", "swish"), ("multiplicative", "clipswish")) for d in (1, 3)]


@pytest.mark.parametrize("kind,act,d", CASES)
def test_reverse_sweep_against_autograd(kind, act, d):
    if kind == "dense":
        net = nets.DenseNet(dimension=d, densenet_depth=2, densenet_growth=8, activation_function=U.ACTIVATIONS[act]())
    else:
        net = U.conditional_net(kind, d, act)
    block64 = U.double_copy(U.make_block(net, 7 + d, context_features=0 if kind == "dense" else CONTEXT))
    plan = block64._kernel_plan()
    assert plan is not None and plan[0] == ACT_IDS[act]
    gen = torch.Generator().manual_seed(100 + d)
    x = torch.randn(5, d, generator=gen).double()
    context = None if kind == "dense" else torch.randn(5, CONTEXT, generator=gen).double()
    gy, gl = torch.randn(5, d, generator=gen).double(), torch.randn(5, generator=gen).double()
    ref, (y_ref, lad_ref) = U.named_gradients(block64, x, context, gy, gl)
    got, (y, lad) = sweep_gradients(block64, plan, x, context, gy, gl)
    assert set(got) == set(ref) and len(ref) > 5
    scale = max(float(v.abs().max()) for v in ref.values())
    assert float((y - y_ref).abs().max()) <= 1e-12 * max(1.0, float(y_ref.abs().max()))
    assert float((lad - lad_ref).abs().max()) <= 1e-12 * max(1.0, float(lad_ref.abs().max()))
    for name in sorted(ref):
        err = float((got[name] - ref[name]).abs().max())
        assert err <= 1e-10 * scale, (kind, act, d, name, err, scale)
    # the spectral clamp is active somewhere, so the gradient went through sigma
    originals = [n for n in ref if n.endswith("parametrizations.weight.original")]
    assert originals and all(float(ref[n].abs().max()) > 0 for n in originals)


@pytest.mark.parametrize("name", sorted(set(BLOCKS) - {"last_layer"}))
def test_differentiable_image_matches_pack_image(name):
    for block in (load_block(name)[0],
                  U.make_block(BLOCKS[name][0](), 3, context_features=CONTEXT if BLOCKS[name][1] else 0)):
        plan = block._kernel_plan()
        with torch.no_grad():
            got = block._training_image(plan)
        want = block._pack_image(plan)
        assert got.dtype == torch.float32 and got.shape == want.shape
        ulps = np.abs(got.numpy().astype(np.float64) - want.numpy().astype(np.float64)) / np.spacing(np.abs(want.numpy()))
        print("%s: largest distance %.2f ulp" % (name, ulps.max()))
        assert ulps.max() <= 2.0, (name, float(ulps.max()))
        assert torch.equal(got == 0, want == 0)      # the padding
    # differentiable, and not cached across calls
    image = block._training_image(plan)
    assert image.requires_grad and block._training_image(plan) is not image


def test_builder_reads_each_weight_once():
    """A training-mode build of the image moves the power-method vectors exactly as one composition call does."""
    block = U.make_block(nets.DenseNet(dimension=3, densenet_depth=2, densenet_growth=8), 5).train()
    a, b = copy.deepcopy(block), copy.deepcopy(block)
    a(torch.randn(4, 3, generator=torch.Generator().manual_seed(1)))
    b._training_image(b._kernel_plan())
    moved = 0
    for (name, u), (_, v), (_, w) in zip(a.named_buffers(), b.named_buffers(), block.named_buffers()):
        if name.endswith("._u") or name.endswith("._v"):
            assert torch.equal(u, v), name
            moved += int(not torch.equal(u, w))
    assert moved > 0

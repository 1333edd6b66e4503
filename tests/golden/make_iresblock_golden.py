"""Generate tests/golden/iresblock_*.npz (invertible residual blocks over Lipschitz DenseNets) by importing the
REFERENCE (FlowConductor) itself.

Runs only where the reference tree exists:
    python tests/golden/make_iresblock_golden.py
It uses make_golden.py's import.  Every block gets non-trivial weights before recording: the ``original`` weights of
alternate layers are scaled up and down so that both branches of the soft normalisation ``W / max(1, sigma / coeff)``
occur in every net (asserted), biases / concatenation weights / activation parameters are perturbed, 30 training-mode
passes let ``_u`` / ``_v`` converge, then ``eval()``.

- iresblock_<case>.npz for the cases of ``BLOCKS``: ``sd::`` state_dict entries, ``x`` (and ``context``), the reference's
  eval-mode float32 ``y32`` / ``lad32``, the same from a float64 deep copy (``y64`` / ``lad64``); for the inverse ``inv_in``,
  ``inv_x32`` / ``inv_lad32``, ``inv_x64`` / ``inv_lad64`` and ``inv_x64_exact``: the float64 fixed point iterated until the
  step is below 1e-13.  The script asserts that the reference's own loop ends before its 1000-iteration cap and prints
  the iteration counts and the float32 noise floors max|ref32 - ref64|.
- iresblock_toy_flow.npz: the 10 x (ActNorm, iResBlock) flow of the reference's examples/toy_2d.py: ``log_prob`` of
  fixed inputs and ``_transform.inverse`` of fixed noise, float32 and float64.
- iresblock_train.npz: training-mode ``forward`` under ``torch.manual_seed`` / ``np.random.seed`` for the unbiased
  Neumann, the biased basic and the brute-force estimator, with the gradient of ``logabsdet.sum()`` with respect to every
  parameter (``<mode>::grad::<name>``).
These fixtures are not part of cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

ROWS = 64
CONTEXT = 3


def blocks(L):
    """name -> (constructor of the contractive net, needs a context)."""
    N = L.nets.invertible_densenet
    A = L.nets.activations
    small = dict(c_embed_hidden_sizes=(16, 16, 6))
    return {
        "toy": (lambda: N.DenseNet(dimension=2, densenet_depth=3, densenet_growth=16, activation_function=A.CSin(10)),
                False),
        "default8": (lambda: N.DenseNet(dimension=8), False),
        "wide16": (lambda: N.DenseNet(dimension=16, densenet_depth=4, densenet_growth=28), False),
        "lipswish": (lambda: N.DenseNet(dimension=4, activation_function=A.LipSwish()), False),
        "tanh": (lambda: N.DenseNet(dimension=5, densenet_growth=12, activation_function="tanh"), False),
        "elu": (lambda: N.DenseNet(dimension=5, densenet_growth=12, activation_function="elu"), False),
        "relu": (lambda: N.DenseNet(dimension=5, densenet_growth=12, activation_function="relu"), False),
        "d1": (lambda: N.DenseNet(dimension=1), False),
        "input_conditional": (lambda: N.InputConditionalDenseNet(
            dimension=4, context_features=CONTEXT, densenet_depth=2, activation_function=A.Swish(), **small), True),
        "multiplicative_input": (lambda: N.MultiplicativeAndInputConditionalDenseNet(
            dimension=4, context_features=CONTEXT, densenet_depth=2, activation_function="CLipSwish",
            m_embed_hidden_sizes=(16, 16), **small), True),
        "last_layer": (lambda: N.LastLayerConditionalDenseNet(
            dimension=3, context_features=CONTEXT, densenet_depth=2, activation_function="CLipSwish"), True),
    }


def roughen(block, gen, x, context):
    """Non-trivial weights, converged power-method vectors, eval mode.  Returns sigma / coeff per normalised layer."""
    with torch.no_grad():
        index = 0
        for name, p in block.nnet.named_parameters():
            if name.endswith("parametrizations.weight.original"):
                p.mul_(2.5 if index % 2 == 0 else 0.6)
                index += 1
            elif name.endswith("bias") and "dense_net" in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
            elif "unnormalized" in name or name.endswith("beta"):
                p.add_(0.3 * torch.randn(p.shape, generator=gen))
        for name, b in block.nnet.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=gen))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=gen))
    block.train()
    for m in block.modules():                     # the running statistics set above stay as they are
        if isinstance(m, torch.nn.BatchNorm1d):
            m.eval()
    for _ in range(30):
        block(x.clone(), context)
    block.eval()
    ratios = []
    with torch.no_grad():
        for name, mod in block.nnet.named_modules():
            if hasattr(mod, "parametrizations"):
                par = mod.parametrizations.weight
                sigma = torch.dot(par[0]._u, torch.mv(par.original, par[0]._v)).item()
                ratios.append(sigma / par[0].coeff)
    assert any(r > 1 for r in ratios) and any(r < 1 for r in ratios), ratios
    return ratios


def count_calls(block):
    counter = [0]
    handle = block.nnet.register_forward_hook(lambda *a: counter.__setitem__(0, counter[0] + 1))
    return counter, handle


def exact_fixed_point(block64, y64, context64):
    with torch.no_grad():
        x = y64 - block64.nnet(y64, context64)
        for i in range(20000):
            new = y64 - block64.nnet(x, context64)
            step = (new - x).abs().max().item()
            x = new
            if step < 1e-13:
                return x, i + 1
    raise AssertionError("the float64 iteration did not reach a 1e-13 step (last %g)" % step)


def record(L, name, build, conditional, gen):
    block = L.transforms.lipschitz.iresblock.iResBlock(build(), brute_force=True)
    d = block.nnet.dimension
    x = torch.randn(ROWS, d, generator=gen)
    noise = torch.randn(ROWS, d, generator=gen)
    context = torch.randn(ROWS, CONTEXT, generator=gen) if conditional else None
    ratios = roughen(block, gen, x, context)
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in block.state_dict().items()}
    out["x"], out["inv_in"] = x.numpy(), noise.numpy()
    if conditional:
        out["context"] = context.numpy()
    block64 = copy.deepcopy(block).double()
    c64 = context.double() if conditional else None
    with torch.no_grad():
        y, lad = block(x.clone(), context)
        y_again, lad_again = block(x.clone(), context)
        assert torch.equal(y, y_again) and torch.equal(lad, lad_again)
        y64, lad64 = block64(x.double(), c64)
        counter, handle = count_calls(block)
        xi, ladi = block.inverse(noise.clone(), context)
        handle.remove()
        ref_iterations = counter[0] - 2          # x0 and the final logabsdet pass are not loop iterations
        assert ref_iterations < 1000, ref_iterations
        xi64, ladi64 = block64.inverse(noise.double(), c64)
    exact, iterations64 = exact_fixed_point(block64, noise.double(), c64)
    for key, value in (("y32", y), ("lad32", lad), ("y64", y64), ("lad64", lad64), ("inv_x32", xi), ("inv_lad32", ladi),
                       ("inv_x64", xi64), ("inv_lad64", ladi64), ("inv_x64_exact", exact)):
        out[key] = value.detach().numpy()
    print("%-22s sigma/coeff %s | floor y %.2e lad %.2e inv x %.2e inv lad %.2e | inverse: reference %d iterations, "
          "%.2e from the float64 fixed point (float64: %d iterations)"
          % (name, " ".join("%.2f" % r for r in ratios), (y.double() - y64).abs().max(),
             (lad.double() - lad64).abs().max(), (xi.double() - xi64).abs().max(),
             (ladi.double() - ladi64).abs().max(), ref_iterations, (xi.double() - exact).abs().max(), iterations64))
    np.savez_compressed(os.path.join(HERE, "iresblock_%s.npz" % name), **out)


def toy_flow(L, gen):
    T = L.transforms
    A = L.nets.activations
    factory = (T.lipschitz.iresblock.iResBlock.Factory().set_logabsdet_estimator(brute_force=True)
               .set_densenet(dimension=2, densenet_depth=3, densenet_growth=16, activation_function=A.CSin(10)))
    layers = []
    for _ in range(10):
        layers += [T.ActNorm(features=2), factory.build()]
    flow = L.flows.Flow(T.CompositeTransform(layers), L.distributions.StandardNormal(shape=[2]))
    data = torch.randn(256, 2, generator=gen) * torch.tensor([1.5, 0.7]) + torch.tensor([0.3, -0.4])
    for layer in layers[1::2]:
        roughen(layer, gen, torch.randn(ROWS, 2, generator=gen), None)
    flow.train()
    flow.log_prob(data)                      # data-dependent ActNorm initialisation
    flow.eval()
    x = torch.randn(ROWS, 2, generator=gen) * 1.2
    noise = torch.randn(ROWS, 2, generator=gen)
    flow64 = copy.deepcopy(flow).double()
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in flow.state_dict().items()}
    with torch.no_grad():
        lp = flow.log_prob(x.clone())
        lp64 = flow64.log_prob(x.double())
        s, lad = flow._transform.inverse(noise.clone())
        s64, lad64 = flow64._transform.inverse(noise.double())
    out.update(x=x.numpy(), noise=noise.numpy(), log_prob32=lp.numpy(), log_prob64=lp64.numpy(), sample32=s.numpy(),
               sample_lad32=lad.numpy(), sample64=s64.numpy(), sample_lad64=lad64.numpy())
    print("toy_flow               floor log_prob %.2e sample %.2e sample lad %.2e"
          % ((lp.double() - lp64).abs().max(), (s.double() - s64).abs().max(), (lad.double() - lad64).abs().max()))
    np.savez_compressed(os.path.join(HERE, "iresblock_toy_flow.npz"), **out)


TRAIN_MODES = {
    "unbiased_neumann": dict(brute_force=False, unbiased_estimator=True, trace_estimator="neumann"),
    "biased_basic": dict(brute_force=False, unbiased_estimator=False, trace_estimator="basic"),
    "brute_force": dict(brute_force=True),
}
TRAIN_SEED = 7


def train_case(L, gen):
    N = L.nets.invertible_densenet
    x = torch.randn(16, 3, generator=gen)
    out = {"x": x.numpy()}
    state = None
    for mode, kwargs in TRAIN_MODES.items():
        block = L.transforms.lipschitz.iresblock.iResBlock(N.DenseNet(dimension=3), **kwargs)
        if state is None:
            roughen(block, gen, x, None)
            state = {k: v.detach().clone() for k, v in block.state_dict().items()}
            out.update({"sd::" + k: v.numpy() for k, v in state.items()})
        block.load_state_dict(state, strict=True)
        block.train()
        torch.manual_seed(TRAIN_SEED)
        np.random.seed(TRAIN_SEED)
        y, lad = block(x.clone())
        lad.sum().backward()
        out[mode + "::y"], out[mode + "::lad"] = y.detach().numpy(), lad.detach().numpy()
        for name, p in block.named_parameters():
            if p.grad is not None:
                out[mode + "::grad::" + name] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "iresblock_train.npz"), **out)


def main():
    L = import_reference()
    import flowcon.transforms.lipschitz.iresblock  # noqa: F401  (not imported by the reference's package init)
    import flowcon.nn.nets.invertible_densenet  # noqa: F401
    L.transforms.lipschitz = flowcon.transforms.lipschitz
    L.nets.invertible_densenet = flowcon.nn.nets.invertible_densenet
    L.nets.activations = flowcon.nn.nets.activations
    for seed, (name, (build, conditional)) in enumerate(blocks(L).items()):
        record(L, name, build, conditional, torch.Generator().manual_seed(100 + seed))
    toy_flow(L, torch.Generator().manual_seed(200))
    train_case(L, torch.Generator().manual_seed(300))


if __name__ == "__main__":
    main()

"""Time the invertible-residual-block kernels against this package's own torch composition on the same GPU.

    python tools/bench_iresblock.py [--out FILE.json] [--repeats R] [--sizes 4096 65536 1048576]

Both sides are timed the same way: device events around one eval-mode ``forward`` / ``inverse`` call under
``torch.no_grad()``, a warm-up call first, the median of R repeats.  The composition is the same module with the
kernels switched off (``iResBlock._use_kernels`` returning None), i.e. D autograd passes + ``slogdet`` for the forward
and the batch-wide fixed-point loop for the inverse.  Blocks: the reference's toy block (D 2, depth 3, growth 16,
CSin(10)) and the default block (depth 2, growth 16, CLipSwish) at D = 8 and 16; plus ``log_prob`` and ``sample`` of
the 10 x (ActNorm, iResBlock) toy flow.  The inverse's largest per-row iteration count is recorded.  Prints one JSON
document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flowconductor_amd import _hip, distributions, flows, transforms  # noqa: E402
from flowconductor_amd.nn import nets  # noqa: E402
from flowconductor_amd.nn.nets import activations  # noqa: E402

DEV = torch.device("cuda:0")


def roughen(block, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for index, (name, p) in enumerate((n, p) for n, p in block.nnet.named_parameters()
                                          if n.endswith("parametrizations.weight.original")):
            p.mul_(2.5 if index % 2 == 0 else 0.6)
    block.train()
    for _ in range(30):
        block(torch.randn(64, block.nnet.dimension, generator=gen))
    return block.eval()


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times)


class composition:
    """Switch the kernels of every iResBlock under ``module`` off for the duration."""

    def __init__(self, module):
        self.blocks = [m for m in module.modules() if isinstance(m, transforms.iResBlock)]

    def __enter__(self):
        for b in self.blocks:
            b._use_kernels = lambda inputs, context: None

    def __exit__(self, *exc):
        for b in self.blocks:
            del b._use_kernels


def bench_block(name, block, sizes, repeats, budget_rows):
    rows = []
    d = block.nnet.dimension
    for n in sizes:
        x = torch.randn(n, d, device=DEV)
        entry = {"block": name, "n": n}
        with torch.no_grad():
            y, _ = block(x)
            entry["forward_kernel_ms"] = timed(lambda: block(x), repeats)
            entry["inverse_kernel_ms"] = timed(lambda: block.inverse(y), repeats)
            entry["inverse_kernel_iterations"] = block.inverse_iterations()
            if n <= budget_rows:
                with composition(block):
                    entry["forward_composition_ms"] = timed(lambda: block(x), max(3, repeats // 4))
                    entry["inverse_composition_ms"] = timed(lambda: block.inverse(y), max(3, repeats // 4))
                entry["forward_speedup"] = entry["forward_composition_ms"] / entry["forward_kernel_ms"]
                entry["inverse_speedup"] = entry["inverse_composition_ms"] / entry["inverse_kernel_ms"]
        rows.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
    return rows


def toy_flow():
    factory = (transforms.iResBlock.Factory().set_logabsdet_estimator(brute_force=True)
               .set_densenet(dimension=2, densenet_depth=3, densenet_growth=16,
                             activation_function=activations.CSin(10)))
    layers = []
    for i in range(10):
        layers += [transforms.ActNorm(features=2), roughen(factory.build(), 50 + i)]
    return flows.Flow(transforms.CompositeTransform(layers), distributions.StandardNormal(shape=[2])).eval().to(DEV)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out")
    parser.add_argument("--repeats", type=int, default=20)
    parser.add_argument("--sizes", type=int, nargs="+", default=[2 ** 12, 2 ** 16, 2 ** 20])
    parser.add_argument("--composition-rows", type=int, default=2 ** 20,
                        help="largest batch at which the composition is timed too")
    args = parser.parse_args()
    torch.manual_seed(0)
    blocks = {
        "toy_d2_depth3_csin": transforms.iResBlock(nets.DenseNet(
            dimension=2, densenet_depth=3, densenet_growth=16, activation_function=activations.CSin(10)),
            brute_force=True),
        "default_d8": transforms.iResBlock(nets.DenseNet(dimension=8), brute_force=True),
        "default_d16": transforms.iResBlock(nets.DenseNet(dimension=16), brute_force=True),
    }
    result = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "library": _hip.library_info(),
              "repeats": args.repeats, "blocks": [], "flow": []}
    for seed, (name, block) in enumerate(blocks.items()):
        result["blocks"] += bench_block(name, roughen(block, seed).to(DEV), args.sizes, args.repeats,
                                        args.composition_rows)
    flow = toy_flow()
    for n in args.sizes:
        x = torch.randn(n, 2, device=DEV)
        entry = {"flow": "toy_10_layers", "n": n}
        with torch.no_grad():
            entry["log_prob_kernel_ms"] = timed(lambda: flow.log_prob(x), args.repeats)
            entry["sample_kernel_ms"] = timed(lambda: flow.sample(n), args.repeats)
            if n <= args.composition_rows:
                with composition(flow):
                    entry["log_prob_composition_ms"] = timed(lambda: flow.log_prob(x), 3)
                    entry["sample_composition_ms"] = timed(lambda: flow.sample(n), 3)
                entry["log_prob_speedup"] = entry["log_prob_composition_ms"] / entry["log_prob_kernel_ms"]
                entry["sample_speedup"] = entry["sample_composition_ms"] / entry["sample_kernel_ms"]
        result["flow"].append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()

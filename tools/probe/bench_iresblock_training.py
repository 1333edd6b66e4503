"""Time a training step of invertible residual blocks on the one-node kernel route (options ``iresblock_training``)
against this package's own torch composition on the same GPU.

    python tools/probe/bench_iresblock_training.py [--out FILE.json] [--repeats R] [--sizes 4096 65536 1048576]

Both routes are timed the same way: device events around one ``train()``-mode forward + backward of the block (loss
``logabsdet.sum() + (y ** 2).sum()``, gradients to the rows and every parameter), a warm-up call first, the median and
the spread (min, max) of R repeats; the peak of ``torch.cuda.max_memory_allocated`` over one call is recorded for
either route.  Blocks: the three of DESIGN.md's iResBlock table -- the reference's toy block (D 2, depth 3, growth 16,
CSin(10)) and the default block (depth 2, growth 16, CLipSwish) at D = 8 and 16 -- plus one training step
(``-log_prob.mean()``, backward) of the 10 x (ActNorm, iResBlock) toy flow.  The composition is skipped above
``--composition-rows`` rows (its double backward keeps every Jacobian row's graph).  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from flowconductor_amd import _hip, distributions, flows, options, transforms  # noqa: E402
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
    return block


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
            "peak_mib": peak / 2 ** 20}


def both_routes(entry, step, n, repeats, composition_rows):
    with options.override(iresblock_training=True):
        entry["kernel"] = timed(step, repeats)
    if n <= composition_rows:
        with options.override(iresblock_training=False):
            entry["composition"] = timed(step, max(3, repeats // 4))
        entry["speedup"] = entry["composition"]["median_ms"] / entry["kernel"]["median_ms"]
    print(json.dumps(entry), file=sys.stderr, flush=True)
    return entry


def block_step(block, x):
    def step():
        block.zero_grad(set_to_none=True)
        x.grad = None
        y, lad = block(x)
        (lad.sum() + (y ** 2).sum()).backward()
    return step


def toy_flow():
    factory = (transforms.iResBlock.Factory().set_logabsdet_estimator(brute_force=True)
               .set_densenet(dimension=2, densenet_depth=3, densenet_growth=16,
                             activation_function=activations.CSin(10)))
    layers = []
    for i in range(10):
        layers += [transforms.ActNorm(features=2), roughen(factory.build(), 50 + i)]
    return flows.Flow(transforms.CompositeTransform(layers), distributions.StandardNormal(shape=[2])).train().to(DEV)


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
        block = roughen(block, seed).to(DEV)
        for n in args.sizes:
            x = torch.randn(n, block.nnet.dimension, device=DEV, requires_grad=True)
            result["blocks"].append(both_routes({"block": name, "n": n}, block_step(block, x), n, args.repeats,
                                                args.composition_rows))
    flow = toy_flow()
    for n in args.sizes:
        x = torch.randn(n, 2, device=DEV)

        def step():
            flow.zero_grad(set_to_none=True)
            (-flow.log_prob(x).mean()).backward()

        result["flow"].append(both_routes({"flow": "toy_10_layers", "n": n}, step, n, args.repeats,
                                          args.composition_rows))
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()

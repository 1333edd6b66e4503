"""Generate tests/golden/bernoulli_*.npz, bernoulli_sample_*.npz, box_d*.npz and sbi_priors.npz by importing the REFERENCE
(FlowConductor) itself.

Runs only where the reference tree exists:
    python tests/golden/make_distributions_golden.py
It uses make_golden.py's import.  The storage scheme is make_rownorm_golden.py's: the reference's float32 results, the results
of a ``.double()`` copy on the same inputs, and the float32 noise floors max|float32 - float64|; [N, D] float64 arrays are kept
as float32 differences to the float32 array or rounded to float32 (gradients), so that every file stays under the size limit.

  bernoulli_{d1,d3,d64,d65,d130,d784,s2x3x5}   ``ConditionalIndependentBernoulli(shape, encoder)`` on 257 rows (33 at D = 784).
      The encoder is a seeded ``nn.Linear(4, D)`` (``sd::`` entries: the distribution's state_dict) on contexts 40 randn, so
      that every case has logits beyond +-30 and within +-1 (asserted); d65 uses the identity encoder on such logits.  Inputs
      are exactly 0 / 1, in s2x3x5 uniform on [0, 1].  Stored: ``context``, ``x``, ``g``; ``logp32`` / ``logp64`` /
      ``floor_logp``; ``mean32`` / ``mean64_minus_mean32`` / ``floor_mean``; the float64 gradients of ``(log_prob * g).sum()``
      with respect to the logits, the inputs and the encoder's parameters (``grad_logits64``, ``grad_x64``,
      ``grad64::<name>``) and the floors of the float32 gradients against them (``floor_grad_logits``, ``floor_grad_x``,
      ``floor_grad::<name>``).
  bernoulli_sample_{c5s7,c4s1}   identity encoder, logits 3 randn of shape [5, 784] / [4, 2, 3, 5]; ``noise`` is what the
      reference's ``_sample`` draws under ``torch.manual_seed(seed)`` (checked: ``samples32`` equals ``noise <
      sigmoid(logits)`` on repeated rows); ``samples64`` the same comparison in float64.  The two agree everywhere and no
      element has |noise - sigmoid64(logits)| < 1e-6 (the seed is advanced until both hold), so a float32 sigmoid that is
      good to 1e-6 reproduces ``samples32`` exactly.
  box_d{1,3,64,130}   ``BoxUniform(low, high)`` built with validation off: 257 rows, about a third outside the box, row 0
      exactly on ``low`` (inside), row 1 with one coordinate exactly on ``high`` (outside), row 2 with a NaN.  ``logp32`` /
      ``logp64`` / ``floor_logp`` (over the finite rows); ``default_validation_raises``: whether the same batch raises
      ``ValueError`` in a ``BoxUniform`` built with the installed torch's default validation.
  sbi_priors   ``MG1Uniform(zeros(3), [10, 10, 1/3])`` (element-wise [64, 3]) and ``LotkaVolterraOscillating()`` ([64]) log_prob
      on 64 points each, some outside the support, validation off (with it on, the installed torch raises there:
      ``lv_default_validation_raises``).
These fixtures are not part of cases.CASES.
"""
import os

import numpy as np
import torch
from torch import nn

from make_golden import HERE, import_reference

ROWS = 257
BERNOULLI = {"d1": [1], "d3": [3], "d64": [64], "d65": [65], "d130": [130], "d784": [784], "s2x3x5": [2, 3, 5]}
IDENTITY, FRACTIONAL = "d65", "s2x3x5"
SAMPLES = {"c5s7": (5, 7, [784]), "c4s1": (4, 1, [2, 3, 5])}
BOX = [1, 3, 64, 130]


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1 << 20, path
    return size


def floor(a32, a64):
    return np.float64((a32.detach().double() - a64.detach()).abs().max().item())


def bernoulli_case(L, name, shape, gen):
    d = int(np.prod(shape))
    rows = 33 if d == 784 else ROWS
    torch.manual_seed(5000 + d)
    encoder = None if name == IDENTITY else nn.Linear(4, d)
    dist = L.distributions.ConditionalIndependentBernoulli(shape, encoder)
    if encoder is None:
        context = torch.randn(rows, d, generator=gen) * 25.0
    else:
        context = torch.randn(rows, 4, generator=gen) * 40.0
    x = torch.rand(rows, *shape, generator=gen)
    if name != FRACTIONAL:
        x = (x < 0.5).float()
    g = torch.randn(rows, generator=gen)
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in dist.state_dict().items()}
    out.update(context=context.numpy(), x=x.numpy(), g=g.numpy())

    def run(dtype):
        taps = []
        enc = None

        def tap(module, args, result):       # (returns None: the encoder's output stays what it is)
            if result.requires_grad:
                result.retain_grad()
                taps.append(result)

        if encoder is not None:
            enc = nn.Linear(4, d).to(dtype)
            enc.load_state_dict({k: v.to(dtype) for k, v in encoder.state_dict().items()})
            enc.register_forward_hook(tap)
        ref = L.distributions.ConditionalIndependentBernoulli(shape, enc)
        c = context.clone().to(dtype).requires_grad_(encoder is None)
        xs = x.clone().to(dtype).requires_grad_(True)
        logp = ref.log_prob(xs, context=c)
        (logp * g.to(dtype)).sum().backward()
        logits_grad = c.grad if encoder is None else taps[0].grad
        grads = {} if enc is None else {k: p.grad for k, p in enc.named_parameters()}
        with torch.no_grad():
            mean = ref.mean(c.detach())
            logits = ref._compute_params(c.detach())
        return logp.detach(), mean, logits, logits_grad.reshape(rows, *shape), xs.grad, grads

    logp32, mean32, logits32, gl32, gx32, gp32 = run(torch.float32)
    logp64, mean64, _, gl64, gx64, gp64 = run(torch.float64)
    assert (logits32 > 30).any() and (logits32 < -30).any() and (logits32.abs() < 1).any(), name
    for t in (logp32, logp64, gl64, gx64, mean64):
        assert torch.isfinite(t).all()
    out.update(logp32=logp32.numpy(), logp64=logp64.numpy(), floor_logp=floor(logp32, logp64),
               mean32=mean32.numpy(), mean64_minus_mean32=(mean64 - mean32.double()).float().numpy(),
               floor_mean=floor(mean32, mean64),
               grad_logits64=gl64.float().numpy(), floor_grad_logits=floor(gl32, gl64),
               grad_x64=gx64.float().numpy(), floor_grad_x=floor(gx32, gx64))
    for k in gp64:
        out["grad64::" + k] = gp64[k].numpy()
        out["floor_grad::" + k] = floor(gp32[k], gp64[k])
    size = save("bernoulli_" + name, out)
    print("bernoulli_%s floors logp %.2e (max|logp| %.1f) grad_logits %.2e grad_x %.2e mean %.2e | %d bytes"
          % (name, out["floor_logp"], float(logp64.abs().max()), out["floor_grad_logits"], out["floor_grad_x"],
             out["floor_mean"], size))


def sample_case(L, name, contexts, draws, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(contexts, *shape, generator=gen) * 3.0
    ref = L.distributions.ConditionalIndependentBernoulli(shape)
    while True:
        torch.manual_seed(seed)
        samples32 = ref._sample(draws, logits)
        torch.manual_seed(seed)
        noise = torch.rand(contexts * draws, *shape)
        rows32 = torch.sigmoid(logits).repeat_interleave(draws, dim=0)
        rows64 = torch.sigmoid(logits.double()).repeat_interleave(draws, dim=0)
        flat32 = samples32.reshape(contexts * draws, *shape)
        assert torch.equal(flat32, (noise < rows32).float())
        samples64 = (noise.double() < rows64).float()
        if torch.equal(flat32, samples64) and float((noise.double() - rows64).abs().min()) >= 1e-6:
            break
        seed += 1
    assert samples32.shape == (contexts, draws, *shape) and samples32.dtype == torch.float32
    size = save("bernoulli_sample_" + name, dict(logits=logits.numpy(), noise=noise.numpy(), samples32=samples32.numpy(),
                                                  samples64=samples64.reshape(samples32.shape).numpy(), seed=np.int64(seed),
                                                  num_samples=np.int64(draws)))
    print("bernoulli_sample_%s seed %d mean %.3f | %d bytes" % (name, seed, float(samples32.mean()), size))


def box_case(L, d, gen):
    BoxUniform = L.distributions.uniform.BoxUniform
    low = -1.0 - torch.rand(d, generator=gen)
    high = 1.0 + 2.0 * torch.rand(d, generator=gen)
    x = low + (high - low) * torch.rand(ROWS, d, generator=gen)
    outside = torch.rand(ROWS, generator=gen) < 1.0 / 3.0
    column = torch.randint(0, d, (ROWS,), generator=gen)
    above = torch.rand(ROWS, generator=gen) < 0.5
    for r in range(3, ROWS):
        if outside[r]:
            j = column[r]
            x[r, j] = high[j] + 0.25 if above[r] else low[j] - 0.25
    x[0] = low
    x[1, 0] = high[0]
    x[2, d - 1] = float("nan")
    default = torch.distributions.Distribution._validate_args
    torch.distributions.Distribution.set_default_validate_args(False)
    try:
        logp32 = BoxUniform(low, high).log_prob(x)
        logp64 = BoxUniform(low.double(), high.double()).log_prob(x.double())
    finally:
        torch.distributions.Distribution.set_default_validate_args(default)
    try:
        BoxUniform(low, high).log_prob(x)
        raises = False
    except ValueError:
        raises = True
    inf32, inf64 = torch.isinf(logp32), torch.isinf(logp64)
    assert torch.equal(inf32, inf64) and not inf32[0] and inf32[1] and inf32[2] and (logp32[inf32] < 0).all()
    assert not torch.isnan(logp32).any() and 0.2 < float(inf32.float().mean()) < 0.5
    size = save("box_d%d" % d, dict(low=low.numpy(), high=high.numpy(), x=x.numpy(), logp32=logp32.numpy(),
                                    logp64=logp64.numpy(), floor_logp=floor(logp32[~inf32], logp64[~inf64]),
                                    nan_row=np.int64(2), default_validation_raises=np.bool_(raises)))
    print("box_d%d outside %d of %d, log volume %.4f, default validation raises: %s | %d bytes"
          % (d, int(inf32.sum()), ROWS, -float(logp64[0]), raises, size))


def prior_cases(L, gen):
    MG1Uniform, LV = L.distributions.MG1Uniform, L.distributions.LotkaVolterraOscillating
    low, high = torch.zeros(3), torch.tensor([10.0, 10.0, 1.0 / 3.0])
    mg1_x = torch.rand(64, 3, generator=gen) * torch.tensor([12.0, 22.0, 0.4])
    lv_mean = torch.log(torch.tensor([0.01, 0.5, 1, 0.01]))
    lv_x = lv_mean + 1.5 * torch.randn(64, 4, generator=gen)
    try:
        LV().log_prob(lv_x)
        lv_raises = False
    except ValueError:
        lv_raises = True
    default = torch.distributions.Distribution._validate_args
    torch.distributions.Distribution.set_default_validate_args(False)
    try:
        mg1_32 = MG1Uniform(low, high).log_prob(mg1_x)
        # (the reference's MG1Uniform builds float32 matrices: its float64 value is the same expression on doubles)
        to_noise = torch.tensor([[1.0, -1, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
        mg1_64 = torch.distributions.Uniform(low.double(), high.double()).log_prob(mg1_x.double() @ to_noise)
        lv32 = LV().log_prob(lv_x)
        # LotkaVolterraOscillating builds float32 constants: its float64 value is the same expression on doubles
        gaussian = torch.distributions.MultivariateNormal(lv_mean.double(), covariance_matrix=0.25 * torch.eye(4).double())
        box = L.distributions.uniform.BoxUniform(-5 * torch.ones(4).double(), 2 * torch.ones(4).double())
        normalizer = -torch.log(torch.erf((2 - lv_mean.double()) / 0.5) - torch.erf((-5 - lv_mean.double()) / 0.5)).sum()
        lv64 = normalizer + gaussian.log_prob(lv_x.double()) + box.log_prob(lv_x.double())
    finally:
        torch.distributions.Distribution.set_default_validate_args(default)
    assert mg1_32.shape == (64, 3) and torch.equal(torch.isinf(mg1_32), torch.isinf(mg1_64))
    assert torch.equal(torch.isinf(lv32), torch.isinf(lv64))
    for t in (mg1_32, lv32):
        assert 0 < int(torch.isinf(t).sum()) < t.numel() and not torch.isnan(t).any()
    fm, fl = ~torch.isinf(mg1_32), ~torch.isinf(lv32)
    size = save("sbi_priors", dict(mg1_low=low.numpy(), mg1_high=high.numpy(), mg1_x=mg1_x.numpy(), mg1_logp32=mg1_32.numpy(),
                                   mg1_logp64=mg1_64.numpy(), mg1_floor=floor(mg1_32[fm], mg1_64[fm]), lv_x=lv_x.numpy(),
                                   lv_logp32=lv32.numpy(), lv_logp64=lv64.numpy(), lv_floor=floor(lv32[fl], lv64[fl]),
                                   lv_default_validation_raises=np.bool_(lv_raises)))
    print("sbi_priors mg1 outside %d of 192 floor %.2e | lv outside %d of 64 floor %.2e, default validation raises: %s | %d bytes"
          % (int((~fm).sum()), floor(mg1_32[fm], mg1_64[fm]), int((~fl).sum()), floor(lv32[fl], lv64[fl]), lv_raises, size))


def main():
    L = import_reference()
    import flowcon.distributions.uniform as uniform
    L.distributions.uniform = uniform
    seed = 900
    for name, shape in BERNOULLI.items():
        bernoulli_case(L, name, shape, torch.Generator().manual_seed(seed))
        seed += 1
    for name, (contexts, draws, shape) in SAMPLES.items():
        sample_case(L, name, contexts, draws, shape, seed)
        seed += 100
    for d in BOX:
        box_case(L, d, torch.Generator().manual_seed(seed))
        seed += 1
    prior_cases(L, torch.Generator().manual_seed(seed))


if __name__ == "__main__":
    main()

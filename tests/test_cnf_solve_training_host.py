"""A whole fixed-step CNF solve as one autograd node, host side: the reverse sweep the backward kernel runs against
autograd, the package's float64 solve against an independent Runge-Kutta loop, the option, the predicate, the CPU route
and the ABI.

Bounds: ``1e-12 max(1, max|expected|)`` for the sweep against autograd through the same loop (the same float64
operations, summed in another order: a few thousand roundings of values of order 10), ``1e-10 max(1, max|expected|)``
for the package's solver against the loop (the stage states are formed in another association)."""
import os
import re

import pytest
import torch

from flowconductor_amd import _hip, ops, options

import _cnf_solve_training_util as U

CASES = [(method, direction, mode) for method in U.METHODS for direction in ("forward", "backward")
         for mode in ("approximate", "brute_force")]


def _problem(method, direction, mode, seed=7):
    kind = {"euler": "concatsquash", "midpoint": "concat", "rk4": "squash"}[method]
    func = U.make_train_func(3, (6, 5), layer_type=kind, nonlinearity="softplus", mode=mode, seed=seed,
                             residual=method == "midpoint", scale_output=0.75 if method == "rk4" else 1).double()
    data = U.make_data(5, 3, seed=seed + 1)
    t0, t1 = (0.1, 0.9) if direction == "forward" else (0.9, 0.1)
    return func, data, t0, t1, {"euler": 3, "midpoint": 2, "rk4": 2}[method]


@pytest.mark.parametrize("method,direction,mode", CASES)
def test_reverse_sweep_is_autograd_through_the_loop(method, direction, mode):
    func, data, t0, t1, steps = _problem(method, direction, mode)
    e = data.e.double()
    z = data.y.double().requires_grad_(True)
    logp = data.c2.double().clone().requires_grad_(True)
    c1, c2 = data.c1.double(), torch.flip(data.c2.double(), [0])
    z_t, logp_t = U.rk_loop(func, z, logp, t0, t1, steps, method, e=e)
    params = list(func.parameters())
    expected = torch.autograd.grad((c1 * z_t).sum() + (c2 * logp_t).sum(), [z, logp] + params)
    g_z, g_logp, g_params = U.reverse_sweep(func, z, logp, t0, t1, steps, method, c1, c2, e=e)
    for got, want in zip([g_z, g_logp] + g_params, expected):
        assert float(want.abs().max()) > 0
        assert U.worst(got, want) <= 1e-12 * U.scale_of(want), (U.worst(got, want), U.scale_of(want))


@pytest.mark.parametrize("method,direction,mode", CASES)
def test_float64_solve_of_the_package_is_the_loop(method, direction, mode):
    func, data, t0, t1, steps = _problem(method, direction, mode, seed=11)
    e = data.e.double()
    cnf = U.make_cnf(func, solver=method, steps=steps, T=abs(t1 - t0))
    c1, c2 = data.c1.double(), data.c2.double()
    got, forward, backward, field = U.evaluate(cnf, data.y, data.c2, c1, c2, route=False, e=e, dtype=torch.float64,
                                               times=torch.tensor([t0, t1], dtype=torch.float64))
    assert (forward, backward, field) == (0, 0, 0)
    z = data.y.double().requires_grad_(True)
    logp = data.c2.double().clone().requires_grad_(True)
    z_t, logp_t = U.rk_loop(func, z, logp, t0, t1, steps, method, e=e)
    names = ["g::" + k for k, _ in cnf.named_parameters()]
    grads = torch.autograd.grad((c1 * z_t).sum() + (c2 * logp_t).sum(), [z, logp] + list(cnf.parameters()))
    want = dict(zip(["g::z", "g::logp"] + names, grads), z_t=z_t, logp_t=logp_t)
    assert set(want) == set(got)
    for key in want:
        assert U.worst(got[key], want[key]) <= 1e-10 * U.scale_of(want[key]), (key, U.worst(got[key], want[key]))


def test_option_choices_and_default():
    assert options.get("cnf_solve_training") is False
    for value in (False, True, "force"):
        with options.override(cnf_solve_training=value):
            assert options.get("cnf_solve_training") == value
    assert options.get("cnf_solve_training") is False
    for bad in ("on", 1, None):
        with pytest.raises(ValueError):
            with options.override(cnf_solve_training=bad):
                pass


def test_solve_train_fits_at_its_edges():
    fits = ops.cnf_solve_train_fits
    assert fits(65, 16, (64, 64, 64), 8, ops.CNF_RK4, True) and fits(65, 1, (), 1, ops.CNF_EULER, False)
    assert not fits(65, 3, (8, 8, 8, 8), 8, ops.CNF_RK4, True)         # four hidden layers
    assert not fits(65, 17, (8,), 8, ops.CNF_RK4, True)                # D = 17
    assert not fits(65, 3, (65,), 8, ops.CNF_RK4, True)                # width 65
    assert fits(65, 3, (64,), 8, ops.CNF_RK4, False)
    assert not fits(65, 3, (8,), 0, ops.CNF_RK4, False) and not fits(65, 3, (8,), 8, 3, False)
    # the tape: 4 bytes * steps * stages * N * D against the cap, nothing allocated
    assert ops.CNF_SOLVE_TRAIN_MAX_TAPE_BYTES == 1 << 30
    rows = ops.CNF_SOLVE_TRAIN_MAX_TAPE_BYTES // (4 * 8 * 4 * 16)
    for hutchinson in (False, True):
        assert fits(rows, 16, (8,), 8, ops.CNF_RK4, hutchinson) and not fits(rows + 1, 16, (8,), 8, ops.CNF_RK4, hutchinson)
    assert fits(4 * rows, 16, (8,), 8, ops.CNF_EULER, True) and not fits(4 * rows + 1, 16, (8,), 8, ops.CNF_EULER, True)
    assert fits(2 * rows, 16, (8,), 8, ops.CNF_MIDPOINT, True) and not fits(2 * rows, 16, (8,), 9, ops.CNF_MIDPOINT, True)


@pytest.mark.parametrize("mode", ["approximate", "brute_force"])
def test_cpu_route_is_the_composition(mode):
    func = U.make_train_func(3, (8, 8), mode=mode, seed=21)
    data = U.make_data(9, 3, seed=22)
    cnf = U.make_cnf(func, solver="rk4", steps=2)
    plain, _, _, _ = U.evaluate(cnf, data.y, data.c2, data.c1, data.c2, route=False, e=data.e)
    for route in (True, "force"):
        got, forward, backward, field = U.evaluate(cnf, data.y, data.c2, data.c1, data.c2, route=route, e=data.e)
        assert (forward, backward, field) == (0, 0, 0) and set(got) == set(plain)
        for key in plain:
            assert torch.equal(got[key], plain[key]), key


def _declared_arity(name):
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "flowcon_hip.h")
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    found = re.findall(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert len(found) == 1, name
    return len([piece for piece in found[0].split(",") if piece.strip()])


@pytest.mark.parametrize("name", ["fc_cnf_integrate_train", "fc_cnf_integrate_backward",
                                  "fc_cnf_integrate_backward_workspace"])
def test_header_declares_the_new_entries(name):
    assert name in _hip.SIGNATURES
    assert _declared_arity(name) == len(_hip.SIGNATURES[name])
    # the entry they generalise is declared as it was
    assert _declared_arity("fc_cnf_integrate") == len(_hip.SIGNATURES["fc_cnf_integrate"]) == 21


def test_abi_version_is_unchanged():
    assert _hip.ABI_VERSION == 3

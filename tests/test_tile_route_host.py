"""The launch decision of csrc/fc_tile.h, read through fc_tile_route (the host function launch_tile itself calls), on a
machine without a GPU: which of the two persistent prefetching kernels, the vector kernel and the scalar kernel each shape
of tests/test_gpu_tile_routes.py reaches."""
import ctypes
import os
import re

import pytest

import _tile_util as U
from flowconductor_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# parameters per dim of the entries that take `cols` (affine, rq, linear, quadratic with / without tails, cubic) ...
COLS_M = (2, 23, 31, 8, 15, 17, 18, 32)
# ... and of the sum of sigmoids with 6 / 8 sigmoids
SOS_M = (19, 25)
ALL_M = COLS_M + SOS_M


def _route(n, d, d_t, m, **kw):
    code, r = U.route(n, d, d_t, d_t * m, **kw)
    assert code == 0
    return r


def test_declaration_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "flowcon_hip.h")).read()
    decl = re.search(r"\bint\s+fc_tile_route\s*\(([^)]*)\)", text)
    assert decl and "fc_tile_route" in _hip.SIGNATURES
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES["fc_tile_route"])


def test_multipliers_are_the_entries_own():
    for name, cfg in U.CONFIGS.items():
        assert cfg.m == U.facade_multiplier(cfg), name
    assert sorted(cfg.m for cfg in U.CONFIGS.values()) == sorted(ALL_M)


@pytest.mark.parametrize("m", ALL_M)
def test_shape_a_aligned(m):
    """517 x 64, 32 transformed: 64 full tiles of 8 rows, then 5 leftover rows on the vector kernel.  A tile holds
    8 * 32 * m / 4 = 64 m parameter float4: over the 6 x 256 of the <6, 1> instance from m = 25 (1600)."""
    want = U.PF82 if m in (25, 31, 32) else U.PF61
    assert _route(517, 64, 32, m) == U.Route(want, 8, 64, 5, U.VECTOR, 5, 1, 192)


@pytest.mark.parametrize("m", ALL_M)
def test_shape_a_misaligned_and_shared(m):
    assert _route(517, 64, 32, m, aligned=False) == U.Route(U.NO_PF, 0, 0, 0, U.SCALAR, 8, 65, 256)
    assert _route(517, 64, 32, m, shared=True) == U.Route(U.NO_PF, 0, 0, 0, U.VECTOR, 8, 65, 256)


@pytest.mark.parametrize("m", ALL_M)
def test_shape_b(m):
    """1031 x 96, 16 transformed: 16 rows x 96 floats are 384 input float4 per tile, over the 256 of <6, 1> for every m."""
    assert _route(1031, 96, 16, m) == U.Route(U.PF82, 16, 64, 7, U.VECTOR, 7, 1, 128)


@pytest.mark.parametrize("m", ALL_M)
def test_shapes_without_a_persistent_launch(m):
    assert _route(100, 130, 65, m) == U.Route(U.NO_PF, 0, 0, 0, U.SCALAR, 3, 34, 256)      # C: 3 x 130 % 4 != 0
    assert _route(3, 6, 3, m) == U.Route(U.NO_PF, 0, 0, 0, U.SCALAR, 3, 1, 64)             # G: N < 4
    assert _route(257, 8, 4, m) == U.Route(U.NO_PF, 0, 0, 0, U.VECTOR, 64, 5, 256)         # H: 4 full tiles


@pytest.mark.parametrize("m", ALL_M)
def test_shape_d_not_a_power_of_two(m):
    want = U.PF82 if m in (31, 32) else U.PF61
    assert _route(259, 60, 60, m) == U.Route(want, 4, 64, 3, U.VECTOR, 3, 1, 192)


def test_sum_of_sigmoids_shapes():
    assert _route(517, 32, 32, 19) == U.Route(U.PF61, 8, 64, 5, U.VECTOR, 5, 1, 192)
    assert _route(517, 32, 32, 25) == U.Route(U.PF82, 8, 64, 5, U.VECTOR, 5, 1, 192)
    assert _route(1031, 16, 16, 19) == U.Route(U.PF61, 16, 64, 7, U.VECTOR, 7, 1, 128)
    assert _route(1031, 16, 16, 25) == U.Route(U.PF82, 16, 64, 7, U.VECTOR, 7, 1, 128)
    for m in SOS_M:
        assert _route(259, 60, 60, m).pf == U.PF61
        assert _route(100, 130, 130, m) == U.Route(U.NO_PF, 0, 0, 0, U.SCALAR, 1, 100, 192)
        assert _route(3, 3, 3, m) == U.Route(U.NO_PF, 0, 0, 0, U.SCALAR, 3, 1, 64)
        assert _route(257, 4, 4, m) == U.Route(U.NO_PF, 0, 0, 0, U.VECTOR, 64, 5, 256)


def test_the_table_the_gpu_tests_assert():
    for name, cfg in U.CONFIGS.items():
        for shape in U.SHAPES:
            n, d, d_t = U.dims(cfg, shape)
            assert _route(n, d, d_t, cfg.m) == U.expected_route(cfg, shape), (name, shape)
            r = U.DISTINCT[shape]
            if U.expected_route(cfg, shape).pf:
                # the distinct rows on their own stay on the vector kernel, and repeat inside the persistent launch
                alone = _route(r, d, d_t, cfg.m)
                assert alone.pf == U.NO_PF and alone.kernel == U.VECTOR and r < 64 * alone.s, (name, shape)


def test_empty_batch_and_refused_shapes():
    assert U.route(0, 64, 32, 64) == (0, U.Route(0, 0, 0, 0, 0, 0, 0, 0))
    lib = _hip.load()
    out = (ctypes.c_int64 * 8)()
    assert lib.fc_tile_route(-1, 64, 32, 64, 0, 1, out) != 0
    assert lib.fc_tile_route(8, 16, 32, 64, 0, 1, out) != 0           # d_t > d
    assert lib.fc_tile_route(8, 64, 32, 64, 0, 1, None) != 0
    # one row beyond the 150 KiB LDS plan: what launch_tile returns before launching
    code, r = U.route(8, 4, 4, 4 * 9601)
    assert code != 0 and r.pf == U.NO_PF and r.kernel == U.NO_KERNEL


def test_invariants_over_a_sweep():
    """Never a persistent launch together with shared parameters or misaligned pointers; leftover rows < S; the two
    launches cover the batch exactly."""
    for d, d_t in ((64, 32), (96, 16), (60, 60), (130, 65), (8, 4), (6, 3), (1, 1), (256, 256), (300, 7)):
        for m in (1, 2, 8, 19, 25, 32, 97):
            for n in (1, 3, 4, 63, 64, 255, 256, 257, 517, 1031, 4096, 100003):
                for shared in (False, True):
                    for aligned in (False, True):
                        code, r = U.route(n, d, d_t, d_t * m, shared, aligned)
                        assert code == 0, (n, d, d_t, m)
                        what = (n, d, d_t, m, shared, aligned, r)
                        if shared or not aligned:
                            assert r.pf == U.NO_PF, what
                        if r.pf:
                            assert r.pf_tiles >= 64 and r.left_rows < r.pf_s, what
                            assert r.pf_s * r.pf_tiles + r.left_rows == n, what
                            assert (r.kernel == U.NO_KERNEL) == (r.left_rows == 0), what
                            if r.left_rows:     # (several tiles where the persistent launch had grown its S)
                                assert (r.grid - 1) * r.s < r.left_rows <= r.grid * r.s, what
                        else:
                            assert r.left_rows == 0 and r.kernel != U.NO_KERNEL, what
                            assert (r.grid - 1) * r.s < n <= r.grid * r.s, what
                        if r.kernel:
                            assert 64 <= r.block <= 256 and r.block % 64 == 0, what
                        if not aligned:
                            assert r.kernel in (U.NO_KERNEL, U.SCALAR), what

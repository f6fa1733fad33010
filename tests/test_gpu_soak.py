"""A short seeded run of tests/soak_vs_oracle.py: random grids, lattices, noise, plateaus, vacuum and refinement modes through
the one-GPU pipeline against the CPU oracle -- assignment map, basin order, refinement log and refined map."""
import pytest

from soak_vs_oracle import run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('method,odd,seed', [('neargrid', False, 101), ('neargrid', True, 102), ('ongrid', False, 103), ('ongrid', True, 104)])
def test_random_cases_equal_the_oracle(method, odd, seed):
    failures = run(25, seed, method, odd)
    assert not failures, '\n'.join(failures)


def test_random_grids_the_brick_lattice_does_not_divide():
    """round 4: grids of 41..149 voxels per axis, any remainder modulo 8 (also 1: the bricks one voxel wide that are never
    certified) -- the brick pipeline with cut bricks against the oracle"""
    failures = run(8, 105, 'neargrid', oddbig=True)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('method,seed', [('neargrid', 106), ('ongrid', 107)])
def test_random_tiny_grids_equal_the_oracle(method, seed):
    """every axis from 3 to 9 voxels: grids below one 8^3 brick, where none of the brick routes applies and the stencils'
    planes x-2 and x+1 (or x+2) can be one plane"""
    failures = run(40, seed, method, tiny=True)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('method,seed', [('neargrid', 108), ('ongrid', 109)])
def test_random_thin_grids_equal_the_oracle(method, seed):
    """one axis from 3 to 9 voxels beside two of 16, 24, 40, 80 or 96: a short axis on both sides of the `>= 16` and
    `nz < 80` route tests"""
    failures = run(12, seed, method, thin=True)
    assert not failures, '\n'.join(failures)


FIXED_SMALL = [(3, 3, 3), (3, 4, 5), (4, 9, 3), (8, 8, 8), (9, 3, 8), (3, 16, 40)]


@pytest.mark.parametrize('method,seed', [('neargrid', 110), ('ongrid', 111)])
def test_fixed_small_grids_equal_the_oracle(method, seed):
    """the smallest grid xb_set_grid accepts, axes of 3 and 4 in every position, exactly one brick, and a thin slab of
    bricks -- named rather than left to the draw"""
    failures = run(len(FIXED_SMALL), seed, method, shapes=FIXED_SMALL)
    assert not failures, '\n'.join(failures)


# ---- magnitude and sign (soak_vs_oracle.MAGNITUDE_CASES; tests/test_magnitude_cpu.py shows on the CPU that each input reaches the
# predicate it is for).  Wall time on an MI355X box: 1.8 s for these 17 tests, the oracle included (the slowest, four grids, 0.3 s).
from soak_vs_oracle import MAGNITUDE_CASES, directed_vacuum_case, oracle_expectation, run_magnitude  # noqa: E402


@pytest.mark.parametrize('name', list(MAGNITUDE_CASES))
def test_extreme_magnitudes_and_signs_equal_the_oracle(name):
    """the four named grids (smallest fused grid, cut bricks, whole bricks with regions, whole sweep tiles) with the density scaled
    by 2^-40 / 2^-44 / 2^-48 (max_grad straddles the 1E-14 of the stay test: gradient and ongrid steps mix under the brick masks),
    2^-140 (every brick potential a subnormal float, without and with a tolerance), 2^130 (potentials beyond FLT_MAX) or shifted
    by -4 (negative densities, a negative tolerance): basins, maxima, assignment, refinement log and refined map == the oracle's"""
    failures = run_magnitude(name)
    assert not failures, '\n'.join(failures)


def test_a_brick_maximum_that_float_rounds_below_the_tolerance_is_walked():
    """ADVICE r6, third finding (brick_is_vacuum): at 2^-140 a brick's maximum m becomes a subnormal float below m; with the
    tolerance between float32(m) * (1 + 1e-6) and m the brick holds voxels above the tolerance, and the relative margin alone would
    keep it off the walk list.  The map, the maxima and a refinement equal the oracle's; the brick is not marked record-less."""
    import numpy as np
    from pybader_amd import _lib
    rho, dm, tg, tol, brick, m = directed_vacuum_case()
    ctx = _lib.Context(0)
    try:
        ctx.set_grid(rho.shape, dm, tg)
        ctx.upload_density(rho)
        ctx.vacuum_assign(tol, 1.0)
        n = ctx.assign('neargrid')
        got0 = ctx.download_labels(np.int64)
        gmax = np.ravel_multi_index(tuple(ctx.maxima().T), rho.shape)
        blab = ctx.brick_labels()
        log = ctx.refine('all', -1)
        got = ctx.download_labels(np.int32)
    finally:
        ctx.close()
    maxima, lab, olog, v = oracle_expectation(rho, tol, 'neargrid', 'all', -1, dm, tg)
    assert blab[brick] != np.iinfo(np.int32).min, 'XB_NOREC: the brick was taken for vacuum'
    assert n == len(maxima) and np.array_equal(gmax, maxima)
    assert np.array_equal(got0, lab)
    assert [tuple(x) for x in log] == [tuple(x) for x in olog] and np.array_equal(got, v)

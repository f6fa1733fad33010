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

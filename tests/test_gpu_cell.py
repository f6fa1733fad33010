"""The four atom-centred analyses on ONE grid whose tiles are clipped on every axis (-m gpu): shape (9, 10, 17), 2 x 2 x 3 tiles of
which the last of every axis holds 1, 2 and 1 voxels, the triclinic cell, three atoms (tests/test_cell_cpu.py builds the input and
says what the CPU knows of it).  The moments, the Voronoi labels, the Hirshfeld field and sums and one ISA iteration share the cell
and tile geometry of csrc/k_cell.h; here each equals its numpy restatement with ==, and the tile kernels' two routes agree.

Two of the results are sums of float atomics in any order.  They are made exact, so that == holds whatever the order:
  the moments   every voxel carries its own label, so a label's sum is its one voxel's terms (what is summed is bit-defined);
  the Hirshfeld sums   the narrow pro-atoms' spheres are disjoint and the density holds multiples of 2^-10: every weight is 1.0 and
                every partial sum of rho is exact (test_cell_cpu.py asserts both)."""
import functools
import math

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib
from test_cell_cpu import KNOTS, LATTICE, SHAPE, SHELLS, case
import test_hirshfeld_cpu as hs
import test_isa_cpu as isa
import test_multipole_cpu as ms
import test_voronoi_cpu as vo

pytestmark = pytest.mark.gpu
PRO, DEF = _lib.XB_HIRSHFELD_PROMOLECULE, _lib.XB_HIRSHFELD_DEFORMATION
VV = hs.VV
TILES = 12


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    c.set_grid(SHAPE, np.zeros(27), np.zeros(9))
    c.upload_density(case().rho)
    yield c
    c.close()


def same_bits(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    diff = got.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ from the restatement, first at {np.flatnonzero(diff)[0]}'


@functools.lru_cache(maxsize=None)
def voronoi_labels():
    lab = vo.reference_labels(SHAPE, LATTICE, case().atoms)
    lab.flags.writeable = False
    return lab


def test_voronoi_labels(ctx):
    c = case()
    stats = ctx.voronoi_assign(LATTICE, c.atoms)
    got = ctx.download_labels(np.int32)
    assert stats['candidate_tiles'] == TILES and stats['full_tiles'] == 0 and 0 < stats['max_candidates'] <= 81, stats
    forced = ctx.voronoi_assign(LATTICE, c.atoms, full_search=True)
    full = ctx.download_labels(np.int32)
    assert forced == {'candidate_tiles': 0, 'full_tiles': TILES, 'max_candidates': 0}
    assert np.array_equal(got, voronoi_labels()) and np.array_equal(full, got)
    assert set(np.unique(got)) == {0, 1, 2}


def test_hirshfeld_field_of_overlapping_pro_atoms(ctx):
    c = case()
    P, _ = hs.restate(SHAPE, LATTICE, c.atoms, c.species, c.wide)
    kept = hs.candidate_counts(SHAPE, LATTICE, c.atoms, c.species, c.wide)
    ctx.hirshfeld_setup(LATTICE, c.atoms, c.species, c.wide.tables, c.wide.r_cut)
    rho = c.rho.reshape(-1)
    for full in (False, True):
        same_bits(ctx.hirshfeld_field(PRO, full), P, f'P (full {full})')
        same_bits(ctx.hirshfeld_field(DEF, full), rho - P, f'rho - P (full {full})')
    stats = ctx.hirshfeld_sum(VV)[3]
    assert stats == {'candidate_tiles': TILES, 'full_tiles': 0, 'max_candidates': int(kept.max())}


def test_hirshfeld_sums_that_are_exact(ctx):
    c = case()
    s = hs.restated_sums(c.rho, *hs.restate(SHAPE, LATTICE, c.atoms, c.species, c.narrow))
    kept = hs.candidate_counts(SHAPE, LATTICE, c.atoms, c.species, c.narrow)
    ctx.hirshfeld_setup(LATTICE, c.atoms, c.species, c.narrow.tables, c.narrow.r_cut)
    for full in (False, True):
        charge, volume, rest, stats = ctx.hirshfeld_sum(VV, full)
        same_bits(charge, s['charge'] * VV, f'the charges (full {full})')
        same_bits(volume, s['volume'] * VV, f'the volumes (full {full})')
        same_bits(rest, np.array([s['rest'][0] * VV, s['rest'][1] * VV]), f'the rest (full {full})')
        want = dict(candidate_tiles=0, full_tiles=TILES, max_candidates=0) if full else dict(candidate_tiles=TILES, full_tiles=0, max_candidates=int(kept.max()))
        assert stats == want
    assert (s['volume'] > 0).all() and s['rest'][1] > 0
    same_bits(ctx.hirshfeld_field(PRO), hs.restate(SHAPE, LATTICE, c.atoms, c.species, c.narrow)[0], 'P of the narrow pro-atoms')


def test_one_isa_iteration(ctx):
    c = case()
    g = isa.geometry(SHAPE, LATTICE, c.atoms, c.r_cut, SHELLS)
    bound = float(np.abs(c.rho).max())
    e = isa.exponent(bound, g.count.max())
    want, _ = isa.run(g, c.rho, e, 1)
    rows = {}
    for route, kw in (('windows', {}), ('direct', {'direct': True}), ('full_search', {'full_search': True})):
        info = ctx.isa_setup(LATTICE, c.atoms, c.r_cut, SHELLS, bound)
        assert info['e'] == e and np.array_equal(ctx.isa_tables()[1], g.count), route
        rows[route], stats = ctx.isa_iterate(1, **kw)
        assert stats['beyond_bound'] == 0 and stats['candidate_tiles'] + stats['full_tiles'] == TILES, route
        assert stats['full_tiles'] == (TILES if route == 'full_search' else 0), route
        assert np.array_equal(rows[route], want), route
    assert np.array_equal(rows['windows'], rows['full_search']) and np.array_equal(rows['windows'], rows['direct'])
    ctx.hirshfeld_release()


def test_moments_of_one_voxel_labels(ctx):
    c = case()
    N = int(np.prod(SHAPE))
    own = voronoi_labels().reshape(-1)
    # the global route: every voxel its own label, about the atom the voxel belongs to
    every = np.arange(N, dtype=np.int32)
    # the LDS route: MS_BINS voxels spread over the grid carry a label, the others none
    few = np.full(N, -1, np.int32)
    at = (np.arange(ms.MS_BINS) * (N // ms.MS_BINS)).astype(np.int64)
    few[at] = np.arange(ms.MS_BINS, dtype=np.int32)
    for what, lab, voxels in (('global', every, np.arange(N)), ('LDS', few, at)):
        cen = np.ascontiguousarray(c.atoms[own[voxels]])
        terms, _, label = ms.reference_terms(c.rho, lab.reshape(SHAPE), LATTICE, cen)
        assert np.array_equal(label[voxels], np.arange(voxels.size))
        ctx.upload_labels(lab.reshape(SHAPE))
        got, volume = ctx.moment_sum(LATTICE, cen, VV)
        same_bits(got, (0.0 + terms[voxels]) * VV, f'the moments ({what} route)')     # (a sum begins at +0.0: a term -0.0 gives +0.0)
        same_bits(volume, np.full(voxels.size, 1.0 * VV), f'the volumes ({what} route)')

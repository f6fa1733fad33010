"""The host arithmetic the atom-centred analyses share (pybader_amd/csrc/host_cell.h), compiled alone for the host with g++ behind a
short extern "C" shim: the 27 image vectors, the cell's length and the tiles per axis against numpy, float64 bit for bit.

Below them: the one input of tests/test_gpu_cell.py, on which the moments, the Voronoi partition, the Hirshfeld weights and ISA meet
the same clipped tiles, and what the CPU can say about it beforehand."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from pybader_amd import _lib, synth
from pybader_amd.hirshfeld import ProAtoms
import test_hirshfeld_cpu as hs
import test_voronoi_cpu as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'pybader_amd', 'csrc', 'host_cell.h')

SHIM = '#include "host_cell.h"\n' + r'''
extern "C" double shift(const double *lat, int x, int y, int z, int j) { return cell_shift(lat, x, y, z, j); }
extern "C" void images27(const double *lat, double *out) { cell_images27(lat, reinterpret_cast<double(*)[3]>(out)); }
extern "C" double len(const double *lat) { return cell_len(lat); }
extern "C" int tiles(int n, int T) { return cell_tiles(n, T); }
'''

# entries from 1e-3 to 1e3, mixed signs: every product and sum of the expressions rounds
WIDE = np.array([[1.0e3, -3.0e-3, 0.7], [-41.3, 2.0e-3, 913.0], [0.05, -77.7, -1.0e-3]])
LATTICES = {'cubic': synth.CUBIC6, 'tric': synth.TRICLINIC, 'wide': WIDE}
_pdbl = C.POINTER(C.c_double)


@pytest.fixture(scope='module')
def cell(tmp_path_factory):
    gxx = shutil.which('g++') or shutil.which('c++')
    if gxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('host_cell')
    src = d / 'shim.cpp'
    src.write_text(SHIM)
    so = d / 'host_cell.so'
    # (-ffp-contract=off as the library's build: the expressions are separate multiplies and adds)
    subprocess.check_call([gxx, '-O1', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', '-shared', '-fPIC', '-I', os.path.dirname(HEADER),
                           '-o', str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.shift.restype = lib.len.restype = C.c_double
    lib.shift.argtypes = [_pdbl, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.images27.argtypes = [_pdbl, _pdbl]
    lib.len.argtypes = [_pdbl]
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize('lname', list(LATTICES))
def test_the_27_image_vectors_equal_numpys_in_the_stated_order(cell, lname):
    lat = np.ascontiguousarray(LATTICES[lname], dtype=np.float64)
    got = np.zeros((27, 3))
    cell.images27(lat.ctypes.data_as(_pdbl), got.ctypes.data_as(_pdbl))
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                i = (x + 1) * 9 + (y + 1) * 3 + (z + 1)
                want = (lat[0] * np.float64(x) + lat[1] * np.float64(y)) + lat[2] * np.float64(z)
                assert np.array_equal(bits(got[i]), bits(want)), (lname, x, y, z)
                one = [cell.shift(lat.ctypes.data_as(_pdbl), x, y, z, j) for j in range(3)]
                assert np.array_equal(bits(one), bits(want)), (lname, x, y, z)
    # a shift beyond the 27, as the Hirshfeld image list has them
    want = (lat[0] * np.float64(-3) + lat[1] * np.float64(2)) + lat[2] * np.float64(5)
    assert np.array_equal(bits([cell.shift(lat.ctypes.data_as(_pdbl), -3, 2, 5, j) for j in range(3)]), bits(want))


@pytest.mark.parametrize('lname', list(LATTICES))
def test_the_length_is_the_sum_of_the_three_norms_in_that_order(cell, lname):
    lat = np.ascontiguousarray(LATTICES[lname], dtype=np.float64)
    want = np.float64(0.0)
    for a in lat:
        want = want + np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    assert np.array_equal(bits(cell.len(lat.ctypes.data_as(_pdbl))), bits(want))


def test_tiles_per_axis(cell):
    assert [cell.tiles(n, 8) for n in (1, 7, 8, 9, 64, 65)] == [1, 1, 1, 2, 8, 9]


def test_the_arithmetic_part_needs_the_standard_headers_only():
    src = open(HEADER).read()
    plain = src[:src.index('#ifdef __HIPCC__')]
    assert [l.split()[1] for l in plain.splitlines() if l.startswith('#include')] == ['<cmath>', '<cstdint>']
    assert '#include' not in src[src.index('#ifdef __HIPCC__'):]


# ---- the input of tests/test_gpu_cell.py ----------------------------------------------------------------------------------------
# 2 x 2 x 3 tiles of 8^3, the last of every axis clipped: to 1, 2 and 1 voxels
SHAPE = (9, 10, 17)
LATTICE = synth.TRICLINIC
ATOMS_FRAC = np.array([[0.12, 0.18, 0.10], [0.58, 0.47, 0.52], [0.31, 0.83, 0.88]])
R_WIDE, R_NARROW, KNOTS, SHELLS = 3.0, 1.0, 64, 16


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case():
    """built once, never written.  rho holds multiples of 2^-10 below 2^7: any sum of its 1530 values is exact in float64, in any
    order.  `narrow`: pro-atoms whose spheres (of all images) are disjoint, so that every voxel has at most one term, its weight
    is p / P = 1.0 exactly, and the sums of xb_hirshfeld_sum -- float atomics in any order -- are exact sums of rho and of ones."""
    c = Case()
    c.shape, c.lattice = SHAPE, LATTICE
    c.atoms = np.ascontiguousarray(ATOMS_FRAC @ LATTICE)
    c.species = np.zeros(3, np.int32)
    c.rho = synth.rough_density(SHAPE, LATTICE, quantum=2.0 ** -10)
    c.wide, c.narrow = hs.bump_proatoms(R_WIDE, KNOTS), hs.bump_proatoms(R_NARROW, KNOTS)
    c.r_cut = np.full(3, R_WIDE)
    for a in (c.atoms, c.species, c.rho, c.r_cut):
        a.flags.writeable = False
    return c


def test_the_input_clips_tiles_on_every_axis_and_a_tile_keeps_fewer_images_than_the_list():
    c = case()
    assert [s % 8 for s in SHAPE] == [1, 2, 1] and hs.n_tiles(SHAPE) == 12
    counts = vo.candidate_counts(SHAPE, LATTICE, c.atoms)
    assert counts.shape == (12,) and counts.min() < 27 * 3 and counts.max() <= _lib.XB_VORONOI_CAND_MAX
    for pro in (c.wide, c.narrow):
        whole = hs.image_list(LATTICE, c.atoms, c.species, pro.r_cut).shape[0]
        counts = hs.candidate_counts(SHAPE, LATTICE, c.atoms, c.species, pro)
        assert counts.shape == (12,) and counts.min() < whole and 0 < counts.max() <= _lib.XB_HIRSHFELD_CAND_MAX, (whole, counts)
    assert counts.min() == 0                                                        # (a tile no narrow pro-atom reaches)


def test_the_exact_sums_of_the_narrow_pro_atoms_are_what_the_docstring_says():
    c = case()
    q = c.rho * 2.0 ** 10
    assert np.array_equal(q, np.rint(q)) and np.abs(c.rho).max() < 2.0 ** 7 and c.rho.size < 2 ** 11      # 10 + 7 + 11 < 53 bits
    P, p = hs.restate(SHAPE, LATTICE, c.atoms, c.species, c.narrow)
    assert ((p > 0).sum(axis=0) <= 1).all() and np.array_equal(p.sum(axis=0), P)
    assert all((p[a] > 0).any() for a in range(3)) and (P == 0).any()
    P, p = hs.restate(SHAPE, LATTICE, c.atoms, c.species, c.wide)
    assert ((p > 0).sum(axis=0) > 1).any()                                          # the wide ones overlap

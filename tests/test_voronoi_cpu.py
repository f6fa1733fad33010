"""The host side of the Voronoi partition (pybader_amd/voronoi.py, xb_voronoi_assign) and the plain numpy restatement of the
definition in include/bader_hip.h / DESIGN.md section 16 that tests/test_gpu_voronoi.py compares the kernel with, map by map
with ==.

`reference_labels` is elementwise IEEE float64 in the order the definition writes, so every d2 carries the bits the device
forms; the label is the lexicographic minimum of (d2, atom).  `candidate_counts` restates phase 1 of csrc/k_voronoi.h (which
images a tile keeps): the GPU tests assert from the call's statistics which route the tiles took, and the checks here say,
without a GPU, that the inputs they use do reach those routes."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, voronoi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8
ORTHO = np.diag([6.0, 5.0, 4.0])
TRIC = np.array([[5.0, 0.0, 0.0], [1.2, 3.1, 0.0], [0.7, -0.9, 2.2]])
LATTICES = {'ortho': ORTHO, 'tric': TRIC}
IMAGES = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def _positions(shape, lat):
    nx, ny, nz = shape
    p0, p1, p2 = (a.reshape(-1).astype(np.float64) for a in np.indices(shape))
    pc = []
    for j in range(3):
        c = lat[j] * p0 / np.float64(nx)
        c = c + lat[3 + j] * p1 / np.float64(ny)
        c = c + lat[6 + j] * p2 / np.float64(nz)
        pc.append(c)
    return pc


def _image_vectors(lat):
    return [[(lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z) for j in range(3)] for x, y, z in IMAGES]


def reference_labels(shape, lattice, atoms):
    """The definition in plain numpy -> int32 labels of `shape`: per atom D(a) = the minimum of d2 over the 27 images, the label
    the atom with the smallest D(a), a tie to the smaller index (a later atom takes a voxel only with a strictly smaller D)."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(9)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    pc, pbc = _positions(shape, lat), _image_vectors(lat)
    best = np.full(pc[0].size, np.inf)
    label = np.full(pc[0].size, np.iinfo(np.int32).max, dtype=np.int32)
    for a, at in enumerate(atoms):
        da = np.full(pc[0].size, np.inf)
        for v in pbc:
            e = [pc[j] - (at[j] + v[j]) for j in range(3)]
            da = np.minimum(da, (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        take = (da < best) | ((da == best) & (a < label))
        best = np.where(take, da, best)
        label = np.where(take, np.int32(a), label)
    return label.reshape(shape)


def scalar_labels(shape, lattice, atoms):
    """the same, one voxel, atom and image at a time in Python floats (IEEE float64), images and atoms in the reverse order:
    a lexicographic minimum does not care"""
    lat = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = [[float(x) for x in at] for at in np.asarray(atoms, dtype=np.float64).reshape(-1, 3)]
    nx, ny, nz = shape
    out = np.zeros(shape, np.int32)
    for p0 in range(nx):
        for p1 in range(ny):
            for p2 in range(nz):
                pc = []
                for j in range(3):
                    c = lat[j] * p0 / nx
                    c += lat[3 + j] * p1 / ny
                    c += lat[6 + j] * p2 / nz
                    pc.append(c)
                best = (float('inf'), len(atoms))
                for a in reversed(range(len(atoms))):
                    for x, y, z in reversed(IMAGES):
                        e = [pc[j] - (atoms[a][j] + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                        best = min(best, ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], a))
                out[p0, p1, p2] = best[1]
    return out


def candidate_counts(shape, lattice, atoms):
    """phase 1 of csrc/k_voronoi.h restated: per 8^3 tile (C order over the tiles) the number of images it keeps -- those within
    d_min + 2 R + slack of the centre of the tile's voxels, R half the longest body diagonal of the box they span"""
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    q = (atoms[:, None, :] + np.array(_image_vectors(lat.reshape(9)), dtype=np.float64)[None, :, :]).reshape(-1, 3)
    length = np.sqrt((lat * lat).sum(axis=1)).sum()
    n = np.array(shape, dtype=np.float64)
    out = []
    for x0 in range(0, shape[0], TILE):
        for y0 in range(0, shape[1], TILE):
            for z0 in range(0, shape[2], TILE):
                lo = np.array([x0, y0, z0])
                ext = np.minimum(TILE, np.array(shape) - lo) - 1.0
                c = ((lo + 0.5 * ext) / n) @ lat
                u = (ext / n)[:, None] * lat
                two_r = max(np.linalg.norm(u[0] + s1 * u[1] + s2 * u[2]) for s1 in (1, -1) for s2 in (1, -1))
                d2 = ((c - q) ** 2).sum(axis=1)
                lim = np.sqrt(d2.min()) + two_r
                lim += 2.0 ** -40 * (lim + length)
                out.append(int((d2 <= lim * lim * (1 + 2.0 ** -40)).sum()))
    return np.array(out)


# ---- inputs (shared with tests/test_gpu_voronoi.py) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_atoms(lname, n, seed=5):
    """n atoms inside the cell, a few of them shifted out of it by a lattice vector (atoms are searched as given, not wrapped)"""
    rng = np.random.default_rng(seed + n)
    frac = rng.random((n, 3))
    if n >= 8:
        frac[1] += (1, 0, 0)
        frac[n // 2] -= (0, 1, 1)
    a = np.ascontiguousarray(frac @ LATTICES[lname])
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def reference(shape, lname, n):
    """reference_labels of one input of the GPU tests, computed once and never written"""
    lab = reference_labels(shape, LATTICES[lname], random_atoms(lname, n))
    lab.flags.writeable = False
    return lab


CANDIDATE_CASES = [((48, 40, 32), 'ortho', 8), ((40, 24, 16), 'tric', 8), ((40, 24, 16), 'tric', 60)]
OVERFLOW_CASE = ((5, 7, 11), 'tric', _lib.XB_VORONOI_CAND_MAX // 16)
MIXED_SHAPE, MIXED_N = (20, 9, 33), 200
THIN_CASE = ((1, 9, 17), 'tric', 8)

TIE_SHAPE, TIE_LATTICE = (16, 16, 16), np.eye(3) * 2.0
TIE_ATOMS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
TIE_COUNTS = [1176, 951, 890, 1079, 0]


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', list(LATTICES))
def test_reference_labels_against_a_scalar_triple_loop(lname):
    shape = (3, 4, 5)
    atoms = random_atoms(lname, 8)
    want = scalar_labels(shape, LATTICES[lname], atoms)
    got = reference_labels(shape, LATTICES[lname], atoms)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert len(set(want.reshape(-1))) >= 4


def test_ties_go_to_the_smaller_atom_index():
    """a cubic cell of edge 2 with 16^3 voxels: h = 2^-3, every position and every d2 is exact, and the atoms sit on voxels, so
    voxels halfway between two of them tie exactly -- thousands do.  The duplicate fifth atom never wins one."""
    lab = reference_labels(TIE_SHAPE, TIE_LATTICE, TIE_ATOMS)
    assert np.bincount(lab.reshape(-1), minlength=5).tolist() == TIE_COUNTS
    assert np.array_equal(lab, scalar_labels(TIE_SHAPE, TIE_LATTICE, TIE_ATOMS))
    # how many voxels tie: those where the best two atoms are equally far -- of all five (the duplicate ties wherever the fourth
    # atom wins), and of the first four alone
    lat = TIE_LATTICE.reshape(9)
    pc, pbc = _positions(TIE_SHAPE, lat), _image_vectors(lat)
    dist = []
    for at in TIE_ATOMS:
        da = np.full(pc[0].size, np.inf)
        for v in pbc:
            e = [pc[j] - (at[j] + v[j]) for j in range(3)]
            da = np.minimum(da, (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        dist.append(da)
    all_five = np.sort(np.array(dist), axis=0)[:2]
    two = np.sort(np.array(dist[:4]), axis=0)[:2]
    print('tied voxels:', int((all_five[0] == all_five[1]).sum()), 'of them without the duplicate:', int((two[0] == two[1]).sum()))
    assert (all_five[0] == all_five[1]).sum() > 1500 and (two[0] == two[1]).sum() > 500
    # and the rule decides them: giving the atoms in another order changes the map only at tied voxels
    perm = [3, 2, 1, 0, 4]
    other = reference_labels(TIE_SHAPE, TIE_LATTICE, TIE_ATOMS[perm])
    moved = np.array(perm)[other].reshape(-1) != lab.reshape(-1)
    assert moved.any() and np.all((two[0] == two[1])[moved])


def test_the_inputs_of_the_gpu_tests_reach_both_routes():
    cap = _lib.XB_VORONOI_CAND_MAX
    for shape, lname, n in CANDIDATE_CASES:
        kept = candidate_counts(shape, LATTICES[lname], random_atoms(lname, n))
        print(shape, lname, n, 'keeps at most', kept.max(), 'of', 27 * n)
        assert kept.min() >= 1 and kept.max() <= cap // 2 and kept.max() < 27 * n // 4
    shape, lname, n = OVERFLOW_CASE
    kept = candidate_counts(shape, LATTICES[lname], random_atoms(lname, n))
    print(shape, lname, n, 'keeps', kept, 'of', 27 * n)
    assert kept.max() > cap + cap // 4 and 27 * n > cap
    for lname in LATTICES:
        kept = candidate_counts(MIXED_SHAPE, LATTICES[lname], random_atoms(lname, MIXED_N))
        print(MIXED_SHAPE, lname, MIXED_N, 'keeps', sorted(kept))
        assert kept.size == 3 * 2 * 5 and (kept > cap + cap // 8).sum() >= 4 and (kept < cap - cap // 8).sum() >= 4
    shape, lname, n = THIN_CASE
    assert candidate_counts(shape, LATTICES[lname], random_atoms(lname, n)).max() <= cap


def test_no_voxel_of_the_physics_case_lies_on_a_bisector():
    """2 x 2 x 2 atoms at (k + 1/2) h-type positions of a cubic cell: every atom gets N / 8 voxels"""
    shape, lat, atoms = physics_case()
    lab = reference_labels(shape, lat, atoms)
    assert np.bincount(lab.reshape(-1), minlength=8).tolist() == [int(np.prod(shape)) // 8] * 8


def physics_case():
    n, h = 24, 0.25
    lat = np.eye(3) * (n * h)
    # atoms at (3 + 1/2) h and (15 + 1/2) h on every axis: half a cell apart, half a voxel off the grid points, so a bisector
    # plane lies at a multiple of h/2 that is no multiple of h... it is: (3.5 + 15.5) / 2 = 9.5 h, between the planes 9 and 10
    pos = np.array([3.5, 15.5]) * h
    atoms = np.array([[x, y, z] for x in pos for y in pos for z in pos])
    return (n, n, n), lat, atoms


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_voronoi_names():
    hdr = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    text = hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_VORONOI_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_VORONOI_')}
    assert declared and declared == mirrored, set(declared.items()) ^ set(mirrored.items())
    assert set(declared) == {'XB_VORONOI_FULL_SEARCH', 'XB_VORONOI_CAND_MAX'} and declared['XB_VORONOI_FULL_SEARCH'] == 1
    cap = declared['XB_VORONOI_CAND_MAX']
    assert 64 <= cap <= 2048 and 2 * (cap * 32 + 1024) <= 160 * 1024, 'several workgroups fit the LDS of a compute unit'
    m = re.search(r'\bint\s+xb_voronoi_assign\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'include/bader_hip.h does not declare xb_voronoi_assign'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['xb_ctx *c', 'const double lattice[9]', 'const double *atoms_cart', 'int64_t n', 'double vac_tol', 'int flags',
                    'int64_t stats[3]']
    res, argtypes = _lib.SYMBOLS['xb_voronoi_assign']
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert res is C.c_int and argtypes == [C.c_void_p, pd, pd, C.c_int64, C.c_double, C.c_int, pi]
    assert callable(getattr(_lib.Context, 'voronoi_assign'))
    # the kernel sizes its list by the header's name, and the definition is written down where the issue asks for it
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_voronoi.h')).read()
    assert 's_cand[XB_VORONOI_CAND_MAX]' in src and '#define VO_TILE %d' % TILE in src
    assert 'TIES GO TO THE SMALLER' in text and 'e[j] = pc[j] - (atom[a][j] + pbc[j])' in text
    # no timer slot and no option key came with it
    assert _lib.XB_TIMER_COUNT == 11 and not hasattr(_lib, 'XB_TIMER_VORONOI')


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.voronoi_flag is False and callable(Bader.voronoi_partition)


def test_voronoi_assign_needs_the_gpu():
    from pybader_amd import build
    build.build_library()
    if _lib.load().xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.ones((4, 4, 4))
    with pytest.raises(_lib.BaderHipError):
        voronoi.voronoi_assign(rho, np.eye(3) * 4.0, np.ones((1, 3)))
    with pytest.raises(_lib.BaderHipError):
        voronoi.voronoi_charges(rho, np.eye(3) * 4.0, np.ones((1, 3)), 1.0)

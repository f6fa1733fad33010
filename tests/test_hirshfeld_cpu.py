"""The host side of the Hirshfeld charges (pybader_amd/hirshfeld.py, xb_hirshfeld_images) and the plain numpy restatement of the
definition in include/bader_hip.h / DESIGN.md section 19 that tests/test_gpu_hirshfeld.py compares the kernels with: the fields
with ==, the sums per atom under the float64 sum bound of sections 13 and 18.

`restate` is elementwise IEEE float64 in the order the definition writes, over the canonical image list, so P and every p_a carry
the bits the device forms.  `image_list` restates the list (with `widen` a visibly wider one: no result depends on the range);
`candidate_counts` restates phase 1 of csrc/k_hirshfeld.h (which images a tile keeps): the GPU tests assert from the call's
statistics which route the tiles took, and the checks here say, without a GPU, that their inputs do reach those routes."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, build, hirshfeld, synth
from pybader_amd.hirshfeld import ProAtoms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8
U = 2.0 ** -53
VV = 0.0371             # a voxel volume that is no power of two
CAP = _lib.XB_HIRSHFELD_CAND_MAX


@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def inverse_by_cofactors(lat):
    A = np.asarray(lat, dtype=np.float64).reshape(3, 3)
    Cf = np.zeros((3, 3))
    for i in range(3):
        for b in range(3):
            i1, i2, b1, b2 = (i + 1) % 3, (i + 2) % 3, (b + 1) % 3, (b + 2) % 3
            Cf[i, b] = A[i1, b1] * A[i2, b2] - A[i1, b2] * A[i2, b1]
    det = (A[0, 0] * Cf[0, 0] + A[0, 1] * Cf[0, 1]) + A[0, 2] * Cf[0, 2]
    return Cf.T / det


def shift_ranges(lattice, atoms, species, r_cut):
    """lo[n, 3], hi[n, 3] of the definition, every operation in its order"""
    M = inverse_by_cofactors(lattice)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    lo, hi = np.zeros(atoms.shape, np.int64), np.zeros(atoms.shape, np.int64)
    for a, at in enumerate(atoms):
        for i in range(3):
            f = (at[0] * M[0, i] + at[1] * M[1, i]) + at[2] * M[2, i]
            g = np.sqrt((M[0, i] * M[0, i] + M[1, i] * M[1, i]) + M[2, i] * M[2, i])
            rho = np.float64(r_cut[species[a]]) * g
            m = np.float64(2.0 ** -20) * ((np.float64(1.0) + abs(f)) + rho)
            lo[a, i] = int(np.floor((-rho - f) - m))
            hi[a, i] = int(np.ceil(((np.float64(1.0) + rho) - f) + m))
    return lo, hi


def image_list(lattice, atoms, species, r_cut, widen=0):
    """the canonical list, int32[m, 4] rows (a, x, y, z); `widen` more shifts at either end of every range"""
    lo, hi = shift_ranges(lattice, atoms, species, r_cut)
    rows = []
    for a in range(lo.shape[0]):
        r = [np.arange(lo[a, i] - widen, hi[a, i] + widen + 1) for i in range(3)]
        x, y, z = (g.reshape(-1) for g in np.meshgrid(*r, indexing='ij'))
        rows.append(np.stack([np.full(x.size, a), x, y, z], axis=1))
    return np.concatenate(rows).astype(np.int32)


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


def restate(shape, lattice, atoms, species, pro, widen=0, prefilter=False):
    """-> (P f64[N], p f64[n, N]): the promolecular density and every atom's share of it, by the definition.

    `prefilter` only saves time on long thin grids: the voxels are taken in runs of 256 (C order), each with a centre and a radius,
    and an image is evaluated at the runs within r_cut + radius + 1e-9 (1 + r_cut + radius) of it alone -- nine orders of magnitude
    more than the rounding of that test, so every voxel left out has d2 >= rc2 and the definition's term 0.  The values formed are
    the same elementwise expressions either way (test_the_prefilter_of_the_restatement_changes_no_bit)."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(9)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    K = pro.knots
    pc = _positions(shape, lat)
    N = pc[0].size
    P, p = np.zeros(N), np.zeros((atoms.shape[0], N))
    rc2 = pro.r_cut * pro.r_cut
    ih2 = np.float64(K) / rc2
    if prefilter:
        B = 256
        nb = -(-N // B)
        pad = [np.concatenate([c, np.full(nb * B - N, c[-1])]).reshape(nb, B) for c in pc]
        centre = [c.mean(axis=1) for c in pad]
        radius = np.sqrt(sum((pad[j] - centre[j][:, None]) ** 2 for j in range(3))).max(axis=1)
    for a, x, y, z in image_list(lattice, atoms, species, pro.r_cut, widen):
        s = species[a]
        q = [atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        if prefilter:
            reach = pro.r_cut[s] + radius
            near = np.sqrt(sum((centre[j] - q[j]) ** 2 for j in range(3))) <= reach + 1e-9 * (1.0 + reach)
            if not near.any():
                continue
            at = np.flatnonzero(np.repeat(near, B)[:N])
        else:
            at = np.arange(N)
        e = [pc[j][at] - q[j] for j in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        inside = np.flatnonzero(d2 < rc2[s])
        if inside.size:
            u = d2[inside] * ih2[s]
            k = np.minimum(u.astype(np.int64), K - 1)
            t = u - k.astype(np.float64)
            f = pro.tables[s]
            term = np.zeros(N)
            term[at[inside]] = f[k] + t * (f[k + 1] - f[k])
            P = P + term
            p[a] = p[a] + term
    return P, p


def restate_scalar(shape, lattice, atoms, species, pro, images):
    """the same, one voxel and image at a time in Python floats (IEEE float64)"""
    lat = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = [[float(x) for x in at] for at in np.asarray(atoms, dtype=np.float64).reshape(-1, 3)]
    nx, ny, nz = shape
    K = pro.knots
    P, p = np.zeros(shape), np.zeros((len(atoms),) + tuple(shape))
    for p0 in range(nx):
        for p1 in range(ny):
            for p2 in range(nz):
                pc = []
                for j in range(3):
                    c = lat[j] * p0 / nx
                    c += lat[3 + j] * p1 / ny
                    c += lat[6 + j] * p2 / nz
                    pc.append(c)
                for a, x, y, z in images:
                    s = int(species[a])
                    rc = float(pro.r_cut[s])
                    rc2 = rc * rc
                    e = [pc[j] - (atoms[a][j] + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                    term = 0.0
                    if not d2 >= rc2:
                        u = d2 * (K / rc2)
                        k = min(int(u), K - 1)
                        t = u - k
                        f = pro.tables[s]
                        term = float(f[k]) + t * (float(f[k + 1]) - float(f[k]))
                    P[p0, p1, p2] += term
                    p[a, p0, p1, p2] += term
    return P.reshape(-1), p.reshape(len(atoms), -1)


def sum_bound(count, mag, vv=VV):
    """the float64 sum bound of sections 13 and 18: `count` terms of total magnitude `mag`, in any order"""
    return (np.asarray(count) + 2) * U * np.asarray(mag) * abs(vv)


def restated_sums(rho, P, p):
    """-> dict: charge, volume (fsum, before voxel_volume), their term counts and magnitudes, rest (sum, count), the terms"""
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    have = P > 0
    w = np.zeros_like(p)
    w[:, have] = p[:, have] / P[have]
    term = rho * w
    out = {
        'charge': np.array([math.fsum(t) for t in term]), 'volume': np.array([math.fsum(x) for x in w]),
        'count': (w != 0).sum(axis=1), 'charge_mag': np.abs(term).sum(axis=1), 'volume_mag': w.sum(axis=1),
        'rest': (math.fsum(rho[~have]), int((~have).sum())), 'rest_mag': float(np.abs(rho[~have]).sum()), 'term': term, 'w': w,
    }
    return out


def candidate_counts(shape, lattice, atoms, species, pro):
    """phase 1 of csrc/k_hirshfeld.h restated WITH THE KERNEL'S OWN EXPRESSIONS, operation by operation in IEEE float64: per 8^3 tile
    (C order over the tiles) the number of images it keeps -- those within r_cut + R + slack of the centre of the tile's voxels, R
    half the longest body diagonal of the box they span.  The same bits decide, so the GPU tests may ask the call's statistics to
    equal these counts exactly, whether or not an image lies within rounding of a tile's limit."""
    lat = [np.float64(v) for v in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    img = image_list(lattice, atoms, species, pro.r_cut)
    sx, sy, sz = (img[:, k].astype(np.float64) for k in (1, 2, 3))
    q = [atoms[img[:, 0], j] + ((lat[j] * sx + lat[3 + j] * sy) + lat[6 + j] * sz) for j in range(3)]
    rc = pro.r_cut[np.asarray(species)[img[:, 0]]]
    length = np.float64(0.0)
    for k in range(3):
        length = length + np.sqrt((lat[3 * k] * lat[3 * k] + lat[3 * k + 1] * lat[3 * k + 1]) + lat[3 * k + 2] * lat[3 * k + 2])
    nx, ny, nz = (np.float64(n) for n in shape)
    tiny = np.float64(2.0 ** -40)
    out = []
    for x0 in range(0, shape[0], TILE):
        for y0 in range(0, shape[1], TILE):
            for z0 in range(0, shape[2], TILE):
                ex, ey, ez = (np.float64(min(TILE, n - o) - 1) for n, o in zip(shape, (x0, y0, z0)))
                fx, fy, fz = np.float64(x0) + 0.5 * ex, np.float64(y0) + 0.5 * ey, np.float64(z0) + 0.5 * ez
                c, u = [], [[], [], []]
                for j in range(3):
                    cj = lat[j] * fx / nx
                    cj = cj + lat[3 + j] * fy / ny
                    cj = cj + lat[6 + j] * fz / nz
                    c.append(cj)
                    u[0].append(lat[j] * ex / nx)
                    u[1].append(lat[3 + j] * ey / ny)
                    u[2].append(lat[6 + j] * ez / nz)
                diag2 = np.float64(0.0)
                for sgn in range(4):
                    s1, s2 = (-1.0 if sgn & 1 else 1.0), (-1.0 if sgn & 2 else 1.0)
                    d2 = np.float64(0.0)
                    for j in range(3):
                        d = (u[0][j] + s1 * u[1][j]) + s2 * u[2][j]
                        d2 = d2 + d * d
                    diag2 = max(diag2, d2)
                R = 0.5 * np.sqrt(diag2)
                lim = rc + R
                lim = lim + tiny * (lim + length)
                lim2 = lim * lim
                lim2 = lim2 + tiny * lim2
                e = [c[j] - q[j] for j in range(3)]
                out.append(int((((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= lim2).sum()))
    return np.array(out)


# ---- inputs (shared with tests/test_gpu_hirshfeld.py) -------------------------------------------------------------------------
def synth_proatoms(atoms5, r_cut, knots):
    """pro-atoms sampled from synth's own atom profile A max(0, 1 - r^2 / (2048 s^2))^1024, one species per atom: a function of r^2,
    so the knots are exact; the last knot is the table's zero"""
    atoms5 = np.asarray(atoms5, dtype=np.float64)
    x = np.arange(knots + 1, dtype=np.float64) * (np.float64(r_cut) * np.float64(r_cut)) / np.float64(knots)
    tab = np.zeros((atoms5.shape[0], knots + 1))
    for s, a in enumerate(atoms5):
        t = np.maximum(np.float64(1.0) - x / (np.float64(2048.0) * a[3] * a[3]), 0.0)
        for _ in range(10):
            t = t * t
        tab[s] = a[4] * t
    tab[:, -1] = 0.0
    return ProAtoms(tab, np.full(atoms5.shape[0], float(r_cut)))


def bump_proatoms(r_cut, knots):
    """one species, (1 - r^2 / r_cut^2)^2: broad, so that every image in reach of a voxel matters to its bits"""
    x = np.arange(knots + 1, dtype=np.float64) / knots
    tab = (1.0 - x) ** 2
    tab[-1] = 0.0
    return ProAtoms(tab[None, :], [float(r_cut)])


LATTICES = {'cubic': synth.CUBIC6, 'tric': synth.TRICLINIC, 'small': synth.CUBIC6 * 0.4}
# name -> (shape, lattice, atoms, r_cut, knots, the route its tiles take)
CASES = {
    'cubic_r2': ((24, 24, 24), 'cubic', 'atoms8', 2.0, 4096, 'candidate'),
    'tric_r2': ((24, 24, 24), 'tric', 'atoms8', 2.0, 4096, 'candidate'),
    'cubic_r3': ((24, 24, 24), 'cubic', 'atoms8', 3.0, 4096, 'candidate'),
    'tric_r3': ((24, 24, 24), 'tric', 'atoms8', 3.0, 4096, 'candidate'),
    'partial': ((40, 36, 44), 'tric', 'atoms8', 3.0, 4096, 'candidate'),
    'odd_k1': ((20, 9, 33), 'cubic', 'atoms8', 3.0, 1, 'candidate'),
    'three': ((3, 3, 3), 'tric', 'atoms8', 3.0, 4096, 'candidate'),
    'thin': ((1, 2, 9), 'cubic', 'atoms8', 2.0, 4096, 'candidate'),
    'small_cell': ((12, 12, 12), 'small', 'atoms8', 3.0, 4096, 'candidate'),
    'twins': ((16, 12, 20), 'tric', 'twins', 2.5, 4096, 'candidate'),
    'many_overflow': ((16, 16, 16), 'cubic', 'grid216', 3.5, 32, 'overflow'),
    'many_candidate': ((32, 32, 32), 'cubic', 'grid216', 1.2, 32, 'candidate'),
    'many_mixed': ((20, 9, 33), 'cubic', 'grid216', 2.0, 32, 'mixed'),
    # more atoms than the sums' kernel has bins (343 > XB_HIRSHFELD_CAND_MAX): bins per slot of the tile's list, flushed per tile
    'more_candidate': ((24, 24, 24), 'cubic', 'grid343', 1.0, 32, 'candidate'),
    'more_overflow': ((16, 16, 16), 'cubic', 'grid343', 3.0, 32, 'overflow'),
    'more_mixed': ((20, 9, 33), 'cubic', 'grid343', 2.0, 32, 'mixed'),
    # more tiles than a sums launch has workgroups on any card of up to 256 compute units (4 x 7 x 256 = 7168): a workgroup takes
    # several tiles, with bins per atom kept over them (8 atoms) and with bins per slot flushed and cleared after each (343 atoms)
    'line': ((1, 1, 160000), 'cubic', 'atoms8', 2.2, 4096, 'candidate'),
    'line_more': ((1, 1, 64000), 'cubic', 'grid343', 0.8, 32, 'candidate'),
}
LONG = ('line', 'line_more')      # restated with the prefilter
FIELD_CASES = list(CASES)
SUM_CASES = list(CASES)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name):
    """one input of the GPU tests: shape, lattice, atoms (Cartesian), species, pro, rho -- built once, never written"""
    shape, lname, kind, r_cut, knots, route = CASES[name]
    c = Case()
    c.name, c.shape, c.lattice, c.route = name, shape, LATTICES[lname], route
    if kind in ('grid216', 'grid343'):
        a5 = synth.atoms_jittered_grid(6 if kind == 'grid216' else 7)
        c.atoms = np.ascontiguousarray(a5[:, :3] @ c.lattice)
        c.species = np.zeros(a5.shape[0], np.int32)
        c.pro = bump_proatoms(r_cut, knots)
        c.rho = synth.synth_density(shape, c.lattice, a5)
    else:
        a5 = synth.ATOMS8
        c.atoms = np.ascontiguousarray(a5[:, :3] @ c.lattice)
        c.species = np.arange(8, dtype=np.int32)
        c.pro = synth_proatoms(a5, r_cut, knots)
        c.rho = synth.synth_density(shape, c.lattice, a5) - synth.BACKGROUND
        if name == 'thin':
            c.atoms = c.atoms.copy()
            c.atoms[2] += c.lattice[0] - 2 * c.lattice[2]      # an atom outside the cell: taken as given
        if kind == 'twins':
            # atom 8 is atom 3 again (same place, same species); species 8 is a second row with species 0's table, taken by atom 1
            c.atoms = np.ascontiguousarray(np.concatenate([c.atoms, c.atoms[3:4]]))
            c.species = np.array([0, 8, 2, 3, 4, 5, 6, 7, 3], np.int32)
            c.pro = ProAtoms(np.concatenate([c.pro.tables, c.pro.tables[0:1]]), np.concatenate([c.pro.r_cut, c.pro.r_cut[0:1]]))
    for a in (c.atoms, c.species, c.rho, c.pro.tables, c.pro.r_cut):
        a.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(P, p) of one input of the GPU tests, computed once and never written"""
    c = case(name)
    P, p = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, prefilter=name in LONG)
    P.flags.writeable = False
    p.flags.writeable = False
    return P, p


@functools.lru_cache(maxsize=None)
def reference_sums(name, f32=False):
    c = case(name)
    rho = c.rho.astype(np.float32).astype(np.float64) if f32 else c.rho
    return restated_sums(rho, *reference(name))


def n_tiles(shape):
    return int(np.prod([-(-s // TILE) for s in shape]))


# ---- the image list: the test that fails without the feature ------------------------------------------------------------------
def list_inputs():
    a8 = synth.ATOMS8
    for lname in ('cubic', 'tric'):
        lat = LATTICES[lname]
        yield f'atoms8 {lname}', lat, a8[:, :3] @ lat, np.arange(8), np.array([3.0, 2.0, 2.5, 1.0, 3.5, 0.5, 2.0, 4.0])
    lat = LATTICES['tric']
    out = (a8[:, :3] @ lat).copy()
    out[1] += 2 * lat[0] - lat[1]
    out[6] -= 3 * lat[2]
    yield 'atoms outside the cell', lat, out, np.zeros(8, np.int64), np.array([2.0])
    lat = LATTICES['small']
    yield '2.4 A cell, r_cut 3', lat, a8[:, :3] @ lat, np.zeros(8, np.int64), np.array([3.0])


def test_image_list_of_the_library_equals_the_restatement(lib):
    for what, lat, atoms, species, r_cut in list_inputs():
        want = image_list(lat, atoms, species, r_cut)
        got = _lib.hirshfeld_images(lat, atoms, species, r_cut)
        per_atom = np.bincount(want[:, 0])
        print(f'{what}: {want.shape[0]} images, {per_atom.min()} to {per_atom.max()} per atom')
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), what
        # canonical: a ascending, then x, y, z ascending
        key = [tuple(r) for r in got.tolist()]
        assert key == sorted(key) and len(set(key)) == len(key)
        if '2.4' in what:
            assert per_atom.min() > 27
    # the range covers every image in reach: a brute force over a much wider one finds no other image within r_cut of a voxel
    for what, lat, atoms, species, r_cut in list_inputs():
        shape = (6, 5, 7)
        pc = np.stack(_positions(shape, np.asarray(lat).reshape(9)), axis=1)
        have = set(tuple(r) for r in image_list(lat, atoms, species, r_cut).tolist())
        for a, x, y, z in image_list(lat, atoms, species, r_cut, widen=2):
            if (a, x, y, z) not in have:
                q = atoms[a] + np.array([x, y, z], dtype=np.float64) @ np.asarray(lat)
                assert ((pc - q) ** 2).sum(axis=1).min() >= r_cut[species[a]] ** 2, (what, a, x, y, z)


def test_image_list_errors(lib):
    lat, atoms, sp, rc = np.eye(3) * 4.0, np.full((2, 3), 2.0), np.zeros(2, np.int32), np.array([1.0])

    def code(*args):
        with pytest.raises(_lib.BaderHipError) as e:
            _lib.hirshfeld_images(*args)
        return e.value.code

    assert _lib.hirshfeld_images(lat, atoms, sp, rc).shape == (2 * 27, 4)
    assert code(lat, atoms, np.array([0, 1], np.int32), rc) == _lib.XB_E_ARG          # a species outside [0, S)
    assert code(lat, atoms, np.array([0, -1], np.int32), rc) == _lib.XB_E_ARG
    assert code(lat, atoms, sp, np.array([0.0])) == _lib.XB_E_ARG
    assert code(lat, atoms, sp, np.array([np.inf])) == _lib.XB_E_ARG
    assert code(lat, atoms * np.nan, sp, rc) == _lib.XB_E_ARG
    assert code(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]), atoms, sp, rc) == _lib.XB_E_ARG   # determinant exactly 0
    assert code(np.where(lat != 0, np.inf, 0.0), atoms, sp, rc) == _lib.XB_E_ARG
    assert code(lat, atoms, sp, np.array([1e4])) == _lib.XB_E_LIMIT                   # 5001^3 images per atom
    assert code(lat, np.zeros((0, 3)), np.zeros(0, np.int32), rc) == _lib.XB_E_ARG


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', ['cubic', 'tric'])
def test_restatement_against_a_scalar_triple_loop(lname):
    shape, lat = (5, 7, 11), LATTICES[lname]
    atoms = synth.ATOMS8[:, :3] @ lat
    species = np.arange(8)
    pro = synth_proatoms(synth.ATOMS8, 2.5, 16)
    P, p = restate(shape, lat, atoms, species, pro)
    Ps, ps = restate_scalar(shape, lat, atoms, species, pro, image_list(lat, atoms, species, pro.r_cut).tolist())
    assert np.array_equal(P, Ps) and np.array_equal(p, ps)
    assert (P > 0).all() and (p > 0).any(axis=1).all()


@pytest.mark.parametrize('name', ['cubic_r2', 'tric_r3', 'small_cell', 'thin'])
def test_a_doubled_image_range_gives_the_same_bits(name):
    c = case(name)
    P, p = reference(name)
    lo, hi = shift_ranges(c.lattice, c.atoms, c.species, c.pro.r_cut)
    widen = int((hi - lo + 1).max() + 1) // 2
    more = image_list(c.lattice, c.atoms, c.species, c.pro.r_cut, widen).shape[0]
    assert more >= 4 * image_list(c.lattice, c.atoms, c.species, c.pro.r_cut).shape[0]
    P2, p2 = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, widen=widen)
    assert np.array_equal(P, P2) and np.array_equal(p, p2)


@pytest.mark.parametrize('name', ['tric_r2', 'thin', 'three', 'many_mixed'])
def test_the_prefilter_of_the_restatement_changes_no_bit(name):
    c = case(name)
    P, p = reference(name)
    P2, p2 = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, prefilter=True)
    assert np.array_equal(P.view(np.uint64), P2.view(np.uint64)) and np.array_equal(p.view(np.uint64), p2.view(np.uint64))


def test_the_long_grids_against_the_scalar_definition_at_voxels_across_them():
    """the two grids of more than 7168 tiles are restated with the prefilter; here voxels picked across them are formed one image
    at a time in Python floats over the whole list, without it"""
    for name in LONG:
        c = case(name)
        P, p = reference(name)
        assert c.shape[:2] == (1, 1)
        pick = [0, 1, 7, 8, c.shape[2] // 3, c.shape[2] // 2 + 5, c.shape[2] - 9, c.shape[2] - 1]
        images = image_list(c.lattice, c.atoms, c.species, c.pro.r_cut).tolist()
        lat = [float(v) for v in np.asarray(c.lattice).reshape(9)]
        K = c.pro.knots
        for v in pick:
            pc = []
            for j in range(3):
                x = lat[j] * 0 / c.shape[0]
                x += lat[3 + j] * 0 / c.shape[1]
                x += lat[6 + j] * v / c.shape[2]
                pc.append(x)
            tot, mine = 0.0, [0.0] * c.atoms.shape[0]
            for a, x, y, z in images:
                sp = int(c.species[a])
                rc2 = float(c.pro.r_cut[sp]) * float(c.pro.r_cut[sp])
                e = [pc[j] - (float(c.atoms[a][j]) + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                if d2 >= rc2:
                    continue
                u = d2 * (K / rc2)
                k = min(int(u), K - 1)
                f = c.pro.tables[sp]
                term = float(f[k]) + (u - k) * (float(f[k + 1]) - float(f[k]))
                tot += term
                mine[a] += term
            assert tot == P[v] and mine == p[:, v].tolist(), (name, v)
        assert n_tiles(c.shape) > 4 * 7 * 256


@pytest.mark.parametrize('name', SUM_CASES)
def test_partition_of_unity(name):
    """sum_a term_a + [P == 0] rho sums to the density's sum, within the bound of a sum of all those terms"""
    c = case(name)
    s = reference_sums(name)
    total = math.fsum(s['charge']) + s['rest'][0]
    want = math.fsum(c.rho.reshape(-1))
    # every voxel's weights sum to 1 within n roundings of the running sum and one per division
    n = c.atoms.shape[0]
    per_voxel = (2 * n + 2) * U * np.abs(c.rho).sum()
    lim = per_voxel + (c.rho.size + 2) * U * np.abs(c.rho).sum()
    print(f'{name}: sum of the shares {total!r}, of the density {want!r}, bound {lim:.3e}, rest {s["rest"]}')
    assert abs(total - want) <= lim
    if name.endswith('_r2'):
        assert s['rest'][1] > 0 and s['rest'][0] != 0
    if name.endswith('_r3'):
        assert s['rest'] == (0.0, 0)
    if name == 'twins':
        _, p = reference(name)
        assert np.array_equal(p[3], p[8]) and np.array_equal(s['term'][3], s['term'][8]), 'a duplicated atom gets the bits of its twin'
        assert s['charge'][3] == s['charge'][8] and s['volume'][3] == s['volume'][8]


# ---- physics, pinned on the CPU -------------------------------------------------------------------------------------------------
def shortest_lattice_vector(lat):
    r = np.arange(-2, 3)
    v = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)
    v = v[(v != 0).any(axis=1)].astype(np.float64) @ np.asarray(lat)
    return float(np.sqrt((v * v).sum(axis=1).min()))


@pytest.mark.parametrize('name', ['cubic_r3', 'tric_r3'])
def test_physics_the_promolecule_of_synths_own_atoms_is_the_density(name):
    """synth_density(24^3) - BACKGROUND is a sum of A g(r^2), g(x) = max(0, 1 - x / (2048 s^2))^1024, over ONE image per atom (the
    one rint picks); the pro-atoms are g at the knots (exact: g is a function of r^2), r_cut = 3, K = 4096, h2 = 9 / 4096.

    TOLERANCE eps for |rho - P| at a voxel, per atom and summed over the atoms (each source is bounded where it is largest):
      interpolation  h2^2 / 8 max |f''|,  f'' = A 1024 1023 / (2048 s^2)^2 (1 - x / (2048 s^2))^1022 <= A 1024 1023 / (2048 s^2)^2
      the cutoff     the image rint picks may lie at or beyond r_cut, where P has 0 and rho has A g(d2) <= A g(9); the table's last
                     interval runs to 0 instead of g(9): at most A g(9) more
      other images   P counts every image within r_cut, rho only rint's.  Another image differs from rint's by a lattice vector, so
                     one of its fractional components is at least 1/2 in magnitude and it lies at least h_min / 2 from the voxel
                     (h_min the cell's smallest height).  Three images within r_cut of one voxel do not exist: three points
                     pairwise >= lambda apart (lambda the shortest lattice vector) need a ball of radius lambda / sqrt(3), which
                     is > 3 in both cells (asserted).  So at most two images count: 2 A g(min(r_cut, h_min / 2)^2)
      rounding       1e-13 max rho covers the few hundred roundings of either side
    Measured, for orientation: 5.5e-6 max rho (cubic).

    CHARGES.  charge_a - vv sum_v p_a = vv sum_v p_a (rho / P - 1) = vv sum_v w_a (rho - P), so it is at most eps * volume_a (plus
    the rounding of the two sums: their bound).  Both cells leave no voxel with P == 0 (asserted)."""
    c = case(name)
    P, p = reference(name)
    s = reference_sums(name)
    rho = c.rho.reshape(-1)
    assert (P > 0).all() and s['rest'] == (0.0, 0)
    lat = np.asarray(c.lattice)
    vol = abs(np.linalg.det(lat))
    h_min = min(vol / np.linalg.norm(np.cross(lat[(i + 1) % 3], lat[(i + 2) % 3])) for i in range(3))
    lam = shortest_lattice_vector(lat)
    r_cut, K = 3.0, 4096
    assert lam / np.sqrt(3.0) > r_cut
    h2 = r_cut * r_cut / K
    near = min(r_cut, h_min / 2) ** 2
    eps = 1e-13 * rho.max()
    for _, _, _, sg, A in synth.ATOMS8:
        R2 = 2048.0 * sg * sg
        g = lambda x: max(0.0, 1.0 - x / R2) ** 1024
        eps += h2 * h2 / 8 * A * 1024 * 1023 / (R2 * R2) + 2 * A * g(r_cut * r_cut) + 2 * A * g(near)
    err = np.abs(rho - P).max()
    print(f'{name}: max |rho - P| = {err:.3e} = {err / rho.max():.3e} max rho; eps = {eps:.3e} = {eps / rho.max():.3e} max rho')
    assert err <= eps and eps < 1e-4 * rho.max()
    vv = vol / rho.size
    for a in range(8):
        pa = math.fsum(p[a]) * vv
        q, v = s['charge'][a] * vv, s['volume'][a] * vv
        lim = eps * v + sum_bound(s['count'][a], s['charge_mag'][a], vv) + sum_bound(s['count'][a], p[a].sum(), vv)
        print(f'  atom {a}: Hirshfeld {q:.9f}, pro-atom {pa:.9f}, relative difference {abs(q - pa) / pa:.2e}, allowed {lim / pa:.2e}')
        assert abs(q - pa) <= lim
    # the exact integral of the profile is A pi^(3/2) R^3 Gamma(1025) / Gamma(1026.5), R^2 = 2048 s^2 -- not (2 pi)^(3/2) A s^3
    sg, A = synth.ATOMS8[0, 3], synth.ATOMS8[0, 4]
    exact = A * math.pi ** 1.5 * (2048 * sg * sg) ** 1.5 * math.exp(math.lgamma(1025) - math.lgamma(1026.5))
    assert abs(exact / ((2 * math.pi) ** 1.5 * A * sg ** 3) - 1) == pytest.approx(1.8e-3, rel=0.05)


# ---- routing ----------------------------------------------------------------------------------------------------------------
def test_the_inputs_of_the_gpu_tests_reach_their_routes():
    for name, (shape, *_, route) in CASES.items():
        c = case(name)
        kept = candidate_counts(shape, c.lattice, c.atoms, c.species, c.pro)
        total = image_list(c.lattice, c.atoms, c.species, c.pro.r_cut).shape[0]
        print(f'{name}: {kept.size} tiles keep {kept.min()} to {kept.max()} of {total} images ({route})')
        assert kept.size == n_tiles(shape) and (kept.min() >= 1 or name == 'line')
        if name == 'line':
            # stretches of this line lie beyond every pro-atom: tiles with an empty list, and voxels that belong to nobody, whose
            # density a workgroup gathers over its tiles
            assert (kept == 0).sum() > n_tiles(shape) // 3 and (kept > 0).sum() > n_tiles(shape) // 3 and reference_sums(name)["rest"][1] > c.rho.size // 3
        if route == 'candidate':
            assert kept.max() <= CAP - CAP // 8
        elif route == 'overflow':
            assert kept.min() > CAP + CAP // 8
        else:
            assert (kept > CAP + CAP // 8).sum() >= 2 and (kept < CAP - CAP // 8).sum() >= 2
            assert not ((kept > CAP - 2) & (kept < CAP + 2)).any()
    # what a tile NEEDS -- the images with a non-zero term at one of its voxels -- is 14 (cubic) and 16 (triclinic) at most at 24^3
    # with r_cut = 3; phase 1 keeps a superset of it in every tile
    for name, want in (('cubic_r3', 14), ('tric_r3', 16)):
        c = case(name)
        need = needed_counts(c.shape, c.lattice, c.atoms, c.species, c.pro)
        kept = candidate_counts(c.shape, c.lattice, c.atoms, c.species, c.pro)
        assert need.max() == want and (kept >= need).all()


def needed_counts(shape, lattice, atoms, species, pro):
    """per 8^3 tile the number of images of the list with d2 < rc2 at one of its voxels at least"""
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    pc = np.stack(_positions(shape, lat.reshape(9)), axis=1).reshape(tuple(shape) + (3,))
    img = image_list(lattice, atoms, species, pro.r_cut)
    q = np.asarray(atoms)[img[:, 0]] + img[:, 1:].astype(np.float64) @ lat
    rc2 = (pro.r_cut * pro.r_cut)[np.asarray(species)[img[:, 0]]]
    out = []
    for x0 in range(0, shape[0], TILE):
        for y0 in range(0, shape[1], TILE):
            for z0 in range(0, shape[2], TILE):
                v = pc[x0:x0 + TILE, y0:y0 + TILE, z0:z0 + TILE].reshape(-1, 3)
                d2 = ((v[:, None, :] - q[None, :, :]) ** 2).sum(axis=2)
                out.append(int((d2 < rc2[None, :]).any(axis=0).sum()))
    return np.array(out)


# ---- the constructors -----------------------------------------------------------------------------------------------------------
def test_from_radial_on_a_known_profile():
    r = np.linspace(0.0, 4.0, 4001)
    pro = ProAtoms.from_radial([(r, np.exp(-r * r)), (r, 2.0 * np.exp(-0.5 * r * r))], [2.0, 3.0], knots=512)
    assert pro.tables.shape == (2, 513) and pro.knots == 512 and pro.n_species == 2 and pro.r_cut.tolist() == [2.0, 3.0]
    assert (pro.tables[:, -1] == 0).all() and (pro.tables >= 0).all()
    for s, (amp, alpha) in enumerate([(1.0, 1.0), (2.0, 0.5)]):
        x = np.arange(513) * pro.r_cut[s] ** 2 / 512            # the knots' r^2
        want = amp * np.exp(-alpha * x)
        # linear interpolation of the profile on a 1e-3 mesh: (1e-3)^2 / 8 max |d2/dr2| <= 1e-6 / 8 * 2 amp alpha
        assert np.abs(pro.tables[s, :-1] - want[:-1]).max() <= 1e-6 / 8 * 2 * amp * alpha * 1.01
    assert np.array_equal(ProAtoms.knot_radii(2.0, 4), np.sqrt(np.arange(5) * 4.0 / 4))
    one = ProAtoms.from_radial([(r, np.exp(-r * r))], 2.0)
    assert one.knots == 4096 and one.joined(one).tables.shape == (2, 4097)
    with pytest.raises(ValueError):
        ProAtoms(np.zeros((2, 5)), [1.0])


def test_from_density_on_a_free_atom_in_a_box():
    shape, lat = (40, 40, 40), np.eye(3) * 8.0
    centre = np.array([4.1, 3.9, 4.05])
    frac = np.stack(np.meshgrid(*(np.arange(n) / n for n in shape), indexing='ij'), -1)
    d = frac - centre / 8.0
    d -= np.rint(d)
    r2 = ((d * 8.0) ** 2).sum(axis=-1)
    rho = 3.0 * np.exp(-0.7 * r2)
    pro = ProAtoms.from_density(rho, lat, centre, 3.0, knots=64)
    assert pro.tables.shape == (1, 65) and pro.tables[0, -1] == 0 and pro.r_cut.tolist() == [3.0]
    x = np.arange(65) * 9.0 / 64
    # a bin is half a knot spacing wide either way: the average of 3 exp(-0.7 x) over it lies within the profile's range there
    half = 0.5 * 9.0 / 64
    lo, hi = 3.0 * np.exp(-0.7 * (x + half)), 3.0 * np.exp(-0.7 * np.maximum(x - half, 0.0))
    got = pro.tables[0]
    assert (got[:-1] >= lo[:-1] * (1 - 1e-12)).all() and (got[:-1] <= hi[:-1] * (1 + 1e-12)).all()


# ---- what the sums' bound is worth --------------------------------------------------------------------------------------------
def test_the_sums_bound_notices_a_voxel_weighed_for_the_wrong_atom():
    """one voxel's weight given to another atom moves both atoms' charge and volume by more than the bound, on every input of the
    GPU sums -- and the voxel is a typical one of its atom (the median magnitude), not the largest"""
    for name in SUM_CASES:
        s = reference_sums(name)
        a = int(np.argmax(s['count']))                                   # the atom with the most terms: the widest bound
        b = int(next(x for x in np.argsort(-s['count']) if x != a))
        mine = np.flatnonzero(s['term'][a] != 0)
        v = mine[np.argsort(np.abs(s['term'][a][mine]))[mine.size // 2]]
        for x in (a, b):
            assert abs(s['term'][a][v]) * VV > sum_bound(s['count'][x] + 1, s['charge_mag'][x] + abs(s['term'][a][v])), (name, x)
            assert s['w'][a][v] * VV > sum_bound(s['count'][x] + 1, s['volume_mag'][x] + s['w'][a][v]), (name, x)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_hirshfeld_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_HIRSHFELD_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_HIRSHFELD_')}
    assert declared and declared == mirrored, set(declared.items()) ^ set(mirrored.items())
    assert declared == {'XB_HIRSHFELD_FULL_SEARCH': 1, 'XB_HIRSHFELD_CAND_MAX': CAP, 'XB_HIRSHFELD_PROMOLECULE': 0,
                        'XB_HIRSHFELD_DEFORMATION': 1}
    assert 64 <= CAP <= 1024 and 8 * (CAP * (48 + 20) + 64) <= 160 * 1024, 'eight workgroups fit the LDS of a compute unit'
    want = {
        'xb_hirshfeld_images': ['const double lattice[9]', 'const double *atoms_cart', 'const int32_t *species', 'int64_t n',
                                'const double *r_cut', 'int64_t n_species', 'int64_t *out_count', 'int32_t *out_images', 'int64_t capacity'],
        'xb_hirshfeld_setup': ['xb_ctx *c', 'const double lattice[9]', 'const double *atoms_cart', 'const int32_t *species', 'int64_t n',
                               'const double *tables', 'const double *r_cut', 'int64_t n_species', 'int64_t knots'],
        'xb_hirshfeld_release': ['xb_ctx *c'],
        'xb_hirshfeld_sum': ['xb_ctx *c', 'double voxel_volume', 'int flags', 'double *charge', 'double *volume', 'double rest[2]',
                             'int64_t stats[3]'],
        'xb_hirshfeld_field': ['xb_ctx *c', 'int mode', 'int flags', 'double *out_host', 'void *out_dev'],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, f'include/bader_hip.h does not declare {name}'
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args, name
        assert _lib.SYMBOLS[name][0] is C.c_int and len(_lib.SYMBOLS[name][1]) == len(args)
    for method in ('hirshfeld_setup', 'hirshfeld_release', 'hirshfeld_sum', 'hirshfeld_field'):
        assert callable(getattr(_lib.Context, method))
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_hirshfeld.h')).read()
    assert 's_cand[XB_HIRSHFELD_CAND_MAX]' in src and '#define HS_TILE %d' % TILE in src
    assert 'NO RESULT DEPENDS ON THE RANGE' in text and 'term = f[s][k] + t*(f[s][k+1] - f[s][k])' in text
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## 19.' in design and 'term = f[s][k] + t*(f[s][k+1] - f[s][k])' in design
    # no timer slot and no option key came with it
    assert _lib.XB_TIMER_COUNT == 11 and not hasattr(_lib, 'XB_TIMER_HIRSHFELD') and not hasattr(_lib, 'XB_OPT_HIRSHFELD')


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.hirshfeld_flag is False and Bader.hirshfeld_field is False and callable(Bader.hirshfeld_analysis)
    assert Bader.proatoms is None and Bader.species is None


def test_hirshfeld_charges_need_the_gpu(lib):
    """without a GPU the calls fail loudly (no fallback); with one they answer"""
    c = case('three')
    if lib.xb_device_count() > 0:
        charge, volume, rest, stats = hirshfeld.hirshfeld_charges(c.rho, c.lattice, c.atoms, c.species, c.pro, 1.0)
        assert charge.shape == volume.shape == (8,) and stats['candidate_tiles'] == 1
        return
    with pytest.raises(_lib.BaderHipError):
        hirshfeld.hirshfeld_charges(c.rho, c.lattice, c.atoms, c.species, c.pro, 1.0)
    with pytest.raises(_lib.BaderHipError):
        hirshfeld.promolecule(c.rho, c.lattice, c.atoms, c.species, c.pro)

"""The stockholder atomic multipoles and radial moments (pybader_amd/stockholder.py, xb_stockholder_moments) restated in plain numpy
from the definition in include/bader_hip.h / DESIGN.md section 25, and what can be said of them without a GPU.
tests/test_gpu_stockmom.py compares the kernel with this restatement: bins and info with ==.

Everything the definition takes from section 19 -- positions, the canonical image list, d2 -- comes from
tests/test_hirshfeld_cpu.py's restatement, the Slater terms from tests/test_mbis_cpu.py's, operation by operation.  `geometry` keeps,
per image of the list, the voxels with d2 < rc2, their e and d2; `bins` is the pass: the setup's own term per pair, P as the running
sum in list order, the twelve integer shares into int64 bins."""
import ctypes as C
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import test_hirshfeld_cpu as hs
import test_isa_cpu as isa_cpu
import test_mbis_cpu as mb
from pybader_amd import _lib, build, stockholder, synth
from pybader_amd.hirshfeld import ProAtoms
from test_hirshfeld_cpu import LATTICES, _positions, candidate_counts, image_list
from test_mbis_cpu import cl2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VV = 0.0371             # a voxel volume that is no power of two
ORDER = (0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 4)
ROWS = 2048 // 12       # the rows of twelve bins that fit the LDS of csrc/k_stockmom.h


@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def exponents(rho_bound, cmax, r_cut_max):
    """(E0 .. E4), with frexp and integers only"""
    lc = int(cmax).bit_length()             # ceil_log2(cmax + 1)
    L = max(0, cl2(float(r_cut_max)))
    return tuple(61 - cl2(float(rho_bound)) - lc - k * L for k in range(5))


class Geometry:
    pass


def geometry(shape, lattice, atoms, species, r_cut, widen=0, prefilter=False):
    """-> Geometry: n, N, images (a list, in the canonical order, of (a, vox int64[], (e0, e1, e2), d2): the voxels with
    d2 < rc2[species[a]], their displacement from THAT image and its square; images that reach no voxel are left out: they add
    nothing), count i64[n].  `prefilter` as test_hirshfeld_cpu.restate's: it only saves time on long thin grids."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(9)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    species = np.asarray(species)
    r_cut = np.asarray(r_cut, dtype=np.float64).reshape(-1)
    n = atoms.shape[0]
    pc = _positions(shape, lat)
    N = pc[0].size
    rc2 = r_cut * r_cut
    if prefilter:
        B = 256
        nb = -(-N // B)
        pad = [np.concatenate([c, np.full(nb * B - N, c[-1])]).reshape(nb, B) for c in pc]
        centre = [c.mean(axis=1) for c in pad]
        radius = np.sqrt(sum((pad[j] - centre[j][:, None]) ** 2 for j in range(3))).max(axis=1)
    g = Geometry()
    g.n, g.N, g.images, g.shape = n, N, [], tuple(shape)
    g.count = np.zeros(n, np.int64)
    for a, x, y, z in image_list(lattice, atoms, species, r_cut, widen):
        s = species[a]
        q = [atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        if prefilter:
            reach = r_cut[s] + radius
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
            g.images.append((int(a), at[inside].astype(np.int64), tuple(ej[inside] for ej in e), d2[inside]))
            g.count[a] += inside.size
    return g


def table_term(pro, species):
    """the term of section 19: the table uniform in r^2"""
    K = pro.knots
    ih2 = np.float64(K) / (pro.r_cut * pro.r_cut)

    def term(a, d2):
        s = species[a]
        u = d2 * ih2[s]
        k = np.minimum(u.astype(np.int64), K - 1)
        t = u - k.astype(np.float64)
        f = pro.tables[s]
        return f[k] + t * (f[k + 1] - f[k])
    return term


def isa_term(A, r_cut):
    """section 23's: the pair (A[a][k], +0.0) through the term of section 19"""
    K = A.shape[1]
    ih2 = np.float64(K) / (r_cut * r_cut)

    def term(a, d2):
        u = d2 * ih2[a]
        k = np.minimum(u.astype(np.int64), K - 1)
        t = u - k.astype(np.float64)
        return A[a][k] + t * np.float64(0.0)
    return term


def mbis_term(tab, shells, N, sigma):
    """section 24's T = ((0 + t_0) + t_1) + ... with r = sqrt(d2)"""
    c, is_ = mb.shell_consts(N, sigma)

    def term(a, d2):
        return mb.terms(tab, np.sqrt(d2), c[a], is_[a], int(shells[a]))[1]
    return term


def shares(s, e, d2, r):
    """the twelve shares of pairs, in the bins' order, each with the index of its exponent"""
    t = [s * e[0], s * e[1], s * e[2]]
    u = s * d2
    return [s, t[0], t[1], t[2], t[0] * e[0], t[0] * e[1], t[0] * e[2], t[1] * e[1], t[1] * e[2], t[2] * e[2], u * r, u * d2]


def bins(g, term, rho, bound, E):
    """the pass -> (bins i64[n, 12], the voxels beyond the bound, P, mag [n, 12] Python ints: the sums of the shares' magnitudes,
    formed in two halves of 31 bits so that they are exact whatever they come to)"""
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    P = np.zeros(g.N)
    Ts = []
    for a, vox, e, d2 in g.images:
        T = term(a, d2)
        Ts.append(T)
        P[vox] = P[vox] + T
    within = np.abs(rho) <= bound
    out, mag = np.zeros((g.n, 12), np.int64), np.zeros((g.n, 12), object)
    for (a, vox, e, d2), T in zip(g.images, Ts):
        Pv, rv = P[vox], rho[vox]
        sel = within[vox] & (Pv > 0) & (T > 0)
        w = T[sel] / Pv[sel]
        s = rv[sel] * w
        dd = d2[sel]
        for c, v in enumerate(shares(s, [x[sel] for x in e], dd, np.sqrt(dd))):
            q = np.rint(np.ldexp(v, E[ORDER[c]])).astype(np.int64)
            out[a, c] += q.sum()
            m = np.abs(q)
            mag[a, c] += (int((m >> 31).sum()) << 31) + int((m & 0x7fffffff).sum())
    return out, int((~within).sum()), P, mag


def bins_scalar(shape, lattice, atoms, species, r_cut, term1, rho, bound, E, images):
    """the same, one voxel and image at a time in Python floats and ints; term1(a, d2) -> T of one pair -> (bins, count)"""
    lat = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = [[float(x) for x in at] for at in np.asarray(atoms, dtype=np.float64).reshape(-1, 3)]
    nx, ny, nz = shape
    rho = np.asarray(rho).reshape(shape)
    out = [[0] * 12 for _ in atoms]
    count = [0] * len(atoms)
    rnd = lambda x: int(np.rint(x))     # (to nearest, ties to even)
    for p0 in range(nx):
        for p1 in range(ny):
            for p2 in range(nz):
                pc = []
                for j in range(3):
                    c = lat[j] * p0 / nx
                    c += lat[3 + j] * p1 / ny
                    c += lat[6 + j] * p2 / nz
                    pc.append(c)
                P, pairs = 0.0, []
                for a, x, y, z in images:
                    rc = float(r_cut[species[a]])
                    e = [pc[j] - (atoms[a][j] + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                    if not d2 < rc * rc:
                        continue
                    count[a] += 1
                    T = term1(a, d2)
                    P += T
                    pairs.append((a, e, d2, T))
                rv = float(rho[p0, p1, p2])
                if not abs(rv) <= bound or not P > 0:
                    continue
                for a, e, d2, T in pairs:
                    if not T > 0:
                        continue
                    w = T / P
                    s = rv * w
                    r = math.sqrt(d2)
                    t = [s * e[0], s * e[1], s * e[2]]
                    u = s * d2
                    vals = [s, t[0], t[1], t[2], t[0] * e[0], t[0] * e[1], t[0] * e[2], t[1] * e[1], t[1] * e[2], t[2] * e[2], u * r, u * d2]
                    for c, v in enumerate(vals):
                        out[a][c] += rnd(math.ldexp(v, E[ORDER[c]]))
    return np.array(out, np.int64), np.array(count, np.int64)


def table_term1(pro, species):
    K = pro.knots

    def term(a, d2):
        s = int(species[a])
        rc = float(pro.r_cut[s])
        u = d2 * (K / (rc * rc))
        k = min(int(u), K - 1)
        f = pro.tables[s]
        return float(f[k]) + (u - k) * (float(f[k + 1]) - float(f[k]))
    return term


def mbis_term1(tab, shells, N, sigma):
    f, d = [float(x) for x in tab.f], [float(x) for x in tab.d]

    def term(a, d2):
        r = math.sqrt(d2)
        T = 0.0
        for i in range(int(shells[a])):
            Nv, sv = float(N[a, i]), float(sigma[a, i])
            q = Nv / (((mb.EIGHT_PI * sv) * sv) * sv)
            c = q if Nv > 0 and math.isfinite(q) else 0.0
            u = (r * (1.0 / sv)) * float(tab.J)
            t = 0.0
            if u < float(tab.KE):
                k = int(u)
                t = c * (f[k] + (u - k) * d[k])
            T += t
        return T
    return term


# ---- inputs (shared with tests/test_gpu_stockmom.py) -------------------------------------------------------------------------------
# name -> (the kind of setup, the case of that kind's own table of inputs, what it is here for)
SETUPS = {
    'hs_cubic': ('hirshfeld', 'cubic_r3', 'a row per atom'),
    'hs_tric': ('hirshfeld', 'tric_r3', 'a row per atom'),
    'hs_odd': ('hirshfeld', 'odd_k1', 'partial tiles (20, 9, 33), K = 1'),
    'hs_three': ('hirshfeld', 'three', '(3, 3, 3)'),
    'hs_thin': ('hirshfeld', 'thin', '(1, 2, 9), an atom outside the cell'),
    'hs_twins': ('hirshfeld', 'twins', 'two atoms of one species, a species nobody takes the first row of'),
    'mbis_one': ('mbis', 'one', '(1, 1, 1)'),
    'isa_one': ('isa', 'one', '(1, 1, 1)'),
    'hs_slots': ('hirshfeld', 'more_candidate', 'grid343 at r_cut 1.0 on 24^3: a row per slot'),
    'hs_rows': ('hirshfeld', 'rows', 'grid343 at r_cut 1.8 on 24^3: more runs in a tile than LDS rows, at most 256 candidates'),
    'hs_overflow': ('hirshfeld', 'more_overflow', 'grid343 at r_cut 3.0 on 16^3: overflow to the full route'),
    'mbis_overflow': ('mbis', 'more_overflow', 'the same on Slater terms'),
    'hs_line': ('hirshfeld', 'line', '(1, 1, 160000): a workgroup takes many tiles'),
    'mbis_negative': ('mbis', 'negative', 'signed shares'),
    'mbis_mixed': ('mbis', 'tric_mixed', 'mixed shell counts'),
    'mbis_thin': ('mbis', 'thin', '(1, 2, 9) on Slater terms'),
    'mbis_table_end': ('mbis', 'table_end', 'most pairs beyond the table: T == 0'),
    'isa_k16': ('isa', 'cubic_r2_k16', 'K = 16, voxels no atom reaches'),
    'isa_three': ('isa', 'three', '(3, 3, 3) on piecewise-constant tables'),
}
LONG = ('hs_line',)
J = 256


def rows_case():
    """grid343 at r_cut 1.8 on 24^3, chosen with candidate_counts: every tile keeps 235 to 249 images, and 175 to 188 atoms reach it"""
    c = hs.Case()
    c.name, c.shape, c.lattice, c.route = 'rows', (24, 24, 24), LATTICES['cubic'], 'candidate'
    a5 = synth.atoms_jittered_grid(7)
    c.atoms = np.ascontiguousarray(a5[:, :3] @ c.lattice)
    c.species = np.zeros(a5.shape[0], np.int32)
    c.pro = hs.bump_proatoms(1.8, 32)
    c.rho = synth.synth_density(c.shape, c.lattice, a5)
    for a in (c.atoms, c.species, c.rho, c.pro.tables, c.pro.r_cut):
        a.flags.writeable = False
    return c


def isa_tables(n, K):
    """tables for the ISA setups: a decaying profile per atom; every other atom's outermost shell is 0 (pairs with T == 0)"""
    A = (1.0 + np.arange(n) % 3)[:, None] * np.exp(-3.0 * np.arange(K) / K)[None, :]
    A[1::2, K - 1] = 0.0
    return np.ascontiguousarray(A)


@functools.lru_cache(maxsize=None)
def setup(name):
    """one input of the GPU tests -- kind, c (the case), shape, lattice, atoms, species, r_cut (per species), rho, bound, term --
    built once, never written"""
    kind, cname, _ = SETUPS[name]
    s = Geometry()
    s.name, s.kind = name, kind
    if kind == 'hirshfeld':
        c = rows_case() if cname == 'rows' else hs.case(cname)
        s.species, s.r_cut = np.asarray(c.species), c.pro.r_cut
        s.term = table_term(c.pro, s.species)
    elif kind == 'isa':
        c = isa_cpu.case(cname)
        n = c.atoms.shape[0]
        s.species, s.r_cut = np.arange(n), c.r_cut
        s.tables = isa_tables(n, c.K)
        s.term = isa_term(s.tables, c.r_cut)
    else:
        c = mb.case(cname)
        s.species, s.r_cut = np.arange(c.atoms.shape[0]), c.r_cut
        s.term = mbis_term(mb.Table(mb.table(), J), c.shells, c.N0, c.s0)
    s.c, s.shape, s.lattice, s.atoms, s.rho = c, c.shape, c.lattice, c.atoms, c.rho
    s.bound = float(np.abs(c.rho).max())
    return s


@functools.lru_cache(maxsize=None)
def geo(name):
    s = setup(name)
    return geometry(s.shape, s.lattice, s.atoms, s.species, s.r_cut, prefilter=name in LONG)


@functools.lru_cache(maxsize=None)
def reference(name, f32=False):
    """(E, bins, the voxels beyond the bound, P, mag) of one input at rho_bound = max |rho|, computed once and never written"""
    s, g = setup(name), geo(name)
    rho = s.rho.astype(np.float32).astype(np.float64) if f32 else s.rho
    bound = float(np.abs(rho).max())
    E = exponents(bound, g.count.max(), s.r_cut.max())
    b, beyond, P, mag = bins(g, s.term, rho, bound, E)
    for a in (b, P):
        a.flags.writeable = False
    return E, b, beyond, P, mag


def moments(E, b, vv=VV):
    """exact scalings"""
    return vv * np.ldexp(b.astype(np.float64), np.array([-E[k] for k in ORDER])[None, :])


# the comparison of tests/test_gpu_stockmom.py (here, so that tests/history_common.py can make it too)
def info_of(g, E, beyond=0):
    """the info of a call on the geometry `g` with the exponents E"""
    return {'E': tuple(E), 'cmax': int(g.count.max()), 'pairs': int(g.count.sum()), 'beyond_bound': beyond}


def want_info(name, E, beyond=0):
    return info_of(geo(name), E, beyond)


CPU_NAMES = [n for n in SETUPS if n not in LONG]


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['hs_three', 'hs_thin', 'mbis_mixed_three', 'mbis_thin'])
def test_restatement_against_a_scalar_triple_loop(name):
    if name == 'mbis_mixed_three':
        c = mb.case('three')
        species, r_cut = np.arange(8), c.r_cut
        tab = mb.Table(mb.table(), J)
        term, term1 = mbis_term(tab, c.shells, c.N0, c.s0), mbis_term1(tab, c.shells, c.N0, c.s0)
        g = geometry(c.shape, c.lattice, c.atoms, species, r_cut)
    else:
        s, g = setup(name), geo(name)
        c, species, r_cut, term = s.c, s.species, s.r_cut, s.term
        if s.kind == 'hirshfeld':
            term1 = table_term1(c.pro, species)
        else:
            term1 = mbis_term1(mb.Table(mb.table(), J), c.shells, c.N0, c.s0)
    rho = np.array(c.rho) * np.where(synth.hash_noise(c.shape, 3) < 0.3, -0.5, 1.0)        # (some negative voxels)
    bound = float(np.abs(rho).max())
    E = exponents(bound, g.count.max(), r_cut.max())
    images = image_list(c.lattice, c.atoms, species, r_cut).tolist()
    b, beyond, P, _ = bins(g, term, rho, bound, E)
    bs, count = bins_scalar(c.shape, c.lattice, c.atoms, species, r_cut, term1, rho, bound, E, images)
    assert np.array_equal(b, bs) and np.array_equal(count, g.count) and beyond == 0, name
    assert (b[:, 0] != 0).any() and (b[:, 10] > 0).any() and (rho < 0).any()
    # a smaller bound: the voxels beyond it add nothing and are counted
    low = float(np.sort(np.abs(rho).reshape(-1))[-3])
    b2, beyond2, _, _ = bins(g, term, rho, low, E)
    bs2, _ = bins_scalar(c.shape, c.lattice, c.atoms, species, r_cut, term1, rho, low, E, images)
    assert np.array_equal(b2, bs2) and beyond2 == int((np.abs(rho) > low).sum()) > 0


def test_the_counts_and_terms_are_those_of_the_three_restatements():
    """count[a] and P of this file's geometry equal what tests/test_hirshfeld_cpu.py, test_isa_cpu.py and test_mbis_cpu.py restate"""
    for name in ('hs_tric', 'hs_thin', 'hs_twins'):
        s, g = setup(name), geo(name)
        P, _ = hs.reference(SETUPS[name][1])
        assert np.array_equal(reference(name)[3].view(np.uint64), P.view(np.uint64)), name
    for name in ('mbis_mixed', 'mbis_thin', 'mbis_negative'):
        s, g = setup(name), geo(name)
        assert np.array_equal(g.count, mb.geo(SETUPS[name][1]).count), name
        P = mb.total(mb.geo(SETUPS[name][1]), mb.Table(mb.table(), J), s.c.shells, s.c.N0, s.c.s0)
        assert np.array_equal(reference(name)[3].view(np.uint64), P.view(np.uint64)), name
    for name in ('isa_k16', 'isa_three'):
        s, g = setup(name), geo(name)
        ig = isa_cpu.geo(SETUPS[name][1])
        assert np.array_equal(g.count, ig.count.sum(axis=1)), name
        assert np.array_equal(reference(name)[3].view(np.uint64), isa_cpu.total(ig, s.tables).view(np.uint64)), name


def test_the_exponents():
    assert exponents(1.0, 0, 1.0) == (61, 61, 61, 61, 61) and exponents(2.0, 1, 3.0) == (59, 57, 55, 53, 51)
    assert exponents(0.5, 3, 0.25) == (60, 60, 60, 60, 60) and exponents(7.5, 13824, 8.0) == (44, 41, 38, 35, 32)
    # cmax shares of magnitude at most rho_bound r_cut^k (1 + 2^-50), each rounded to an integer: below 2^62
    for bound in (1e-300, 0.7, 1.0, 1.5, 7.5, 1e6, 1e300):
        for cmax in (0, 1, 5, 8, 13824, 2 ** 33):
            for rc in (1e-3, 0.5, 1.0, 3.0, 8.0, 1e4):
                E = exponents(bound, cmax, rc)
                for k in range(5):
                    top = math.floor(Fraction(bound) * Fraction(rc) ** k * (1 + Fraction(1, 2 ** 50)) * Fraction(2) ** E[k]) + 1
                    assert max(cmax, 1) * top < 2 ** 62, (bound, cmax, rc, k)


@pytest.mark.parametrize('name', CPU_NAMES)
def test_no_bin_reaches_2_62(name):
    """at rho_bound equal to the exact max |rho|: not the bins, and not the sums of the shares' magnitudes either, so no partial sum
    in any order of the atomics does"""
    E, b, beyond, P, mag = reference(name)
    s, g = setup(name), geo(name)
    assert beyond == 0 and s.bound == float(np.abs(s.rho).max())
    print(f'{name}: E {E}, cmax {int(g.count.max())}, the largest |bin| 2^{math.log2(max(int(np.abs(b).max()), 1)):.2f}, of magnitudes 2^{math.log2(max(int(mag.max()), 1)):.2f}')
    assert int(np.abs(b).max()) < 2 ** 62 and int(mag.max()) < 2 ** 62
    assert all(abs(int(x)) <= int(y) for x, y in zip(b.reshape(-1), mag.reshape(-1)))


# ---- symmetry, exactly ----------------------------------------------------------------------------------------------------------
def symmetric_cell():
    """a cubic cell of side 8.0 on 16^3 -- the spacing 0.5 is exact, so e is exactly antisymmetric about a voxel -- one atom on the
    voxel (8, 8, 8), and a density that is a symmetric function of the three index distances to it: inversion-symmetric through
    the atom, symmetric under the three mirrors and under the permutations of the axes"""
    shape, lat = (16, 16, 16), np.eye(3) * 8.0
    d = np.abs(np.arange(16) - 8)
    d = np.minimum(d, 16 - d).astype(np.float64)
    dx, dy, dz = np.meshgrid(d, d, d, indexing='ij')
    rho = 1.0 / (1.0 + ((dx * dx + dy * dy) + dz * dz)) + 0.125 * (dx * dy) * dz - 0.3
    return shape, lat, np.array([[4.0, 4.0, 4.0]]), np.ascontiguousarray(rho)


@pytest.mark.parametrize('kind', ['table', 'slater'])
def test_exact_cancellation_on_a_symmetric_input(kind):
    shape, lat, atoms, rho = symmetric_cell()
    r_cut = np.array([4.75])            # beyond half the cell: the images at +-8 take part, each its own copy of the atom
    g = geometry(shape, lat, atoms, [0], r_cut)
    per_voxel = np.bincount(np.concatenate([vox for _, vox, _, _ in g.images]), minlength=g.N)
    assert len(g.images) > 1 and per_voxel.max() == 2, 'two images at most reach a voxel: P is a sum of two terms, the same in either order'
    if kind == 'table':
        term = table_term(hs.bump_proatoms(4.75, 64), [0])
    else:
        term = mbis_term(mb.Table(mb.table(), J), [2], np.array([[0.5, 0.5]]), np.array([[0.3, 0.9]]))
    assert (rho < 0).any() and (rho > 0).any()
    bound = float(np.abs(rho).max())
    E = exponents(bound, g.count.max(), 4.75)
    b, beyond, P, _ = bins(g, term, rho, bound, E)
    assert beyond == 0 and b[0, 0] != 0 and b[0, 10] != 0 and b[0, 11] != 0
    assert b[0, 1:4].tolist() == [0, 0, 0], 'the dipole cancels exactly'
    assert b[0, [5, 6, 8]].tolist() == [0, 0, 0], 'the off-diagonal second moments cancel exactly'
    assert b[0, 4] == b[0, 7] == b[0, 9] != 0, 'the diagonal second moments are equal'


@pytest.mark.parametrize('kind', ['table', 'slater'])
def test_translation_by_a_lattice_vector_changes_no_bit(kind):
    shape, lat, _, _ = symmetric_cell()
    atoms = np.array([[4.0, 4.0, 4.0], [2.5, 3.0, 5.5]])
    moved = atoms + np.array([[8.0, 0.0, -8.0], [-8.0, 16.0, 0.0]])
    rho = synth.hash_noise(shape, 5) - 0.25
    r_cut = np.array([4.75, 3.5])
    if kind == 'table':
        pro = ProAtoms(np.concatenate([hs.bump_proatoms(4.75, 64).tables, 2.0 * hs.bump_proatoms(3.5, 64).tables]), r_cut)
        term = table_term(pro, [0, 1])
    else:
        term = mbis_term(mb.Table(mb.table(), J), [2, 1], np.array([[0.5, 0.5], [1.0, 0.0]]), np.array([[0.3, 0.9], [0.5, 1.0]]))
    bound = float(np.abs(rho).max())
    got = []
    for at in (atoms, moved):
        g = geometry(shape, lat, at, [0, 1], r_cut)
        E = exponents(bound, g.count.max(), r_cut.max())
        got.append((E, g.count.tolist(), bins(g, term, rho, bound, E)[0]))
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1] and np.array_equal(got[0][2], got[1][2])
    assert (got[0][2][:, 1:4] != 0).all(), 'and this input cancels nothing'


# ---- the sum rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['hs_cubic', 'hs_thin', 'mbis_mixed', 'mbis_negative', 'isa_k16'])
def test_the_charges_and_the_rest_account_for_the_density(name):
    """BOUND, stated before running, in units of the quantum 2^-E0 of bin 0.  At a voxel within the bound with P > 0 and k pairs with
    T > 0 the shares are rint(2^E0 fl(rho fl(T / P))).  P is the running sum of the pairs' T, so sum T / P = 1 + theta with
    |theta| <= (k - 1) u; each quotient carries one more u, the product with rho another: the shares sum to rho 2^E0 (1 + theta'),
    |theta'| <= (k + 2) u to first order (asserted with a factor 1 + 2^-40).  Each rint moves a share by at most half a quantum.
    Every voxel within the bound is either shared so or belongs to the rest (P == 0).  So, with `pairs` the number of pairs that add,
      |sum_a bins[a][0] - sum_{v: P > 0} rho 2^E0| <= pairs / 2 + sum_v |rho_v| 2^E0 (k_v + 2) u,
    and  sum_a moments[a][0] + rest = sum_v rho vv  within 2^-E0 vv times that, rest = vv sum_{v: P == 0} rho taken exactly, plus the two
    roundings a result carries -- (double)bin and the product with vv -- of u |bin| quanta each."""
    s, g = setup(name), geo(name)
    E, b, beyond, P, _ = reference(name)
    rho = s.rho.reshape(-1)
    k = np.zeros(g.N, np.int64)
    for a, vox, e, d2 in g.images:
        k[vox] += s.term(a, d2) > 0
    have = P > 0
    want = sum(Fraction(float(x)) for x in rho[have]) * Fraction(2) ** E[0]
    lim = Fraction(int(k[have].sum()), 2) + Fraction(float((np.ldexp(np.abs(rho[have]), E[0]) * (k[have] + 2) * 2.0 ** -53).sum() * (1 + 2.0 ** -40)))
    got = int(b[:, 0].sum())
    print(f'{name}: sum bins[:, 0] - sum rho 2^E0 = {float(got - want):.4g} quanta, bound {float(lim):.4g}; {int((~have).sum())} voxels in the rest')
    assert beyond == 0 and abs(got - want) <= lim
    # the same in the results' units
    scaling = 2 * sum(abs(int(x)) for x in b[:, 0]) * Fraction(1, 2 ** 53)
    total = sum(Fraction(float(x)) for x in moments(E, b)[:, 0]) + Fraction(VV) * sum(Fraction(float(x)) for x in rho[~have])
    assert abs(total - Fraction(VV) * sum(Fraction(float(x)) for x in rho)) <= (lim + scaling) * Fraction(VV) / Fraction(2) ** E[0] * (1 + Fraction(1, 2 ** 40))
    if name == 'isa_k16':
        assert (~have).sum() > 0
    if name == 'mbis_negative':
        assert (b[:, 0] < 0).any() and (b[:, 0] > 0).any()


# ---- the free atoms' radial moments ---------------------------------------------------------------------------------------------
def test_radial_moment_of_a_one_segment_table_against_its_closed_form():
    """K = 1: rho0 = f0 (1 - x / R2) in x = r^2 up to R2 = r_cut^2, and with p = (k + 1) / 2
      4 pi int rho0 r^(k+2) dr = 2 pi f0 [R2^(p+1) / (p + 1) - R2^(p+2) / ((p + 2) R2)] = 2 pi f0 r_cut^(k+3) / ((p + 1) (p + 2)):
      k = 0: 8 pi f0 r_cut^3 / 15 (the population);  k = 3: pi f0 r_cut^6 / 6.
    TOLERANCE.  The library forms the two terms of the bracket separately: each a power (1 ulp of the libm), a division, a product
    with f or the slope (itself a division) and their differences with exact zeros: at most 5 roundings, 5 u relative, each.  Their
    difference is 4 / 15 (k = 0) or 1 / 12 (k = 3) of R2^(p+1) where the terms are 2/3, 2/5 or 1/3, 1/4 of it: an amplification of
    (2/3 + 2/5) / (4/15) = 4 or (1/3 + 1/4) / (1/12) = 7.  With the subtraction, the sum over one segment and the factor 2 pi (3 more)
    that is 7 * 5 + 3 = 38 u at most; the closed form on this side carries some 6 u of its own: 48 u."""
    for f0, rc in ((1.0, 1.0), (0.37, 2.5), (11.0, 0.8), (3.3, 3.0)):
        pro = ProAtoms([[f0, 0.0]], [rc])
        for k, want in ((0, 8.0 * math.pi * f0 * rc ** 3 / 15.0), (3, math.pi * f0 * rc ** 6 / 6.0)):
            got = pro.radial_moment(k)
            assert got.shape == (1,) and abs(got[0] - want) <= 48 * 2.0 ** -53 * want, (f0, rc, k, got[0], want)
    # more knots of the same straight line in x give the same integral; two species come back in order
    x = np.arange(9) / 8.0
    pro = ProAtoms([2.0 * (1.0 - x), 1.0 - x], [1.5, 1.5])
    got = pro.radial_moment(3)
    assert got.shape == (2,) and got[0] == pytest.approx(math.pi * 2.0 * 1.5 ** 6 / 6.0, rel=1e-13) and got[1] == pytest.approx(got[0] / 2, rel=1e-13)
    # a Gaussian in r, resolved well by the r^2 spacing: 4 pi int exp(-r^2) r^2 dr = pi^(3/2) up to the tail beyond r_cut = 6
    r = np.linspace(0.0, 6.0, 60001)
    g = ProAtoms.from_radial([(r, np.exp(-r * r))], 6.0, knots=1 << 16)
    assert g.radial_moment(0)[0] == pytest.approx(math.pi ** 1.5, rel=1e-6) and g.radial_moment(2)[0] == pytest.approx(1.5 * math.pi ** 1.5, rel=1e-6)
    with pytest.raises(ValueError):
        pro.radial_moment(-3)


# ---- the results ----------------------------------------------------------------------------------------------------------------
def test_the_results_object_scales_exactly_and_reads_as_multipole_rows():
    E = (40, 38, 36, 34, 32)
    b = np.arange(24, dtype=np.int64).reshape(2, 12) * 1000003 - 7000000
    m = stockholder.StockholderMoments(b, {'E': E, 'cmax': 5, 'pairs': 9, 'beyond_bound': 0}, {}, VV, species=[1, 0])
    want = np.array([[VV * math.ldexp(float(b[a, c]), -E[ORDER[c]]) for c in range(12)] for a in range(2)])
    assert np.array_equal(m.moments.view(np.uint64), want.view(np.uint64)) and np.array_equal(moments(E, b).view(np.uint64), want.view(np.uint64))
    assert np.array_equal(m.charge, want[:, 0]) and np.array_equal(m.dipole, -want[:, 1:4])
    m2 = m.second_moment
    assert m2.shape == (2, 3, 3) and np.array_equal(m2[:, 0, 1], want[:, 5]) and np.array_equal(m2[:, 2, 1], want[:, 8]) and np.array_equal(m2[:, 2, 2], want[:, 9])
    assert np.array_equal(m.r2, (want[:, 4] + want[:, 7]) + want[:, 9]) and np.array_equal(m.r3, want[:, 10]) and np.array_equal(m.r4, want[:, 11])
    q = m.quadrupole
    assert np.allclose(np.trace(q, axis1=1, axis2=2), 0.0, atol=1e-12 * np.abs(want).max())
    assert np.array_equal(m.volume_ratio([2.0, 4.0]), want[:, 10] / np.array([4.0, 2.0]))
    with pytest.raises(ValueError):
        m.volume_ratio([1.0])


def test_the_inputs_of_the_gpu_tests_reach_their_purpose():
    """asserted on the CPU: the inputs of tests/test_gpu_stockmom.py do what they are there for"""
    # hs_rows: every tile answers from a list of at most 256 candidates, and more atoms reach it than rows fit the LDS: each of them
    # has an image among the candidates (phase 1 keeps a superset), so the tile's list has more runs than rows
    s, g = setup('hs_rows'), geo('hs_rows')
    kept = candidate_counts(s.shape, s.lattice, s.atoms, s.species, s.c.pro)
    nt = [-(-x // 8) for x in s.shape]
    pairs = set()
    for a, vox, _, _ in g.images:
        x, y, z = np.unravel_index(vox, s.shape)
        pairs.update((int(t), a) for t in np.unique(((x // 8) * nt[1] + y // 8) * nt[2] + z // 8))
    per_tile = np.bincount([t for t, _ in pairs], minlength=nt[0] * nt[1] * nt[2])
    print(f'hs_rows: the tiles keep {kept.min()} to {kept.max()} images; between {per_tile.min()} and {per_tile.max()} atoms reach a tile')
    assert kept.max() <= _lib.XB_HIRSHFELD_CAND_MAX and per_tile.min() > ROWS and g.n == 343
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_stockmom.h')).read()
    assert '#define SM_LDS_WORDS 2048' in src and '#define SM_BINS 12' in src
    # hs_slots: more atoms than rows, every tile within the rows; hs_overflow: every tile beyond the candidates
    s = setup('hs_slots')
    assert s.atoms.shape[0] > ROWS and candidate_counts(s.shape, s.lattice, s.atoms, s.species, s.c.pro).max() <= ROWS
    for name in ('hs_overflow', 'mbis_overflow'):
        s = setup(name)
        pro = s.c.pro if s.kind == 'hirshfeld' else s.c
        assert candidate_counts(s.shape, s.lattice, s.atoms, s.species, pro).min() > _lib.XB_HIRSHFELD_CAND_MAX
    assert setup('hs_cubic').atoms.shape[0] <= ROWS and hs.n_tiles(setup('hs_line').shape) > 4 * 7 * 256
    assert not (0 <= np.linalg.solve(setup('hs_thin').lattice.T, setup('hs_thin').atoms[2])).all()
    assert setup('mbis_mixed').c.shells.tolist() == mb.MIXED and setup('isa_k16').c.K == 16
    assert (setup('mbis_negative').rho < 0).any() and (reference('mbis_negative')[1][:, 0] < 0).any()
    # T == 0 pairs exist where they are meant to
    for name in ('mbis_table_end', 'isa_k16'):
        s, g = setup(name), geo(name)
        assert sum(int((s.term(a, d2) == 0).sum()) for a, _, _, d2 in g.images) > 0, name


# ---- ABI and refusals -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_stockholder_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_STOCKMOM_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_STOCKMOM_')}
    assert declared == mirrored == {'XB_STOCKMOM_DIRECT': 2}
    assert _lib.XB_STOCKMOM_DIRECT & _lib.XB_HIRSHFELD_FULL_SEARCH == 0
    m = re.search(r'\bint\s+xb_stockholder_moments\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'include/bader_hip.h does not declare xb_stockholder_moments'
    args = ['xb_ctx *c', 'double rho_bound', 'int flags', 'int64_t *bins_out', 'int64_t info[8]', 'int64_t stats[3]']
    assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
    assert _lib.SYMBOLS['xb_stockholder_moments'][0] is C.c_int and len(_lib.SYMBOLS['xb_stockholder_moments'][1]) == len(args)
    assert callable(_lib.Context.stockholder_moments)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for line in ('E_k = 61 - cl2(rho_bound) - cl2(cmax + 1) - k*L', 'w = T / P,  s = rho * w,  r = sqrt(d2),  t_j = s * e[j],  u = s * d2'):
        assert line in text and line in design, line
    assert '## 25.' in design
    assert _lib.XB_TIMER_COUNT == 11 and not hasattr(_lib, 'XB_OPT_STOCKMOM'), 'no timer slot and no option key came with it'
    assert stockholder.ORDER == ORDER


def test_the_library_exports_the_call_and_refuses_a_null_context(lib):
    assert lib.xb_stockholder_moments is not None
    out, info, st = (C.c_int64 * 12)(), (C.c_int64 * 8)(), (C.c_int64 * 3)()
    assert lib.xb_stockholder_moments(None, 1.0, 0, out, info, st) == _lib.XB_E_ARG
    assert lib.xb_stockholder_moments(None, 1.0, 0, None, None, None) == _lib.XB_E_ARG
    assert list(out) == [0] * 12 and list(info) == [0] * 8


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.stockholder_moments_flag is False
    for kind in ('hirshfeld', 'isa', 'mbis'):
        for what in ('moments', 'dipole', 'quadrupole', 'r3', 'r4'):
            assert not hasattr(Bader, f'{kind}_{what}')
    assert not hasattr(Bader, 'hirshfeld_volume_ratio')


def test_the_moments_need_the_gpu(lib):
    """without a GPU the call fails loudly (no fallback); with one it answers"""
    s = setup('hs_three')
    if lib.xb_device_count() > 0:
        m = stockholder.hirshfeld_moments(s.rho, s.lattice, s.atoms, s.species, s.c.pro, VV)
        assert m.moments.shape == (8, 12) and np.array_equal(m.bins, reference('hs_three')[1])
        return
    with pytest.raises(_lib.BaderHipError):
        stockholder.hirshfeld_moments(s.rho, s.lattice, s.atoms, s.species, s.c.pro, VV)

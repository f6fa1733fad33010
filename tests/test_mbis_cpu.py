"""The minimal-basis iterative stockholder atoms (pybader_amd/mbis.py, xb_mbis_setup / xb_mbis_iterate) restated in plain numpy from
the definition in include/bader_hip.h / DESIGN.md section 24, and what can be said of the iteration without a GPU.
tests/test_gpu_mbis.py compares the kernels with this restatement: info, counts, rows, parameters and fields with ==.

Everything the definition takes from section 19 -- positions, the canonical image list, d2 -- comes from
tests/test_hirshfeld_cpu.py's restatement, operation by operation.  `geometry` keeps, per image of the list, the voxels with
d2 < rc2 and r = sqrt(d2); `iterate` is one iteration: the shells' terms from the table, P as the running sum in list order, the
integer shares into int64 bins, the next parameters from the bins."""
import ctypes as C
import functools
import math
import os
import re
import time
import warnings
from fractions import Fraction

import numpy as np
import pytest

from pybader_amd import _lib, build, mbis, synth
from test_hirshfeld_cpu import LATTICES, _positions, candidate_counts, image_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT_PI = 8.0 * math.pi
VV = 0.0371             # a voxel volume that is no power of two


@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def cl2(x):
    """ceil_log2 of a positive float by frexp"""
    m, ex = math.frexp(x)
    return ex - 1 if m == 0.5 else ex


def exponents(rho_bound, cmax, r_cut_max, n_vox):
    """(eN, eS, eV, eR), with frexp and integers only"""
    lc = int(cmax).bit_length()             # ceil_log2(cmax + 1)
    eN = 61 - cl2(float(rho_bound)) - lc
    return eN, eN - max(0, cl2(float(r_cut_max))), 61 - lc, 61 - cl2(float(rho_bound)) - int(n_vox).bit_length()


class Geometry:
    pass


def geometry(shape, lattice, atoms, r_cut, widen=0, prefilter=False):
    """-> Geometry: n, N, images (a list, in the canonical order, of (a, vox int64[], r f64[]): the voxels with d2 < rc2[a] and
    r = sqrt(d2); images that reach no voxel are left out: they add nothing), count i64[n].  `prefilter` as
    test_hirshfeld_cpu.restate's: it only saves time on long thin grids."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(9)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    n = atoms.shape[0]
    r_cut = np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (n,))
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
    g.n, g.N, g.images, g.shape, g.r_cut = n, N, [], tuple(shape), r_cut.copy()
    g.count = np.zeros(n, np.int64)
    for a, x, y, z in image_list(lattice, atoms, np.arange(n), r_cut, widen):
        q = [atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        if prefilter:
            reach = r_cut[a] + radius
            near = np.sqrt(sum((centre[j] - q[j]) ** 2 for j in range(3))) <= reach + 1e-9 * (1.0 + reach)
            if not near.any():
                continue
            at = np.flatnonzero(np.repeat(near, B)[:N])
        else:
            at = np.arange(N)
        e = [pc[j][at] - q[j] for j in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        inside = np.flatnonzero(d2 < rc2[a])
        if inside.size:
            g.images.append((int(a), at[inside].astype(np.int64), np.sqrt(d2[inside])))
            g.count[a] += inside.size
    return g


class Table:
    """the pairs (f[k], d[k]) of a table E[0 .. KE], the differences formed as the library forms them"""

    def __init__(self, E, J):
        E = np.asarray(E, dtype=np.float64)
        self.J, self.KE = int(J), E.size - 1
        self.f, self.d = E[:-1].copy(), E[1:] - E[:-1]


def shell_consts(N, sigma):
    """(c, is) per shell"""
    N, sigma = np.asarray(N, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    den = ((np.float64(EIGHT_PI) * sigma) * sigma) * sigma
    with np.errstate(all='ignore'):
        q = N / den
        c = np.where((N > 0) & np.isfinite(q), q, 0.0)
        return c, np.float64(1.0) / sigma


def terms(tab, r, c, is_, m):
    """the m shells' terms t f64[m, len(r)] of one image and T = ((0 + t_0) + t_1) + ..."""
    t = np.zeros((m, r.size))
    T = np.zeros(r.size)
    for i in range(m):
        with np.errstate(all='ignore'):
            u = (r * is_[i]) * np.float64(tab.J)
        inside = u < np.float64(tab.KE)
        k = u[inside].astype(np.int64)
        w = u[inside] - k.astype(np.float64)
        t[i, inside] = c[i] * (tab.f[k] + w * tab.d[k])
        T = T + t[i]
    return t, T


def total(g, tab, shells, N, sigma):
    """P: the running sum of the images' terms in list order (a voxel occurs at most once per image)"""
    c, is_ = shell_consts(N, sigma)
    P = np.zeros(g.N)
    for a, vox, r in g.images:
        P[vox] = P[vox] + terms(tab, r, c[a], is_[a], int(shells[a]))[1]
    return P


def iterate(g, tab, shells, rho, N, sigma, bound, e, vv=VV):
    """one iteration -> (N', sigma', row = (qsum i64[n], vsum i64[n], (restq, restn)), binN, binS, the voxels beyond the bound, P)"""
    eN, eS, eV, eR = e
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    M = N.shape[1]
    c, is_ = shell_consts(N, sigma)
    P = total(g, tab, shells, N, sigma)
    within = np.abs(rho) <= bound
    binN, binS, binV = np.zeros((g.n, M), np.int64), np.zeros((g.n, M), np.int64), np.zeros(g.n, np.int64)
    for a, vox, r in g.images:
        m = int(shells[a])
        t, T = terms(tab, r, c[a], is_[a], m)
        Pv, rv = P[vox], rho[vox]
        ok = within[vox] & (Pv > 0)
        for i in range(m):
            sel = ok & (t[i] > 0)
            s = rv[sel] * (t[i][sel] / Pv[sel])
            binN[a, i] += np.rint(np.ldexp(s, eN)).astype(np.int64).sum()
            binS[a, i] += np.rint(np.ldexp(r[sel] * s, eS)).astype(np.int64).sum()
        sel = ok & (T > 0)
        binV[a] += np.rint(np.ldexp(T[sel] / Pv[sel], eV)).astype(np.int64).sum()
    none = within & ~(P > 0)
    rest = (int(np.rint(np.ldexp(rho[none], eR)).astype(np.int64).sum()), int(none.sum()))
    N1, s1 = np.zeros_like(N), sigma.copy()
    for a in range(g.n):
        for i in range(M):
            if binN[a, i] > 0:
                raw = math.ldexp(float(binN[a, i]), -eN)
                N1[a, i] = raw * vv
                w = math.ldexp(float(binS[a, i]), -eS) / (3.0 * raw)
                if binS[a, i] > 0 and w > 0 and math.isfinite(w):
                    s1[a, i] = w
    return N1, s1, (binN.sum(axis=1), binV, rest), binN, binS, int((~within).sum()), P


def run(g, tab, shells, rho, N, sigma, bound, e, iters, vv=VV):
    """-> the rows and the parameters after each iteration"""
    rows, pars = [], []
    for _ in range(iters):
        N, sigma, row, _, _, beyond, _ = iterate(g, tab, shells, rho, N, sigma, bound, e, vv)
        assert beyond == 0
        rows.append(row)
        pars.append((N, sigma))
    return rows, pars


def iterate_scalar(shape, lattice, atoms, r_cut, shells, tab, rho, N, sigma, bound, e, images, vv=VV):
    """the same, one voxel, image and shell at a time in Python floats and ints -> (N', sigma', binN, binS, binV, rest, count)"""
    eN, eS, eV, eR = e
    lat = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = [[float(x) for x in at] for at in np.asarray(atoms, dtype=np.float64).reshape(-1, 3)]
    nx, ny, nz = shape
    n, M = len(atoms), N.shape[1]
    rho = np.asarray(rho).reshape(shape)
    f, d = [float(x) for x in tab.f], [float(x) for x in tab.d]
    cs = [[0.0] * M for _ in range(n)]
    iss = [[0.0] * M for _ in range(n)]
    for a in range(n):
        for i in range(int(shells[a])):
            Nv, sv = float(N[a, i]), float(sigma[a, i])
            den = ((EIGHT_PI * sv) * sv) * sv
            q = Nv / den
            cs[a][i] = q if Nv > 0 and math.isfinite(q) else 0.0
            iss[a][i] = 1.0 / sv
    binN = [[0] * M for _ in range(n)]
    binS = [[0] * M for _ in range(n)]
    binV, count, restq, restn = [0] * n, [0] * n, 0, 0
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
                    rc = float(r_cut[a])
                    ee = [pc[j] - (atoms[a][j] + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                    d2 = (ee[0] * ee[0] + ee[1] * ee[1]) + ee[2] * ee[2]
                    if not d2 < rc * rc:
                        continue
                    count[a] += 1
                    r = math.sqrt(d2)
                    ts, T = [], 0.0
                    for i in range(int(shells[a])):
                        u = (r * iss[a][i]) * float(tab.J)
                        t = 0.0
                        if u < float(tab.KE):
                            k = int(u)
                            t = cs[a][i] * (f[k] + (u - k) * d[k])
                        ts.append(t)
                        T += t
                    P += T
                    pairs.append((a, r, ts, T))
                rv = float(rho[p0, p1, p2])
                if not abs(rv) <= bound:
                    continue
                if not P > 0:
                    restq += rnd(math.ldexp(rv, eR))
                    restn += 1
                    continue
                for a, r, ts, T in pairs:
                    for i, t in enumerate(ts):
                        if t > 0:
                            s = rv * (t / P)
                            binN[a][i] += rnd(math.ldexp(s, eN))
                            binS[a][i] += rnd(math.ldexp(r * s, eS))
                    if T > 0:
                        binV[a] += rnd(math.ldexp(T / P, eV))
    N1, s1 = np.zeros_like(N), sigma.copy()
    for a in range(n):
        for i in range(M):
            if binN[a][i] > 0:
                raw = math.ldexp(float(binN[a][i]), -eN)
                N1[a, i] = raw * vv
                w = math.ldexp(float(binS[a][i]), -eS) / (3.0 * raw)
                if binS[a][i] > 0 and w > 0 and math.isfinite(w):
                    s1[a, i] = w
    return N1, s1, np.array(binN, np.int64), np.array(binS, np.int64), np.array(binV, np.int64), (restq, restn), np.array(count, np.int64)


def results(e, row, vv=VV):
    """(charge, volume, rest) of a row: exact scalings"""
    qsum, vsum, rest = row
    return (vv * np.ldexp(qsum.astype(np.float64), -e[0]), vv * np.ldexp(vsum.astype(np.float64), -e[2]),
            np.array([vv * math.ldexp(float(rest[0]), -e[3]), vv * float(rest[1])]))


# the comparison of tests/test_gpu_mbis.py (here, so that tests/history_common.py can make it too)
def same_rows(got, want, what):
    """(qsum, vsum, rest) of a call against the restated rows"""
    q, v, r = got
    assert q.dtype == v.dtype == r.dtype == np.int64 and q.shape[0] == len(want), what
    assert np.array_equal(q, np.array([w[0] for w in want])), f'{what}: qsum'
    assert np.array_equal(v, np.array([w[1] for w in want])), f'{what}: vsum'
    assert np.array_equal(r, np.array([w[2] for w in want], np.int64)), f'{what}: rest'


@functools.lru_cache(maxsize=None)
def table(J=256, x_max=48):
    E = mbis.exp_table(J, x_max)
    E.flags.writeable = False
    return E


# ---- inputs (shared with tests/test_gpu_mbis.py) -------------------------------------------------------------------------------
# name -> (shape, lattice, atoms, r_cut, shells, the route its tiles take)
MIXED = [1, 2, 3, 2, 1, 2, 3, 1]
CASES = {
    'cubic_m1': ((24, 24, 24), 'cubic', 'atoms8', 3.0, 1, 'candidate'),
    'tric_mixed': ((24, 24, 24), 'tric', 'atoms8', 3.0, MIXED, 'candidate'),
    'odd': ((20, 9, 33), 'cubic', 'atoms8', 3.0, 2, 'candidate'),            # partial tiles
    'three': ((3, 3, 3), 'tric', 'atoms8', 3.0, MIXED, 'candidate'),
    'thin': ((1, 2, 9), 'cubic', 'atoms8', 2.0, 1, 'candidate'),            # with an atom outside the cell
    'one': ((1, 1, 1), 'tric', 'atoms8', 3.0, 2, 'candidate'),
    'more_overflow': ((16, 16, 16), 'cubic', 'grid343', 3.0, 1, 'overflow'),      # more than 256 candidates: the full route
    'more_slots': ((24, 24, 24), 'cubic', 'grid343', 1.0, 1, 'candidate'),        # 343 atoms: a row of bins per slot of the list
    'more_slots_m8': ((24, 24, 24), 'cubic', 'grid343', 1.5, 8, 'candidate'),     # ... and more runs in a tile than rows fit in LDS
    'line': ((1, 1, 160000), 'cubic', 'atoms8', 2.2, 2, 'candidate'),             # a workgroup takes many tiles
    'negative': ((24, 24, 24), 'tric', 'atoms8', 3.0, 2, 'candidate'),
    'table_end': ((24, 24, 24), 'cubic', 'atoms8', 3.0, 1, 'candidate'),
}
LONG = ('line',)


@functools.lru_cache(maxsize=None)
def case(name):
    """one input of the GPU tests: shape, lattice, atoms (Cartesian), r_cut, shells, the start, rho, bound -- built once, never written"""
    shape, lname, kind, r_cut, shells, route = CASES[name]
    c = Geometry()
    c.name, c.shape, c.lattice, c.route = name, shape, LATTICES[lname], route
    if kind == 'grid343':
        a5 = synth.atoms_jittered_grid(7)
        c.rho = synth.synth_density(shape, c.lattice, a5)
    else:
        a5 = synth.ATOMS8
        c.rho = synth.synth_density(shape, c.lattice, a5) - synth.BACKGROUND
    c.atoms = np.ascontiguousarray(a5[:, :3] @ c.lattice)
    n = c.atoms.shape[0]
    if name == 'thin':
        c.atoms = c.atoms.copy()
        c.atoms[2] += c.lattice[0] - 2 * c.lattice[2]      # an atom outside the cell: taken as given
    if name == 'negative':
        # the density times -1 within 1.2 A of atom 6 (the nearest image): both of its shells sum below zero, die and stay dead
        lat9 = c.lattice.reshape(9)
        pc = _positions(shape, lat9)
        near = np.zeros(c.rho.size, bool)
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                for z in (-1, 0, 1):
                    q = c.atoms[6] + x * c.lattice[0] + y * c.lattice[1] + z * c.lattice[2]
                    near |= sum((pc[j] - q[j]) ** 2 for j in range(3)) < 1.2 ** 2
        c.rho = np.ascontiguousarray(np.where(near.reshape(shape), -c.rho, c.rho))
    c.r_cut = np.full(n, float(r_cut))
    c.shells = np.broadcast_to(np.asarray(shells if np.ndim(shells) == 0 else (list(shells) * n)[:n], np.int32), (n,)).copy()
    if name == 'more_slots_m8':
        c.shells = (1 + np.arange(n) % 8).astype(np.int32)
    c.N0, c.s0 = mbis.default_initial(c.shells)
    if name == 'table_end':
        c.s0 = np.full_like(c.s0, 0.02)                    # the table ends at r = 48 sigma = 0.96 A: most pairs lie beyond it
    c.bound = float(np.abs(c.rho).max())
    for a in (c.atoms, c.rho, c.r_cut, c.shells, c.N0, c.s0):
        a.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def geo(name):
    c = case(name)
    return geometry(c.shape, c.lattice, c.atoms, c.r_cut, prefilter=name in LONG)


def case_exponents(name):
    c, g = case(name), geo(name)
    return exponents(c.bound, g.count.max(), c.r_cut.max(), g.N)


@functools.lru_cache(maxsize=None)
def reference(name, iters=7):
    """(e, the rows, the parameters after each iteration) of one input, computed once and never written"""
    c, g = case(name), geo(name)
    e = case_exponents(name)
    rows, pars = run(g, Table(table(), 256), c.shells, c.rho, c.N0, c.s0, c.bound, e, iters)
    return e, rows, pars


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', ['cubic', 'tric'])
def test_restatement_against_a_scalar_triple_loop(lname):
    shape, lat = (5, 7, 11), LATTICES[lname]
    atoms = synth.ATOMS8[:, :3] @ lat
    r_cut = np.array([2.5, 2.0, 3.0, 1.5, 2.5, 2.2, 1.0, 2.8])
    shells = np.array(MIXED)
    rho = synth.synth_density(shape, lat, synth.ATOMS8) - synth.BACKGROUND
    rho = rho * np.where(synth.hash_noise(shape, 3) < 0.1, -0.5, 1.0)        # (some negative voxels)
    tab = Table(mbis.exp_table(16, 6), 16)                                  # (a short, coarse table: its end is reached)
    g = geometry(shape, lat, atoms, r_cut)
    bound = float(np.abs(rho).max())
    e = exponents(bound, g.count.max(), r_cut.max(), g.N)
    images = image_list(lat, atoms, np.arange(8), r_cut).tolist()
    N, sigma = mbis.default_initial(shells)
    beyond_table = 0
    for it in range(3):
        N1, s1, row, binN, binS, beyond, P = iterate(g, tab, shells, rho, N, sigma, bound, e)
        got = iterate_scalar(shape, lat, atoms, r_cut, shells, tab, rho, N, sigma, bound, e, images)
        assert np.array_equal(g.count, got[6]) and np.array_equal(binN, got[2]) and np.array_equal(binS, got[3]), (lname, it)
        assert np.array_equal(row[1], got[4]) and row[2] == got[5] and beyond == 0, (lname, it)
        assert np.array_equal(N1.view(np.uint64), got[0].view(np.uint64)) and np.array_equal(s1.view(np.uint64), got[1].view(np.uint64)), (lname, it)
        assert np.array_equal(row[0], binN.sum(axis=1))
        beyond_table += sum(int(((r / sigma[a, 0]) * 16 >= tab.KE).sum()) for a, _, r in g.images)
        N, sigma = N1, s1
    assert (g.count > 0).all() and (N > 0).any() and beyond_table > 0


@pytest.mark.parametrize('name', ['cubic_m1', 'tric_mixed', 'thin', 'three'])
def test_counts_against_a_brute_force_over_a_wider_image_range(name):
    """every (voxel, image) pair over a range three shifts wider at either end, one dense d2 matrix: the same counts"""
    c, g = case(name), geo(name)
    lat = np.asarray(c.lattice, dtype=np.float64).reshape(9)
    pc = _positions(c.shape, lat)
    n = c.atoms.shape[0]
    wide = image_list(c.lattice, c.atoms, np.arange(n), c.r_cut, widen=3)
    assert wide.shape[0] > 3 * image_list(c.lattice, c.atoms, np.arange(n), c.r_cut).shape[0]
    count = np.zeros_like(g.count)
    for a, x, y, z in wide:
        q = [c.atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        e = [pc[j] - q[j] for j in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        count[a] += int((d2 < c.r_cut[a] * c.r_cut[a]).sum())
    assert np.array_equal(count, g.count) and count.sum() > 0
    assert np.array_equal(geometry(c.shape, c.lattice, c.atoms, c.r_cut, widen=2).count, g.count)


def test_the_exponents_against_exact_integers_and_the_bound_of_2_62():
    for p in list(range(-1074, -1060)) + list(range(-70, 70)) + list(range(1010, 1024)):
        x = math.ldexp(1.0, p)
        for v in (x, float(np.nextafter(x, 0.0)), float(np.nextafter(x, np.inf))):
            if v > 0 and math.isfinite(v):
                assert Fraction(2) ** (cl2(v) - 1) < Fraction(v) <= Fraction(2) ** cl2(v), (p, v)
    # no bin can reach 2^62: cmax pairs (N_vox voxels for the rest) of at most rint(x 2^e) each, x the largest share of its kind:
    # rho_bound for binN and the rest, rho_bound r_cut for binS (r < r_cut), 1 for binV; qsum sums a pair's shells, whose shares
    # sum to rho T / P <= rho_bound up to m + 2 roundings: the factor 1 + 2^-40 and a quantum per shell cover them
    for bound in (1e-300, 0.7, 1.0, 1.5, 7.5, 1e6, 1e300):
        for cmax in (0, 1, 5, 8, 13824, 2 ** 33):
            for rc in (1e-3, 0.5, 1.0, 3.0, 8.0, 1e4):
                for n_vox in (1, 13824, 2 ** 27, 2 ** 40):
                    eN, eS, eV, eR = exponents(bound, cmax, rc, n_vox)
                    top = lambda x, e: math.floor(Fraction(x) * Fraction(2) ** e) + 1
                    assert max(cmax, 1) * top(bound, eN) < 2 ** 62
                    assert max(cmax, 1) * (top(bound * (1 + 2.0 ** -40), eN) + 8) < 2 ** 62
                    assert max(cmax, 1) * top(Fraction(bound) * Fraction(rc), eS) < 2 ** 62
                    assert max(cmax, 1) * top(1.0, eV) < 2 ** 62
                    assert n_vox * top(bound, eR) < 2 ** 62
    assert exponents(1.0, 0, 1.0, 1) == (61, 61, 61, 60) and exponents(2.0, 1, 3.0, 7) == (59, 57, 60, 57)
    assert exponents(0.5, 3, 0.25, 8) == (60, 60, 59, 58)


@pytest.mark.parametrize('name', ['cubic_m1', 'tric_mixed'])
def test_the_sums_account_for_every_voxel(name):
    """BOUND, stated before running.  At a voxel with P > 0 and k (pair, shell) terms > 0 over m pairs the shares are
    rint(rho 2^eN fl(t / P)).  P is the running sum of the pairs' T, each T the running sum of its shells: relative error at most
    (k - 1) u; each quotient one more u, the product with rho another: the shares sum to rho 2^eN (1 + theta), |theta| <= (k + 2) u
    (to first order; asserted with a factor 1 + 2^-40).  Each rint moves a share by at most half a quantum.  Every voxel within the
    bound is either shared so or goes to the rest.  So
      |sum_a qsum[a] - sum_{v: P > 0} rho 2^eN| <= sum_v [ k_v / 2 + |rho_v| 2^eN (k_v + 2) u ]   and   restn + #{v: P > 0} = N_vox."""
    c, g = case(name), geo(name)
    e, rows, pars = reference(name, 7)
    tab = Table(table(), 256)
    rho = c.rho.reshape(-1)
    N, sigma = c.N0, c.s0
    for it in range(3):
        cs, is_ = shell_consts(N, sigma)
        k = np.zeros(g.N, np.int64)
        for a, vox, r in g.images:
            k[vox] += (terms(tab, r, cs[a], is_[a], int(c.shells[a]))[0] > 0).sum(axis=0)
        P = total(g, tab, c.shells, N, sigma)
        have = P > 0
        qsum, vsum, rest = rows[it]
        want = sum(Fraction(float(x)) for x in rho[have]) * Fraction(2) ** e[0]
        lim = Fraction(int(k[have].sum()), 2) + Fraction(float((np.ldexp(np.abs(rho[have]), e[0]) * (k[have] + 2) * 2.0 ** -53).sum() * (1 + 2.0 ** -40)))
        got = int(qsum.sum())
        print(f'{name} iteration {it}: sum qsum - sum rho 2^eN = {float(got - want):.4g}, bound {float(lim):.4g}')
        assert abs(got - want) <= lim and rest[1] + int(have.sum()) == g.N
        assert rest[0] == int(np.rint(np.ldexp(rho[~have], e[3])).astype(np.int64).sum())
        N, sigma = pars[it]


# ---- what the method does -------------------------------------------------------------------------------------------------------
def converge(g, tab, shells, rho, N, sigma, bound, e, vv, tol=1e-6, max_iter=500):
    last, it = None, 0
    while it < max_iter:
        N, sigma, row, _, _, _, _ = iterate(g, tab, shells, rho, N, sigma, bound, e, vv)
        it += 1
        charge = results(e, row, vv)[0]
        if last is not None and np.max(np.abs(charge - last)) < tol:
            return N, sigma, charge, it, True
        last = charge
    return N, sigma, last, it, False


MEASURED_SYNTH_DISTANCE = 1.70e-2     # measured on the CPU (the numpy restatement), see the test below
MEASURED_SYNTH_ITERATIONS = 9


def test_convergence_on_the_synth_input_and_the_distance_to_the_atoms_own_integrals():
    """synth_density(24^3) - BACKGROUND in the cubic cell is the sum of eight overlapping atoms A g(r^2), each with the known integral
    A pi^(3/2) R^3 Gamma(1025) / Gamma(1026.5), R^2 = 2048 s^2.  MBIS with one shell and r_cut = 3 converges to tol = 1e-6 well within
    max_iter (ISA needs 286 iterations on this input, tests/test_isa_cpu.py).  How far its charges lie from the atoms' own integrals
    follows from no bound: the atoms are Gaussians, the model is exponential.  MEASURED ON THE CPU (numpy restatement, 9 iterations):
    max_a |q_a - integral_a| = 1.70e-2 of charges between 1.16 and 13.28 (atom 5); asserted at TWICE the measured value."""
    name = 'cubic_m1'
    c, g = case(name), geo(name)
    vv = abs(np.linalg.det(c.lattice)) / g.N
    e = case_exponents(name)
    N, sigma, charge, it, ok = converge(g, Table(table(), 256), c.shells, c.rho, c.N0, c.s0, c.bound, e, vv)
    exact = np.array([amp * math.pi ** 1.5 * (2048 * sg * sg) ** 1.5 * math.exp(math.lgamma(1025) - math.lgamma(1026.5))
                      for _, _, _, sg, amp in synth.ATOMS8])
    dist = np.abs(charge - exact)
    print(f'{name}: {it} iterations; MBIS {charge.round(5).tolist()}; integrals {exact.round(5).tolist()}; max distance {dist.max():.4e}')
    assert ok and it <= 4 * MEASURED_SYNTH_ITERATIONS
    assert dist.max() <= 2 * MEASURED_SYNTH_DISTANCE
    # the charges are the populations: N' = raw vv, summed over the shells, is the charge up to the roundings of the scaling
    assert np.allclose(N.sum(axis=1), charge, rtol=1e-12, atol=0)


def slater_density(shape, lattice, atoms, N, sigma, reach=2):
    """sum over atoms and their images within `reach` cells of N / (8 pi sigma^3) exp(-r / sigma)"""
    lat9 = np.asarray(lattice, dtype=np.float64).reshape(9)
    pc = _positions(shape, lat9)
    rho = np.zeros(pc[0].size)
    rng = range(-reach, reach + 1)
    for at, Nv, sv in zip(atoms, N, sigma):
        for x in rng:
            for y in rng:
                for z in rng:
                    q = at + x * lattice[0] + y * lattice[1] + z * lattice[2]
                    r = np.sqrt(sum((pc[j] - q[j]) ** 2 for j in range(3)))
                    rho += Nv / (8.0 * math.pi * sv ** 3) * np.exp(-r / sv)
    return rho.reshape(shape)


MEASURED_SLATER_DISTANCE = 8.19e-2    # measured on the CPU (the numpy restatement), see the test below


def test_slater_atoms_are_recovered_with_a_wide_cutoff():
    """A density that IS a sum of Slater atoms (sigma from 0.25 to 0.5 A, the populations of synth.ATOMS8) on 24^3 in the cubic cell,
    fitted with one shell per atom and r_cut = 6 A: the fixed point of the iteration on the continuum is the atoms themselves; what
    remains is the 0.25 A grid under a cusp and the truncation at r_cut.  (A 32^3 triclinic input with r_cut = 8 A has about 2.7
    million pairs and would take this restatement well over 20 s; this smaller input stands in.)  MEASURED ON THE CPU (numpy
    restatement, 198 iterations): max_a |N_a - N*_a| = 8.19e-2 of populations between 1.17 and 13.26 (sigma within 5.5e-3 A, the
    tail beyond the cutoff 4.7e-4); asserted at TWICE the measured value."""
    shape, lat = (24, 24, 24), synth.CUBIC6
    atoms = np.ascontiguousarray(synth.ATOMS8[:, :3] @ lat)
    want_N = synth.ATOMS8[:, 4].copy()
    want_s = np.linspace(0.25, 0.5, 8)
    rho = slater_density(shape, lat, atoms, want_N, want_s)
    start = time.time()
    g = geometry(shape, lat, atoms, 6.0)
    vv = abs(np.linalg.det(lat)) / g.N
    bound = float(np.abs(rho).max())
    e = exponents(bound, g.count.max(), 6.0, g.N)
    shells = np.ones(8, np.int32)
    N0, s0 = mbis.default_initial(shells)
    N, sigma, charge, it, ok = converge(g, Table(table(), 256), shells, rho, N0, s0, bound, e, vv)
    dist = np.abs(N[:, 0] - want_N)
    lost = mbis.tail(N, sigma, np.full(8, 6.0))
    print(f'slater 24^3 r_cut 6: {it} iterations in {time.time() - start:.1f} s; N {N[:, 0].round(4).tolist()}; sigma {sigma[:, 0].round(4).tolist()}; '
          f'max |N - N*| {dist.max():.4e}; max |sigma - sigma*| {np.abs(sigma[:, 0] - want_s).max():.4e}; tail {lost.max():.3e}')
    assert ok
    assert dist.max() <= 2 * MEASURED_SLATER_DISTANCE


def test_tail_against_its_closed_form():
    """the share of N / (8 pi s^3) exp(-r / s) beyond R is e^-x (1 + x + x^2 / 2), x = R / s: against a fine radial quadrature and the
    limits"""
    N = np.array([[2.0, 6.0], [1.5, 0.0], [0.0, 0.0]])
    sg = np.array([[0.1, 0.7], [0.45, 1.0], [1.0, 1.0]])
    rc = np.array([3.0, 2.0, 5.0])
    got = mbis.tail(N, sg, rc)
    for a in range(2):
        lost = 0.0
        for i in range(2):
            x = rc[a] / sg[a, i]
            lost += N[a, i] * math.exp(-x) * (1 + x + x * x / 2)
            # the quadrature of 4 pi r^2 rho0 from R to R + 60 s, by the midpoint rule
            r = rc[a] + (np.arange(400000) + 0.5) * (60 * sg[a, i] / 400000)
            quad = float((4 * math.pi * r * r * N[a, i] / (8 * math.pi * sg[a, i] ** 3) * np.exp(-r / sg[a, i])).sum() * (60 * sg[a, i] / 400000))
            assert abs(quad - N[a, i] * math.exp(-x) * (1 + x + x * x / 2)) <= 1e-9 * max(N[a, i], 1e-300)
        assert got[a] == pytest.approx(lost / N[a].sum(), rel=1e-14)
    assert got[2] == 0.0 and mbis.tail([[1.0]], [[1.0]], [0.0])[0] == 1.0
    assert mbis.tail([[1.0]], [[0.5]], [3.0])[0] == pytest.approx(math.exp(-6.0) * 25.0, rel=1e-14)


def test_the_starts():
    N, sg = mbis.default_initial([1, 3, 2])
    assert np.array_equal(N, [[1, 0, 0], [1 / 3, 1 / 3, 1 / 3], [0.5, 0.5, 0]]) and np.array_equal(sg, [[0.2, 1, 1], [0.2, 0.4, 0.8], [0.2, 0.4, 1]])
    sh, N, sg = mbis.initial_from_numbers([1, 8, 14, 26])
    assert sh.tolist() == [1, 2, 3, 4] and N.shape == sg.shape == (4, 4)
    assert np.allclose(N.sum(axis=1), [1, 8, 14, 26], rtol=1e-15) and np.allclose(N[1, :2], [1.6, 6.4]) and np.allclose(N[3], np.array([2, 8, 8, 18]) * 26 / 36)
    alpha = mbis.BOHR / sg
    assert alpha[0, 0] == pytest.approx(2.0) and np.allclose(alpha[1, :2], [16.0, 2.0]) and np.allclose(alpha[2, :3], [28.0, math.sqrt(56.0), 2.0])
    assert np.allclose(alpha[3, 1:] / alpha[3, :-1], (1 / 26) ** (1 / 3))
    with pytest.raises(ValueError):
        mbis.initial_from_numbers([0])
    E = mbis.exp_table(4, 3)
    assert E.shape == (13,) and E[0] == 1.0 and E[12] == 0.0 and E[4] == np.exp(-1.0) and (np.diff(E) < 0).all()
    assert mbis.exp_table().nbytes == 8 * (48 * 256 + 1)


def test_the_inputs_of_the_gpu_tests_reach_their_purpose():
    """asserted on the restatement: the inputs of tests/test_gpu_mbis.py do what they are there for"""
    tab = Table(table(), 256)
    # negative: both shells of atom 6 die after iteration 1 and stay dead; every other shell lives
    e, rows, pars = reference('negative')
    assert case('negative').shells[6] == 2 and (case('negative').rho < 0).any()
    for N, _ in pars:
        assert (N[6] == 0).all() and (np.delete(N, 6, axis=0) > 0).all()
    # table_end: at the start most pairs lie beyond the table and many voxels have P == 0; it recovers from iteration 2
    c, g = case('table_end'), geo('table_end')
    beyond = sum(int(((r / 0.02) * 256 >= tab.KE).sum()) for _, _, r in g.images)
    e, rows, pars = reference('table_end')
    empty = [row[2][1] for row in rows]
    print(f'table_end: {beyond} of {int(g.count.sum())} pairs beyond the table, voxels with P == 0 per iteration {empty}')
    assert beyond > 0.9 * g.count.sum() and empty[0] > 0.5 * g.N and all(x < empty[0] // 4 for x in empty[2:]) and empty[2:] == [empty[2]] * 5
    # more_slots_m8: some tile is reached by more atoms than the 120 rows of 17 bins that fit the LDS of csrc/k_mbis.h
    for name, rows_cap in (('more_slots', 256), ('more_slots_m8', 2048 // 17)):
        c, g = case(name), geo(name)
        assert g.n == 343 and g.n > rows_cap
        nt = [-(-s // 8) for s in c.shape]
        pairs = set()
        for a, vox, _ in g.images:
            x, y, z = np.unravel_index(vox, c.shape)
            pairs.update((int(t), a) for t in np.unique(((x // 8) * nt[1] + y // 8) * nt[2] + z // 8))
        per_tile = np.bincount([t for t, _ in pairs], minlength=nt[0] * nt[1] * nt[2])
        print(f'{name}: between {per_tile.min()} and {per_tile.max()} atoms reach a tile')
        assert (per_tile.min() > rows_cap) == (name == 'more_slots_m8') and (per_tile.max() > rows_cap) == (name == 'more_slots_m8')
        kept = candidate_counts(c.shape, c.lattice, c.atoms, np.arange(g.n), c)      # (c.r_cut: one cutoff per atom)
        assert kept.max() <= _lib.XB_HIRSHFELD_CAND_MAX, 'and every tile answers from its candidate list'
    assert case('more_slots_m8').shells.max() == 8 and case('tric_mixed').shells.tolist() == MIXED
    assert not (0 <= np.linalg.solve(case('thin').lattice.T, case('thin').atoms[2])).all()
    assert -(-160000 // 8) > 4 * 7 * 256, 'more tiles on the line than any launch has workgroups'
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_mbis.h')).read()
    assert '#define MBIS_LDS_WORDS 2048' in src


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_mbis_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_MBIS_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_MBIS_')}
    assert declared == mirrored == {'XB_MBIS_DIRECT': 2, 'XB_MBIS_KEEP': 4, 'XB_MBIS_ITERS_MAX': 64, 'XB_MBIS_SHELLS_MAX': 8}
    assert _lib.XB_MBIS_DIRECT & _lib.XB_HIRSHFELD_FULL_SEARCH == 0 and _lib.XB_MBIS_KEEP & (_lib.XB_MBIS_DIRECT | _lib.XB_HIRSHFELD_FULL_SEARCH) == 0
    want = {
        'xb_mbis_setup': ['xb_ctx *c', 'const double lattice[9]', 'const double *atoms_cart', 'int64_t n', 'const double *r_cut',
                          'const int32_t *shells', 'const double *etable', 'int64_t J', 'int64_t KE', 'const double *init_N',
                          'const double *init_sigma', 'double rho_bound', 'double voxel_volume', 'int64_t out_info[6]'],
        'xb_mbis_iterate': ['xb_ctx *c', 'int64_t iters', 'int flags', 'int64_t *qsum_out', 'int64_t *vsum_out', 'int64_t *rest_out',
                            'int64_t stats[4]'],
        'xb_mbis_params': ['xb_ctx *c', 'double *N_out', 'double *sigma_out', 'int64_t *count_out'],
        'xb_mbis_load': ['xb_ctx *c', 'const double *N', 'const double *sigma'],
        'xb_mbis_field': ['xb_ctx *c', 'int mode', 'int flags', 'double *out_host', 'void *out_dev'],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, f'include/bader_hip.h does not declare {name}'
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args, name
        assert _lib.SYMBOLS[name][0] is C.c_int and len(_lib.SYMBOLS[name][1]) == len(args)
    for method in ('mbis_setup', 'mbis_iterate', 'mbis_params', 'mbis_load', 'mbis_field'):
        assert callable(getattr(_lib.Context, method))
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for line in ('eN = 61 - cl2(rho_bound) - cl2(cmax + 1)', 't_i = c_i*(f[k] + w*d[k])', 'correctly rounded'):
        assert line in text and line in design, line
    assert '## 24.' in design
    assert _lib.XB_TIMER_COUNT == 11, 'no timer slot came with it'


def test_the_library_exports_the_calls(lib):
    for name in ('xb_mbis_setup', 'xb_mbis_iterate', 'xb_mbis_params', 'xb_mbis_load', 'xb_mbis_field'):
        assert getattr(lib, name) is not None
    # a null context is an argument error in all five, found before anything else
    assert lib.xb_mbis_setup(None, None, None, 1, None, None, None, 1, 1, None, None, 1.0, 1.0, None) == _lib.XB_E_ARG
    assert lib.xb_mbis_iterate(None, 1, 0, None, None, None, None) == _lib.XB_E_ARG
    assert lib.xb_mbis_params(None, None, None, None) == _lib.XB_E_ARG
    assert lib.xb_mbis_load(None, None, None) == _lib.XB_E_ARG
    assert lib.xb_mbis_field(None, 0, 0, None, None) == _lib.XB_E_ARG


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.mbis_flag is False and callable(Bader.mbis_analysis)
    assert Bader.mbis_shells == 1 and Bader.mbis_r_cut == 5.0 and Bader.mbis_tol == 1e-6


def test_mbis_charges_need_the_gpu(lib):
    """without a GPU the call fails loudly (no fallback); with one it answers"""
    c = case('three')
    if lib.xb_device_count() > 0:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            r = mbis.mbis_charges(c.rho, c.lattice, c.atoms, 1.0, shells=c.shells, r_cut=3.0, max_iter=3, tol=0.0)
        assert r.charge.shape == (8,) and r.iterations == 3
        return
    with pytest.raises(_lib.BaderHipError):
        mbis.mbis_charges(c.rho, c.lattice, c.atoms, 1.0, shells=c.shells, r_cut=3.0, max_iter=3)

"""The host side of IGM (pybader_amd/igm.py) and the plain numpy restatement of the definition in include/bader_hip.h / DESIGN.md
section 27 that tests/test_gpu_igm.py compares the kernels with: both fields with ==.

`restate` is elementwise IEEE float64 in the order the definition writes, one image of the canonical list at a time over all
voxels: P, gP, p_a and gp_a are running sums in list order, the atoms are closed ascending.  An image beyond its cutoff is not
added at all (its voxels are left out by index), as the definition says.  `restate_scalar` does the same one voxel and one image
at a time in Python floats.  The gradient of the density is tests/test_laplacian_cpu.py's restatement of section 18.

The inputs are those of tests/test_hirshfeld_cpu.py (`case`), shared and never written."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import test_hirshfeld_cpu as HS
from pybader_amd import _lib, build, igm
from pybader_amd.hirshfeld import ProAtoms
from pybader_amd.interface import Bader
from test_laplacian_cpu import grouped, restated_values, sum_bound
from test_multipole_cpu import VV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
PRO, STOCK = _lib.XB_IGM_PRO, _lib.XB_IGM_STOCKHOLDER
MODES = {'pro': PRO, 'stockholder': STOCK}
P_MIN = 1e-6


@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def nrm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def table_sums(shape, lattice, atoms, species, pro, widen=0, flat=False):
    """the pass over the canonical image list, which no fragment, mode or floor enters -> dict: P f64[N], gP f64[3, N], pa f64[n, N],
    gpa f64[n, 3, N] (the running sums), S f64[3, N] (the sum of |G| over all images), cnt int[N] (the images within their cutoff).
    `flat`: the tables are an ISA setup's, piecewise constant: the pair of knot k is (f[k], +0.0)"""
    lat = np.asarray(lattice, dtype=np.float64).reshape(9)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    n, K = atoms.shape[0], pro.knots
    pc = HS._positions(shape, lat)
    N = pc[0].size
    rc2 = pro.r_cut * pro.r_cut
    ih2 = np.float64(K) / rc2
    P, gP, S, cnt = np.zeros(N), np.zeros((3, N)), np.zeros((3, N)), np.zeros(N, np.int64)
    pa, gpa = np.zeros((n, N)), np.zeros((n, 3, N))
    for a, x, y, z in HS.image_list(lattice, atoms, species, pro.r_cut, widen):
        s = species[a]
        q = [atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        e = [pc[j] - q[j] for j in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        at = np.flatnonzero(d2 < rc2[s])
        if not at.size:
            continue
        u = d2[at] * ih2[s]
        k = np.minimum(u.astype(np.int64), K - 1)
        t = u - k.astype(np.float64)
        f = pro.tables[s]
        df = np.zeros(at.size) if flat else f[k + 1] - f[k]
        T = f[k] + t * df
        sl = df * ih2[s]
        c = sl + sl
        P[at] = P[at] + T
        pa[a, at] = pa[a, at] + T
        cnt[at] += 1
        for j in range(3):
            G = c * e[j][at]
            gP[j, at] = gP[j, at] + G
            gpa[a, j, at] = gpa[a, j, at] + G
            S[j, at] = S[j, at] + np.abs(G)
    return {'P': P, 'gP': gP, 'pa': pa, 'gpa': gpa, 'S': S, 'cnt': cnt}


def restate(shape, lattice, atoms, species, pro, rho, fragment, mode, p_min=P_MIN, widen=0, flat=False, sums=None):
    """-> dict: dg, dgi f64[N] (the fields), and what the property tests need: P, reached, g, gI f64[3, N], S, cnt (table_sums'),
    gr, rho, iP.  `sums`: table_sums of the same input, made before"""
    fragment = np.asarray(fragment, dtype=np.int64).reshape(-1)
    n = fragment.shape[0]
    F = max(int(fragment.max()) + 1, 1)
    t = table_sums(shape, lattice, atoms, species, pro, widen, flat) if sums is None else sums
    P, gP, pa, gpa, S, cnt = (t[k] for k in ('P', 'gP', 'pa', 'gpa', 'S', 'cnt'))
    N = P.size
    reached = P > p_min
    r = np.asarray(rho, dtype=np.float64).reshape(-1)
    gr = restated_values(np.asarray(rho, dtype=np.float64).reshape(shape), np.asarray(lattice).reshape(3, 3))[1:4].reshape(3, N)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        iP = np.where(reached, 1.0 / np.where(reached, P, 1.0), 0.0)
    g, gI, gF = np.zeros((3, N)), np.zeros((3, N)), np.zeros((F, 3, N))
    for a in range(n):
        if fragment[a] < 0:
            continue
        have = np.flatnonzero(pa[a] > 0)
        w = pa[a, have] * iP[have]
        for j in range(3):
            if mode == PRO:
                ga = gpa[a, j, have]
            else:
                ga = w * gr[j, have] + r[have] * ((gpa[a, j, have] - w * gP[j, have]) * iP[have])
            g[j, have] = g[j, have] + ga
            gI[j, have] = gI[j, have] + np.abs(ga)
            gF[fragment[a], j, have] = gF[fragment[a], j, have] + ga
    gX = np.abs(gF[0])
    for f in range(1, F):
        gX = gX + np.abs(gF[f])
    ng = nrm(g)
    dg = np.where(reached, nrm(gI) - ng, 0.0)
    dgi = np.where(reached, nrm(gX) - ng, 0.0)
    return {'dg': dg, 'dgi': dgi, 'P': P, 'reached': reached, 'g': g, 'gI': gI, 'S': S, 'cnt': cnt, 'gr': gr, 'rho': r, 'iP': iP}


def restate_scalar(shape, lattice, atoms, species, pro, rho, fragment, mode, p_min=P_MIN):
    """the same, one voxel and image at a time in Python floats (IEEE float64) -> (dg, dgi) f64[N]"""
    lat = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = [[float(x) for x in at] for at in np.asarray(atoms, dtype=np.float64).reshape(-1, 3)]
    fragment = [int(f) for f in fragment]
    images = [tuple(int(v) for v in row) for row in HS.image_list(lattice, atoms, species, pro.r_cut)]
    nx, ny, nz = shape
    K, n = pro.knots, len(atoms)
    F = max(max(fragment) + 1, 1)
    rho = np.asarray(rho, dtype=np.float64).reshape(shape)
    grad = restated_values(rho, np.asarray(lattice).reshape(3, 3))[1:4]
    dg, dgi = np.zeros(shape), np.zeros(shape)
    for p0 in range(nx):
        for p1 in range(ny):
            for p2 in range(nz):
                pc = []
                for j in range(3):
                    c = lat[j] * p0 / nx
                    c += lat[3 + j] * p1 / ny
                    c += lat[6 + j] * p2 / nz
                    pc.append(c)
                P, gP = 0.0, [0.0, 0.0, 0.0]
                pa, gpa = [0.0] * n, [[0.0, 0.0, 0.0] for _ in range(n)]
                for a, x, y, z in images:
                    s = int(species[a])
                    rc = float(pro.r_cut[s])
                    rc2 = rc * rc
                    ih2 = K / rc2
                    e = [pc[j] - (atoms[a][j] + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                    if d2 >= rc2:
                        continue
                    u = d2 * ih2
                    k = min(int(u), K - 1)
                    t = u - k
                    f, df = float(pro.tables[s][k]), float(pro.tables[s][k + 1]) - float(pro.tables[s][k])
                    T = f + t * df
                    sl = df * ih2
                    c = sl + sl
                    P += T
                    pa[a] += T
                    for j in range(3):
                        G = c * e[j]
                        gP[j] += G
                        gpa[a][j] += G
                if not P > p_min:
                    continue
                r, gr = float(rho[p0, p1, p2]), [float(grad[j][p0, p1, p2]) for j in range(3)]
                g, gI, gF = [0.0] * 3, [0.0] * 3, [[0.0] * 3 for _ in range(F)]
                for a in range(n):
                    if fragment[a] < 0 or not pa[a] > 0.0:
                        continue
                    if mode == PRO:
                        ga = gpa[a]
                    else:
                        iP = 1.0 / P
                        w = pa[a] * iP
                        ga = [w * gr[j] + r * ((gpa[a][j] - w * gP[j]) * iP) for j in range(3)]
                    for j in range(3):
                        g[j] += ga[j]
                        gI[j] += abs(ga[j])
                        gF[fragment[a]][j] += ga[j]
                gX = [abs(gF[0][j]) for j in range(3)]
                for f in range(1, F):
                    gX = [gX[j] + abs(gF[f][j]) for j in range(3)]
                norm = lambda v: math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])   # noqa: E731
                dg[p0, p1, p2] = norm(gI) - norm(g)
                dgi[p0, p1, p2] = norm(gX) - norm(g)
    return dg.reshape(-1), dgi.reshape(-1)


# ---- inputs (shared with tests/test_gpu_igm.py) -----------------------------------------------------------------------------------
def fragments(n, F, loose=False):
    """atoms dealt to F fragments in blocks (the first n / F atoms are fragment 0, ...); `loose`: every fifth atom, from atom 1
    on, in no fragment"""
    fr = (np.arange(n) * F // n).astype(np.int32)
    if loose:
        fr[1::5] = -1
    fr.flags.writeable = False
    return fr


@functools.lru_cache(maxsize=None)
def sums(name):
    """table_sums of one input of tests/test_hirshfeld_cpu.py, computed once and never written"""
    c = HS.case(name)
    t = table_sums(c.shape, c.lattice, c.atoms, c.species, c.pro)
    for a in t.values():
        a.flags.writeable = False
    return t


@functools.lru_cache(maxsize=None)
def reference(name, F, loose, mode, p_min=P_MIN):
    """the restated fields of one input of tests/test_hirshfeld_cpu.py, computed once and never written"""
    c = HS.case(name)
    v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fragments(c.atoms.shape[0], F, loose), MODES[mode], p_min,
                sums=sums(name))
    for a in v.values():
        a.flags.writeable = False
    return v


# ---- the comparisons of tests/test_gpu_igm.py (here, so that tests/history_common.py can make them too) ---------------------------
def keys_of(val, x, lab, n, cut, rho_split):
    inside = (val >= cut) & (lab >= 0) & (lab < n)
    cls = np.where(x < -rho_split, 0, np.where(x > rho_split, 2, 1))
    return np.where(inside, 3 * lab.astype(np.int64) + cls, -1).reshape(-1)


def sum_reference(rho, val, x, lab, n, cut, rho_split):
    """per key 3 a + class: ((fsum, count, fsum of magnitudes) of rho, the same of the field)"""
    k = keys_of(val, x, lab, n, cut, rho_split)
    return grouped(np.asarray(rho, dtype=np.float64), k, 3 * n), grouped(val, k, 3 * n)


def check_sums(got, c, val, x, lab, n, cut, rho_split, what):
    count, charge, integral = got
    (s1, cnt, mag1), (s2, _, mag2) = sum_reference(c.rho, val, x, lab, n, cut, rho_split)
    print(what, 'voxels in the region', int(cnt.sum()), 'per class', [int(cnt[j::3].sum()) for j in range(3)])
    assert count.shape == charge.shape == integral.shape == (n, 3) and count.dtype == np.int64
    assert np.array_equal(count.reshape(-1), cnt), what + ': counts'
    assert np.all(np.abs(charge.reshape(-1) - s1 * VV) <= sum_bound(cnt, mag1)), what + ': the sums of rho'
    assert np.all(np.abs(integral.reshape(-1) - s2 * VV) <= sum_bound(cnt, mag2)), what + ': the sums of the field'
    return cnt


def regions_difference(count, charge, integral, reference, what):
    """None, or what of igm_regions differs from `reference` = sum_reference(...): the region must hold 50 voxels to say anything"""
    (s1, cnt, mag1), (s2, _, mag2) = reference
    if cnt.sum() < 50:
        return f'{what}: the restated region holds {int(cnt.sum())} voxels, too few to say anything'
    if not np.array_equal(count.reshape(-1), cnt):
        return f'{what}: counts differ ({count.reshape(-1).tolist()} against {cnt.tolist()})'
    if not np.all(np.abs(charge.reshape(-1) - s1 * VV) <= sum_bound(cnt, mag1)):
        return f'{what}: the sums of rho differ'
    if not np.all(np.abs(integral.reshape(-1) - s2 * VV) <= sum_bound(cnt, mag2)):
        return f'{what}: the sums of the field differ'
    return None


def exact_case():
    """an input on which every position, image and difference is exact in float64: a cubic cell of edge 8, atoms at multiples of
    1/64, 8 voxels per axis.  A translation of an atom by a lattice vector then moves its images to exactly the same points"""
    rng = np.random.default_rng(11)
    lattice = np.eye(3) * 8.0
    atoms = rng.integers(0, 512, (5, 3)).astype(np.float64) / 64.0
    species = np.array([0, 1, 0, 1, 0], np.int32)
    x = np.arange(65, dtype=np.float64) / 64
    tab = np.stack([(1.0 - x) ** 2, 0.5 * (1.0 - x) ** 3])
    tab[:, -1] = 0.0
    pro = ProAtoms(tab, [3.0, 2.5])
    rho = rng.random((8, 8, 8)) + 0.1
    return (8, 8, 8), lattice, atoms, species, pro, rho


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', ['three', 'thin'])
def test_vector_and_scalar_restatement_agree_bit_for_bit(name, mode):
    c = HS.case(name)
    for F, loose in ((2, False), (3, True)):
        fr = fragments(8, F, loose)
        v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode])
        dg, dgi = restate_scalar(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode])
        assert (bits(v['dg']) == bits(dg)).all() and (bits(v['dgi']) == bits(dgi)).all(), (name, mode, F)
        assert v['reached'].any()


@pytest.mark.parametrize('name', ['cubic_r3', 'tric_r2'])
def test_the_stockholder_gradients_sum_to_the_gradient_of_the_density(name):
    """With every atom in a fragment, sum_a ga = gr sum_a w_a + rho (sum_a gp_a - gP sum_a w_a) / P = gr exactly when sum_a p_a = P
    and sum_a gp_a = gP.  THE BOUND, per component j at a reached voxel with m images inside their cutoff and n atoms: P, the p_a,
    gP and the gp_a are running sums of at most m terms, so they lie within m u of their exact values RELATIVE TO THE SUM OF THE
    MAGNITUDES of their terms -- P and sum_a p_a (positive terms) within m u P, gP_j and sum_a gp_a,j within m u S_j with
    S_j = sum_i |G_i,j|.  Every ga,j is formed from them with six more roundings and the n of them are added with n more.  With
    M_j = |gr_j| + 2 |rho| S_j / P, the size of the terms that cancel,  |sum_a ga,j - gr_j| <= 2 (m + n + 10) u M_j."""
    v = reference(name, 2, False, 'stockholder')
    c = HS.case(name)
    at = v['reached']
    assert at.sum() > 1000
    n = c.atoms.shape[0]
    for j in range(3):
        M = np.abs(v['gr'][j]) + 2.0 * np.abs(v['rho']) * v['S'][j] * v['iP']
        err = np.abs(v['g'][j] - v['gr'][j])[at]
        bound = (2.0 * (v['cnt'] + n + 10) * U * M)[at]
        assert (err <= bound).all(), (name, j, float((err / np.maximum(bound, 1e-300)).max()))
    assert np.abs(v['gr']).max() > 1.0      # (the gradients are not small: the bound is a relative one)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', ['cubic_r3', 'tric_r2', 'twins'])
def test_inter_does_not_exceed_the_whole_beyond_rounding(name, mode):
    """gX_j = sum_F |sum_{a in F} ga,j| <= sum_a |ga,j| = gI_j and nrm is monotone in the magnitudes, so dgi <= dg.  THE BOUND: the
    sums gF and gI of at most n terms each lie within n u gI_j of their exact values, gX adds F roundings, each norm five: dgi - dg
    = nrm(gX) - nrm(gI) <= (2 n + F + 10) u nrm(gI)."""
    n = HS.case(name).atoms.shape[0]
    for F in (2, 4):
        v = reference(name, F, False, mode)
        bound = (2 * n + F + 10) * U * nrm(v['gI'])
        assert (v['dgi'] <= v['dg'] + bound).all(), (name, mode, F)
        assert v['dgi'].max() > 0 and v['dg'].max() > 0
        assert v['dg'].min() > -1e-12 and v['dgi'].min() > -1e-12


def test_the_issues_figures_hold_on_cubic_r3():
    """6 - 8 % of the voxels have dgi above 1 % of its maximum: regions and domains are not empty there"""
    v = reference('cubic_r3', 2, False, 'stockholder')
    share = float((v['dgi'] > 0.01 * v['dgi'].max()).mean())
    assert 0.02 < share < 0.2, share


@pytest.mark.parametrize('mode', list(MODES))
def test_one_fragment_of_every_atom_has_no_inter_part(mode):
    c = HS.case('tric_r2')
    v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, np.zeros(8, np.int32), MODES[mode])
    assert (v['dgi'] == 0).all() and v['dg'].max() > 0      # (gX is |g| per component: the same squares)


def test_every_atom_in_its_own_fragment_is_refused():
    with pytest.raises(ValueError, match='at most 4'):
        igm.check_fragments(np.arange(8), 8)
    fr, F = igm.check_fragments(np.array([0, 3, -1, 1]), 4)
    assert F == 4 and fr.dtype == np.int32
    for bad in (np.array([0, -2, 0, 0]), np.zeros(3, np.int32), np.zeros(4), np.zeros((2, 2), np.int32)):
        with pytest.raises(ValueError):
            igm.check_fragments(bad, 4)


@pytest.mark.parametrize('mode', list(MODES))
def test_translation_by_a_lattice_vector_changes_no_bit(mode):
    shape, lattice, atoms, species, pro, rho = exact_case()
    fr = np.array([0, 1, 0, -1, 1], np.int32)
    v = restate(shape, lattice, atoms, species, pro, rho, fr, MODES[mode])
    moved = atoms.copy()
    moved[1] += lattice[0] - lattice[2]
    moved[4] -= 2 * lattice[1]
    w = restate(shape, lattice, moved, species, pro, rho, fr, MODES[mode])
    assert v['dg'].max() > 0 and v['dgi'].max() > 0
    assert (bits(v['dg']) == bits(w['dg'])).all() and (bits(v['dgi']) == bits(w['dgi'])).all()


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', ['three', 'odd_k1'])
def test_a_wider_image_range_gives_the_same_bits(name, mode):
    c = HS.case(name)
    fr = fragments(8, 3, True)
    v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode])
    lo, hi = HS.shift_ranges(c.lattice, c.atoms, c.species, c.pro.r_cut)
    widen = int((hi - lo + 1).max() + 1) // 2          # (at least doubles every range)
    w = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode], widen=widen)
    assert (bits(v['dg']) == bits(w['dg'])).all() and (bits(v['dgi']) == bits(w['dgi'])).all()


def test_atoms_of_no_fragment_change_the_floor_only():
    """PRO mode: an atom with fragment -1 enters P and nothing else, so the fields are those of the input without the atom
    wherever that input is reached too, and P is the Hirshfeld restatement's with every atom"""
    c = HS.case('cubic_r3')
    fr = np.array([0, 0, -1, 0, 1, 1, -1, 1], np.int32)
    v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, PRO)
    keep = fr >= 0
    sp = np.arange(int(keep.sum()), dtype=np.int32)
    pro = ProAtoms(c.pro.tables[c.species[keep]], c.pro.r_cut[c.species[keep]])
    w = restate(c.shape, c.lattice, c.atoms[keep], sp, pro, c.rho, fr[keep], PRO)
    both = w['reached']
    assert both.sum() > 1000 and (v['reached'] | ~both).all()
    assert (bits(v['dg'])[both] == bits(w['dg'])[both]).all() and (bits(v['dgi'])[both] == bits(w['dgi'])[both]).all()
    assert (bits(v['P']) == bits(HS.reference('cubic_r3')[0])).all()
    assert (v['reached'] & ~both).any()      # (the atoms of no fragment do reach voxels the others do not)


def test_the_floor_is_a_strict_comparison():
    c = HS.case('tric_r2')
    fr = fragments(8, 2)
    P = HS.reference('tric_r2')[0]
    p_min = float(np.sort(P[P > 0])[P[P > 0].size // 3])
    v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, STOCK, p_min)
    at = np.flatnonzero(P == p_min)
    assert at.size and not v['reached'][at].any() and (v['dg'][at] == 0).all() and (P <= 0).any()


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_igm_calls():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    want = {
        'xb_igm_field': ['xb_ctx *c', 'const double lattice[9]', 'const int32_t *fragment', 'int n_fragments', 'int mode', 'double p_min',
                         'int flags', 'double *dg_host', 'double *dgi_host', 'void *dg_dev', 'void *dgi_dev', 'int64_t stats[3]'],
        'xb_igm_sum': ['xb_ctx *c', 'const void *val_dev', 'const void *x_dev', 'int64_t n', 'double voxel_volume', 'double cut',
                       'double rho_split', 'int64_t *count', 'double *charge', 'double *integral'],
    }
    vp, pd, pi, i64, dbl, i = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int64, C.c_double, C.c_int
    types = {'xb_igm_field': [vp, pd, vp, i, i, dbl, i, vp, vp, vp, vp, pi], 'xb_igm_sum': [vp, vp, vp, i64, dbl, dbl, dbl, pi, pd, pd]}
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        assert [' '.join(a.split()) for a in m.group(1).split(',')] == args, name
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and argtypes == types[name], name
    for method in ('igm_field', 'igm_sum'):
        assert callable(getattr(_lib.Context, method))
    m = re.search(r'enum\s*\{\s*XB_IGM_PRO = (\d+), XB_IGM_STOCKHOLDER = (\d+), XB_IGM_FRAGMENTS_MAX = (\d+)\s*\}', hdr)
    assert m and tuple(int(x) for x in m.groups()) == (_lib.XB_IGM_PRO, _lib.XB_IGM_STOCKHOLDER, _lib.XB_IGM_FRAGMENTS_MAX) == (0, 1, 4)
    # the definition is written down where the issue asks for it; no timer slot, option key or block came with it
    for line in ('sl   = df * ih2', 'c    = sl + sl', 'G[j] = c * e[j]', 'ga[j] = w * gr[j] + rho * ((gp_a[j] - w * gP[j]) * iP)',
                 'nrm(v) = sqrt((v0*v0 + v1*v1) + v2*v2)', 'piecewise constant'):
        assert line in text, line
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 27\.', design, flags=re.M) and 'piecewise constant' in design
    assert _lib.XB_TIMER_COUNT == 11 and not any(k.startswith(('XB_OPT_IGM', 'XB_TIMER_IGM')) for k in dir(_lib))
    blocks = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'ctx_buffers.h')).read()
    assert 'igm' not in blocks.lower(), 'both calls use the block of the NCI sums'
    assert igm.P_MIN == 1e-6 and igm.MODES == {'pro': 0, 'stockholder': 1}


def test_the_library_exports_the_calls_and_refuses_a_null_context(lib):
    lat = (C.c_double * 9)(*np.eye(3).reshape(-1))
    fr = (C.c_int32 * 2)(0, 1)
    st = (C.c_int64 * 3)()
    out = (C.c_double * 8)()
    assert lib.xb_igm_field(None, lat, fr, 2, 0, 0.0, 0, C.cast(out, C.c_void_p), None, None, None, st) == _lib.XB_E_ARG
    assert b'xb_igm_field' in lib.xb_last_error()
    cnt = (C.c_int64 * 3)()
    assert lib.xb_igm_sum(None, C.cast(out, C.c_void_p), C.cast(out, C.c_void_p), 1, 1.0, 0.5, 0.01, cnt, out, out) == _lib.XB_E_STATE
    assert b'xb_igm_sum' in lib.xb_last_error()


def test_the_python_layer_refuses_before_it_touches_the_device():
    c = HS.case('three')
    args = (c.rho, c.lattice, c.atoms)
    with pytest.raises(ValueError, match='at most 4'):
        igm.igm_fields(*args, np.arange(8), c.species, c.pro)
    with pytest.raises(ValueError, match='mode'):
        igm.igm_fields(*args, fragments(8, 2), c.species, c.pro, mode='hirshfeld')
    for p_min in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='p_min'):
            igm.igm_fields(*args, fragments(8, 2), c.species, c.pro, p_min=p_min)
    with pytest.raises(ValueError, match='either'):
        igm.igm_fields(*args, fragments(8, 2))
    with pytest.raises(ValueError, match='species'):
        igm.igm_fields(*args, fragments(8, 2), None, c.pro)
    for cut in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='bound'):
            igm.igm_isosurface(*args, fragments(8, 2), cut, c.species, c.pro)
        with pytest.raises(ValueError, match='bound'):
            igm.igm_domains(*args, fragments(8, 2), level=cut, species=c.species, proatoms=c.pro)
        with pytest.raises(ValueError, match='bound'):
            igm.igm_regions(c.rho, np.zeros(c.shape, np.int32), c.lattice, c.atoms, fragments(8, 2), 8, 1.0, cut, species=c.species, proatoms=c.pro)


def test_bader_has_the_flags_and_they_are_off():
    assert Bader.igm_flag is False and Bader.igm_domains_flag is False and Bader.igm_fragments is None
    assert (Bader.igm_mode, Bader.igm_cut, Bader.igm_rho_split, Bader.igm_p_min) == ('stockholder', igm.DG_CUT, igm.RHO_SPLIT, igm.P_MIN)
    assert callable(Bader.igm_analysis) and callable(Bader.igm_domain_analysis)

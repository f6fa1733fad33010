"""The host side of the NCI index (pybader_amd/nci.py) and the plain numpy restatement of the definition in include/bader_hip.h /
DESIGN.md section 20 that tests/test_gpu_nci.py compares the kernels with.

The restatement stands on test_laplacian_cpu.restated_values -- rho, the gradient and the Hessian of the 19-point stencil are
not restated a second time -- and adds g2, the invariants, sigma, q and r8, the region, the classes and the bins, each operation
one elementwise IEEE float64 operation in the order the definition writes.  Everything but the field s is therefore the bits the
device forms.  sigma is written here as the definition reads (the sequence, its sign changes, its trailing zeros), not as
pybader_amd.nci or the kernel compute it.

What the restatement itself is checked against: numpy.linalg.eigvalsh for sigma, on whole grids and on hand-made matrices; the
division form sqrt(g2) / (C rho^(4/3)) < e for the multiplicative test; a binary search for the bins counted one edge at a time.

The sums per key 3 a + class are compared with math.fsum under the bound test_laplacian_cpu.sum_bound / test_gpu_sums.bound use,
with their arguments:

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

test_the_bound_notices_a_voxel_in_the_wrong_class shows for every input of the GPU sums what that bound is worth."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, build, nci, synth
from test_laplacian_cpu import COHERENT_SHAPE, coherent_maps, grouped, restated_values, sum_bound
from test_multipole_cpu import VV, label_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATS = {'tric': synth.TRICLINIC, 'cubic': synth.CUBIC6}
NCI_C = float.fromhex('0x1.8bfd4dd6882cbp+2')          # the header's XB_NCI_C
SIGMA_GRIDS = [(24, 20, 28), (9, 7, 33), (40, 12, 16), (24, 24, 24)]
CUTS = [(0.5, 0.05), (0.5, 0.3), (1.0, 1.0), (0.3, 0.5)]     # (s_cut, rho_cut) of the region tests
RHO_SPLIT = 0.01


def _define(name, text):
    return int(re.search(r'^#define %s (\d+)' % name, text, re.M).group(1))


try:
    with open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_stencil.h')) as _f:
        ST_BINS = _define('ST_BINS', _f.read())
except OSError:         # (the tests below then fail one by one instead of the module failing to import)
    ST_BINS = 0
LABELS_LDS = ST_BINS // 3       # the label count up to which the sums' keys fit the LDS bins


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def invariants(H):
    """(I1, I2, I3) of H = (xx, xy, xz, yy, yz, zz)"""
    xx, xy, xz, yy, yz, zz = H
    i1 = (xx + yy) + zz
    i2 = ((xx * yy - xy * xy) + (xx * zz - xz * xz)) + (yy * zz - yz * yz)
    i3 = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)
    return i1, i2, i3


def sigma_of(i1, i2, i3):
    """Descartes' rule as the definition reads: the sequence (1, -I1, I2, -I3), p its sign changes with zeros skipped, z its
    trailing zeros, neg = 3 - p - z; +1 if p >= 2, -1 if neg >= 2, else 0"""
    i1, i2, i3 = (np.asarray(a, dtype=np.float64) for a in (i1, i2, i3))
    seq = [np.ones(i1.shape), -i1, i2, -i3]
    sign = [np.where(t > 0, 1, np.where(t < 0, -1, 0)) for t in seq]
    p = np.zeros(i1.shape, np.int64)
    for a in range(4):                      # a pair (a, b) of non-zero entries with only zeros between them changes sign or not
        for b in range(a + 1, 4):
            between = np.ones(i1.shape, bool)
            for k in range(a + 1, b):
                between &= sign[k] == 0
            p += between & (sign[a] * sign[b] == -1)
    z = np.zeros(i1.shape, np.int64)
    trailing = np.ones(i1.shape, bool)
    for t in sign[:0:-1]:
        trailing &= t == 0
        z += trailing
    neg = 3 - p - z
    assert (p + z <= 3).all()
    return np.where(p >= 2, 1, np.where(neg >= 2, -1, 0)).astype(np.int64)


def thresholds(edges):
    a = NCI_C * np.asarray(edges, dtype=np.float64)
    a2 = a * a
    return (a2 * a2) * a2


def restated(rho, lattice):
    """every per-voxel value of the definition: rho, g2, sigma, r2, r8, q, x and the field s (the only one not bit-defined)"""
    vals = restated_values(np.ascontiguousarray(rho, dtype=np.float64), lattice)
    rho, (gx, gy, gz) = vals[0], vals[1:4]
    g2 = (gx * gx + gy * gy) + gz * gz
    sigma = sigma_of(*invariants(vals[4:]))
    r2 = rho * rho
    r4 = r2 * r2
    r8 = r4 * r4
    q = (g2 * g2) * g2
    pos = rho > 0
    x = np.where(pos, sigma.astype(np.float64) * rho, 0.0)
    safe = np.where(pos, rho, 1.0)
    s = np.where(pos, np.sqrt(g2) / (NCI_C * (safe * np.cbrt(safe))), np.inf)
    out = {'rho': rho, 'g2': g2, 'sigma': sigma, 'r2': r2, 'r8': r8, 'q': q, 'x': x, 's': s, 'pos': pos, 'hessian': vals[4:]}
    for a in out.values():
        a.flags.writeable = False
    return out


def below(v, e):
    """ "s < e" of the definition"""
    return v['q'] < thresholds(e) * v['r8']


def region(v, s_cut, rho_cut):
    return v['pos'] & below(v, s_cut) & (v['rho'] < rho_cut)


def classes(v, rho_split):
    return np.where(v['x'] < -rho_split, 0, np.where(v['x'] > rho_split, 2, 1))


def keys(v, labels, n, s_cut, rho_cut, rho_split):
    """3 a + class of the voxels of the region with a label in [0, n), -1 elsewhere (flat, int64)"""
    lab = np.asarray(labels).astype(np.int64)
    ok = region(v, s_cut, rho_cut) & (lab >= 0) & (lab < n)
    return np.where(ok, 3 * lab + classes(v, rho_split), -1).reshape(-1)


def bins_by_count(products, value):
    """the definition's bin: (the number of j with products[j] <= value) - 1; products [m + 1, ...]"""
    return sum((pj <= value).astype(np.int64) for pj in products) - 1


def bins_by_search(products, value):
    """the same by a binary search per voxel over the monotone products"""
    m1 = len(products)
    stack = np.stack([np.broadcast_to(pj, value.shape) for pj in products])
    lo, hi = np.zeros(value.shape, np.int64), np.full(value.shape, m1, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = np.where(act, (lo + hi) // 2, 0)
        take = np.take_along_axis(stack, mid[None], axis=0)[0] <= value
        lo = np.where(act & take, mid + 1, lo)
        hi = np.where(act & ~take, mid, hi)
    return lo - 1


def histogram(v, s_edges, x_edges):
    """int64[n_s, n_x] of the definition"""
    t = thresholds(s_edges)
    ks = bins_by_count([tj * v['r8'] for tj in t], v['q'])
    kx = bins_by_count(list(np.asarray(x_edges, dtype=np.float64)), v['x'])
    n_s, n_x = len(s_edges) - 1, len(x_edges) - 1
    ok = v['pos'] & (ks >= 0) & (ks < n_s) & (kx >= 0) & (kx < n_x)
    out = np.zeros((n_s, n_x), np.int64)
    np.add.at(out, (ks[ok], kx[ok]), 1)
    return out


# ---- the inputs (shared with tests/test_gpu_nci.py) ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def density(kind, shape, lname):
    """synth: the eight synthetic atoms on their background.  rough: the same + 0.02 hash noise.  holes: rough with voxels that
    are +0.0, -0.0 and negative (no region, no bin, s = +inf there).  Never written."""
    lat = LATS[lname]
    if kind == 'synth':
        rho = synth.synth_density(shape, lat)
    else:
        rho = synth.rough_density(shape, lat, noise=0.02)
    if kind == 'holes':
        flat = rho.reshape(-1)
        flat[::7] = 0.0
        flat[3::11] = -0.0
        flat[5::13] = -flat[5::13]
    rho = np.ascontiguousarray(rho)
    rho.flags.writeable = False
    return rho


@functools.lru_cache(maxsize=None)
def values(kind, shape, lname):
    return restated(density(kind, shape, lname), LATS[lname])


SUM_SHAPES = [(13, 17, 19), (20, 9, 33)]
N_LABELS = [2, LABELS_LDS, LABELS_LDS + 1, 3000]      # both sides of the LDS limit (85 | 86), and the global route far above it
SUM_CUTS = (1.5, 1.0, 0.03)                            # (s_cut, rho_cut, rho_split): every class holds voxels on every input


def sum_inputs():
    """(what, density kind, shape, lattice name, labels, n) for every sum the GPU file checks: the noise maps of
    test_multipole_cpu.label_map (labels -1, n, n + 7 and INT32_MAX among them) and the coherent maps of test_laplacian_cpu"""
    for shape in SUM_SHAPES:
        for lname in LATS:
            for n in N_LABELS:
                yield f'{shape} {lname} n {n}', 'holes', shape, lname, label_map(shape, n), n
    for lname in LATS:
        for what, (lab, n_own) in coherent_maps(COHERENT_SHAPE).items():
            for n in (n_own, LABELS_LDS + 1):
                yield f'{what}, {lname}, n {n}', 'rough', COHERENT_SHAPE, lname, np.ascontiguousarray(lab, dtype=np.int32), n


def sum_reference(v, lab, n, cuts=SUM_CUTS):
    """per key 3 a + class: ((fsum, count, fsum of magnitudes) of rho, the same of rho^2)"""
    k = keys(v, lab, n, *cuts)
    return grouped(v['rho'], k, 3 * n), grouped(v['r2'], k, 3 * n)


# ---- the comparisons of tests/test_gpu_nci.py (here, so that tests/history_common.py can make them too) ------------------------
S_REL = 16 * 2.0 ** -52


def check_s(got, v, what):
    """+inf exactly where the restatement has it, within the bound elsewhere (the measured maximum printed first)"""
    want = v['s']
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isposinf(got), ~v['pos']), f'{what}: s is +inf exactly where rho <= 0'
    fin = v['pos']
    err = np.abs(got[fin] - want[fin])
    rel = float(np.max(err / np.where(want[fin] > 0, want[fin], 1.0), initial=0.0))
    print(f'{what}: s off by at most {rel / 2.0 ** -52:.2f} * 2^-52 relative (bound 16)')
    assert np.all(err <= S_REL * want[fin]), f'{what}: s off by {rel / 2.0 ** -52:.2f} * 2^-52 relative'


def check_sums(got, v, lab, n, what, cuts=SUM_CUTS):
    """counts ==; the bound for the sums of rho and of rho^2 of every key (each figure printed before it is asserted)"""
    (s1, cnt, mag1), (s2, cnt2, mag2) = sum_reference(v, lab, n, cuts)
    count, charge, charge2 = got
    assert count.shape == charge.shape == charge2.shape == (n, 3) and count.dtype == np.int64
    assert np.array_equal(count.reshape(-1), cnt) and np.array_equal(cnt, cnt2), f'{what}: counts'
    for name, g, w, mag in (('sum of rho', charge, s1, mag1), ('sum of rho^2', charge2, s2, mag2)):
        lim = sum_bound(cnt, mag)
        err = np.abs(g.reshape(-1) - w * VV)
        k = int(np.argmax(err - lim))
        print(f'{what}: {name}, worst key {k} ({cnt[k]} voxels): off by {err[k]:.3e}, bound {lim[k]:.3e}')
        assert np.all(err <= lim), f'{what}: {name} of key {k} ({cnt[k]} voxels) off by {err[k]:.3e}, bound {lim[k]:.3e}'
        assert not g.reshape(-1)[cnt == 0].any(), f'{what}: something landed on a key nobody carries'
    return cnt


# the thresholds and edges of the call-history tests: the region and the bins hold voxels on every grid of history_common
HISTORY_CUTS = (1.0, 1.0, 0.03)
HISTORY_EDGES = (np.array([0.1, 0.3, 0.5, 1.0, 2.0]), np.array([-0.5, -0.03, 0.0, 0.03, 0.5]))


def fields_difference(s, x, v, what):
    """None, or which of the two fields of nci_fields differs from the restated values `v`"""
    if not np.array_equal(x.view(np.uint64), v['x'].view(np.uint64)):
        return f'{what}: x differs'
    ok = v['pos']
    if not np.array_equal(np.isposinf(s), ~ok) or not np.all(np.abs(s[ok] - v['s'][ok]) <= S_REL * v['s'][ok]):
        return f'{what}: s differs'
    return None


def regions_difference(count, charge, charge2, reference, what):
    """None, or what of nci_regions differs from `reference` = sum_reference(v, lab, n, cuts)"""
    (s1, cnt, mag1), (s2, _, mag2) = reference
    if not np.array_equal(count.reshape(-1), cnt) or cnt.sum() < 100:
        return f'{what}: counts differ'
    if not np.all(np.abs(charge.reshape(-1) - s1 * VV) <= sum_bound(cnt, mag1)):
        return f'{what}: the sums of rho differ'
    if not np.all(np.abs(charge2.reshape(-1) - s2 * VV) <= sum_bound(cnt, mag2)):
        return f'{what}: the sums of rho^2 differ'
    return None


def histogram_difference(got, want, what):
    return None if np.array_equal(got, want) and want.sum() > 100 else f'{what}: {int((got != want).sum())} bins differ'


# ---- 1. sigma against eigvalsh ---------------------------------------------------------------------------------------------------
def full(H):
    xx, xy, xz, yy, yz, zz = (np.asarray(a, dtype=np.float64) for a in H)
    return np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)


@pytest.mark.parametrize('kind', ['synth', 'rough'])
@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', SIGMA_GRIDS)
def test_sigma_is_the_sign_of_the_middle_eigenvalue(shape, lname, kind):
    v = values(kind, shape, lname)
    lam = np.linalg.eigvalsh(full(v['hessian']))
    decided = np.abs(lam[..., 1]) > 1e-9 * np.abs(lam).max(axis=-1)
    excluded = int((~decided).sum())
    wrong = int((v['sigma'][decided] != np.sign(lam[..., 1][decided])).sum())
    print(f'{kind} {lname} {shape}: {excluded} of {decided.size} voxels excluded, {wrong} wrong; sigma -1/0/+1: '
          f'{[int((v["sigma"] == k).sum()) for k in (-1, 0, 1)]}')
    assert excluded <= decided.size // 100
    assert wrong == 0
    assert np.array_equal(nci.descartes_sign(*nci.invariants(v['hessian'])), v['sigma']), 'pybader_amd.nci computes the same sigma'


# ---- 2. hand-made matrices -------------------------------------------------------------------------------------------------------
HAND = [((-3.0, -2.0, -1.0), -1), ((-4.0, -2.0, 1.0), -1), ((-1.0, 2.0, 3.0), 1), ((1.0, 2.0, 5.0), 1), ((-2.0, 0.0, 3.0), 0),
        ((0.0, 0.0, 4.0), 0), ((-5.0, -1.0, 0.0), -1), ((0.0, 0.0, 0.0), 0), ((0.0, 2.0, 3.0), 1), ((-2.0, 0.0, 0.0), 0)]
# integer matrices with orthogonal columns of equal length: Q D Q^T is a rotated copy of D times that length squared, and every
# entry and every invariant is an integer -- exact in float64, so a zero eigenvalue stays an exact zero of I3
ROTATIONS = [np.eye(3), np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]),
             np.array([[1.0, 2, 2], [2, 1, -2], [2, -2, 1]]), np.array([[2.0, 3, 6], [3, -6, 2], [6, 2, -3]])]


@pytest.mark.parametrize('eig,want', HAND)
def test_hand_made_matrices(eig, want):
    for Q in ROTATIONS:
        assert np.array_equal(Q @ Q.T, (Q[0] @ Q[0]) * np.eye(3))
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)):
            A = Q @ np.diag(np.array(eig)[list(order)]) @ Q.T
            assert np.array_equal(A, A.T)
            H = [A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]]
            assert int(sigma_of(*invariants(H))) == want, (eig, order, Q.tolist())
            assert int(nci.descartes_sign(*nci.invariants(np.array(H)))) == want


def test_sigma_is_defined_for_every_input():
    bad = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0]
    grid = np.array(np.meshgrid(bad, bad, bad)).reshape(3, -1)
    s = sigma_of(*grid)
    assert set(np.unique(s)) <= {-1, 0, 1} and np.array_equal(s, nci.descartes_sign(*grid))


# ---- 3. "s < e" against the division form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', SIGMA_GRIDS)
def test_the_multiplicative_test_is_the_division_form(shape, lname):
    v = values('rough', shape, lname)
    for s_cut, rho_cut in CUTS:
        mult = below(v, s_cut)
        div = v['s'] < s_cut
        close = np.abs(v['s'] - s_cut) <= 1e-12 * s_cut
        reg = region(v, s_cut, rho_cut)
        signs = [int((reg & (v['sigma'] == k)).sum()) for k in (-1, 0, 1)]
        print(f'{lname} {shape} s < {s_cut}, rho < {rho_cut}: {int(reg.sum())} voxels in the region, sigma -1/0/+1 {signs}, '
              f'{int(close.sum())} within 1e-12 of the threshold')
        assert np.array_equal(mult[~close], div[~close])
        assert int(close.sum()) <= close.size // 1000
    # the regions are no empty sets: over the four thresholds every grid has voxels inside, of both signs
    big = region(v, 1.0, 1.0)
    assert big.any() and (v['sigma'][big] < 0).any() and (v['sigma'][big] > 0).any()


def test_thresholds_of_the_python_layer():
    e = np.array([0.0, 0.1, 0.5, 1.0, 2.5])
    assert np.array_equal(nci.thresholds(e).view(np.uint64), thresholds(e).view(np.uint64))
    assert nci.thresholds(0.5).shape == () and float(nci.thresholds(0.5)) == float(thresholds(0.5))
    assert nci.C == NCI_C == _lib.NCI_C and abs(NCI_C - 2.0 * (3.0 * math.pi ** 2) ** (1.0 / 3.0)) <= 2.0 ** -50
    assert abs(nci.E_PER_A3 - 6.748334) < 1e-6 and (nci.S_CUT, nci.RHO_CUT, nci.RHO_SPLIT) == (0.5, 0.05, 0.01)
    for bad in ([-0.1], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            nci.thresholds(bad)


# ---- 4. bins -----------------------------------------------------------------------------------------------------------------------
def test_bins_by_count_equal_bins_by_binary_search():
    v = values('holes', (20, 9, 33), 'tric')
    for s_edges in ([0.1, 0.2, 0.5, 1.0, 3.0], list(np.linspace(0.15, 2.0, 41)), [0.3, 0.31]):
        prod = [tj * v['r8'] for tj in thresholds(s_edges)]
        a, b = bins_by_count(prod, v['q']), bins_by_search(prod, v['q'])
        assert np.array_equal(a, b) and a.min() == -1 and a.max() == len(s_edges) - 1, 'voxels fall outside on both sides'
    for x_edges in ([-0.3, -0.05, 0.0, 0.05, 0.3], list(np.linspace(-0.2, 0.2, 33))):
        a, b = bins_by_count(list(np.array(x_edges)), v['x']), bins_by_search(list(np.array(x_edges)), v['x'])
        assert np.array_equal(a, b) and a.min() == -1 and a.max() == len(x_edges) - 1


def test_histogram_counts_every_positive_voxel_once_inside_wide_edges():
    v = values('holes', (13, 17, 19), 'cubic')
    wide = histogram(v, [0.0, 0.5, 1e6], [-1e3, 0.0, 1e3])
    assert wide.sum() == int(v['pos'].sum()) and (wide > 0).all()
    # x = 0.0 (sigma = 0) lies in the bin that starts at the edge 0.0
    assert wide[:, 1].sum() == int((v['pos'] & (v['sigma'] >= 0)).sum())


# ---- 5. degenerate inputs ----------------------------------------------------------------------------------------------------------
def test_a_constant_positive_field():
    for lname in LATS:
        v = restated(np.full((5, 6, 7), 0.03125), LATS[lname])
        assert not v['sigma'].any() and not v['g2'].any() and not v['x'].any() and not v['s'].any()
        assert region(v, 0.5, 0.05).all() and (classes(v, 0.01) == 1).all()
        k = keys(v, np.zeros((5, 6, 7), np.int32), 1, 0.5, 0.05, 0.01)
        assert (k == 1).all()


def test_voxels_without_density_are_nowhere():
    v = values('holes', (13, 17, 19), 'tric')
    out = ~v['pos']
    assert out.sum() > 100 and (v['rho'][out] <= 0).all()
    assert np.isposinf(v['s'][out]).all() and not v['x'][out].any() and not np.signbit(v['x'][out]).any()
    assert np.isfinite(v['s'][v['pos']]).all()
    assert not region(v, 1e6, 1e6)[out].any()
    k = keys(v, np.zeros(v['rho'].shape, np.int32), 1, 1e6, 1e6, 0.01)
    assert (k.reshape(out.shape)[out] == -1).all() and (k.reshape(out.shape)[~out] >= 0).all()
    assert histogram(v, [0.0, 1e6], [-1e6, 1e6]).sum() == int(v['pos'].sum())


def test_point_classes_of_the_python_layer_are_the_restatement():
    """nci.point_classes decides from the ten values of a voxel what the kernels decide from its stencil"""
    for kind, shape, lname in (('holes', (13, 17, 19), 'tric'), ('rough', (9, 7, 33), 'cubic')):
        rho = density(kind, shape, lname)
        v = values(kind, shape, lname)
        ten = np.ascontiguousarray(restated_values(rho, LATS[lname]).reshape(10, -1).T)
        for s_cut, rho_cut in CUTS:
            want = np.where(region(v, s_cut, rho_cut), classes(v, RHO_SPLIT), -1).reshape(-1)
            got = nci.point_classes(ten, s_cut, rho_cut, RHO_SPLIT)
            assert got.dtype == np.int8 and np.array_equal(got, want)


# ---- what the sums' bound is worth ---------------------------------------------------------------------------------------------
def test_every_class_holds_voxels_on_every_input_of_the_sums():
    for what, kind, shape, lname, lab, n in sum_inputs():
        k = keys(values(kind, shape, lname), lab, n, *SUM_CUTS)
        per_class = [int(((k >= 0) & (k % 3 == c)).sum()) for c in range(3)]
        assert min(per_class) >= 20, (what, per_class)


def test_the_bound_notices_a_voxel_in_the_wrong_class():
    """one voxel of the region counted in another class of its label moves both keys' sums of rho and of rho^2 by more than the
    bound, on every input of the GPU sums -- and the voxel is a typical one of its key (the median density), not the largest"""
    seen = 0
    for what, kind, shape, lname, lab, n in sum_inputs():
        v = values(kind, shape, lname)
        k = keys(v, lab, n, *SUM_CUTS)
        for terms in (v['rho'].reshape(-1), v['r2'].reshape(-1)):
            s, cnt, mag = grouped(terms, k, 3 * n)
            lim = sum_bound(cnt, mag)
            a = int(np.argmax(cnt))                                  # the key with the most voxels: the widest bound
            b = 3 * (a // 3) + (a % 3 + 1) % 3                       # another class of the same label
            mine = np.flatnonzero(k == a)
            vox = mine[np.argsort(terms[mine])[mine.size // 2]]
            wrong = k.copy()
            wrong[vox] = b
            s2, cnt2, _ = grouped(terms, wrong, 3 * n)
            for key in (a, b):
                assert abs(s2[key] - s[key]) * VV > lim[key], (what, key)
                assert cnt2[key] != cnt[key]
        seen += 1
    assert seen >= 2 * len(SUM_SHAPES) * len(N_LABELS)


# ---- 6. ABI and errors -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


def test_header_and_binding_agree_on_the_nci_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_NCI_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_NCI_')}
    assert declared and declared == mirrored, set(declared.items()) ^ set(mirrored.items())
    assert declared == {'XB_NCI_ATTRACTIVE': 0, 'XB_NCI_VDW': 1, 'XB_NCI_REPULSIVE': 2, 'XB_NCI_CLASSES': 3,
                        'XB_NCI_HIST_LDS_BINS': 1024, 'XB_NCI_BINS_MAX': 1 << 24}
    m = re.search(r'^#define XB_NCI_C (\S+)', hdr, re.M)
    assert m and float.fromhex(m.group(1)) == _lib.NCI_C == NCI_C
    want = {
        'xb_nci_field': ['xb_ctx *c', 'const double lattice[9]', 'int flags', 'double *s_host', 'double *x_host', 'void *s_dev',
                         'void *x_dev'],
        'xb_nci_sum': ['xb_ctx *c', 'const double lattice[9]', 'int64_t n', 'double voxel_volume', 'double s_cut', 'double rho_cut',
                       'double rho_split', 'int flags', 'int64_t *count', 'double *charge', 'double *charge2'],
        'xb_nci_hist': ['xb_ctx *c', 'const double lattice[9]', 'const double *s_edges', 'int64_t n_s', 'const double *x_edges',
                        'int64_t n_x', 'int flags', 'int64_t *counts'],
    }
    vp, pd, pi, i64, dbl, i = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int64, C.c_double, C.c_int
    types = {'xb_nci_field': [vp, pd, i, vp, vp, vp, vp], 'xb_nci_sum': [vp, pd, i64, dbl, dbl, dbl, dbl, i, pi, pd, pd],
             'xb_nci_hist': [vp, pd, pd, i64, pd, i64, i, pi]}
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, 'include/bader_hip.h does not declare ' + name
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and argtypes == types[name], name
    for method in ('nci_field', 'nci_sum', 'nci_hist'):
        assert callable(getattr(_lib.Context, method))
    # the definition is written down where the issue asks for it; no timer slot and no option key came with it
    assert 'I3 = (Hxx*(Hyy*Hzz - Hyz*Hyz) - Hxy*(Hxy*Hzz - Hyz*Hxz)) + Hxz*(Hxy*Hyz - Hyy*Hxz)' in text
    assert 'Denormal products take' in text and 'q < T(e)*r8' in text
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 20\.', design, flags=re.M)
    assert _lib.XB_TIMER_COUNT == 11 and not any(k.startswith(('XB_OPT_NCI', 'XB_TIMER_NCI')) for k in dir(_lib))
    assert LABELS_LDS == 85 and (10 * 10 * 34 * 8 + _lib.XB_NCI_HIST_LDS_BINS * 4) * 5 <= 160 * 1024


def test_the_library_exports_the_calls_and_refuses_a_null_context(lib):
    lat = (C.c_double * 9)(*synth.CUBIC6.reshape(-1))
    out = np.full(4, -7.0)
    cnt = np.full(6, -7, np.int64)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    edges = (C.c_double * 3)(0.0, 0.5, 1.0)
    assert lib.xb_nci_field(None, lat, 0, out.ctypes.data, out.ctypes.data, None, None) == _lib.XB_E_STATE
    assert lib.xb_nci_sum(None, lat, 2, 1.0, 0.5, 0.05, 0.01, 0, cnt.ctypes.data_as(pi), out.ctypes.data_as(pd),
                          out.ctypes.data_as(pd)) == _lib.XB_E_STATE
    assert lib.xb_nci_hist(None, lat, edges, 2, edges, 2, 0, cnt.ctypes.data_as(pi)) == _lib.XB_E_STATE
    assert (out == -7.0).all() and (cnt == -7).all(), 'a refused call writes nothing'


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.nci_flag is False and callable(Bader.nci_analysis)
    assert (Bader.nci_s_cut, Bader.nci_rho_cut, Bader.nci_rho_split) == (nci.S_CUT, nci.RHO_CUT, nci.RHO_SPLIT)


def test_the_calls_need_the_gpu(lib):
    if lib.xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.full((4, 4, 4), 0.02)
    lab = np.zeros((4, 4, 4), np.int32)
    for call in (lambda: nci.nci_fields(rho, np.eye(3)), lambda: nci.nci_regions(rho, lab, np.eye(3), 1, 1.0),
                 lambda: nci.nci_histogram(rho, np.eye(3), [0.0, 1.0], [-1.0, 1.0]),
                 lambda: nci.bond_classes(rho, np.eye(3), [0])):
        with pytest.raises(_lib.BaderHipError):
            call()

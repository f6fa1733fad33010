"""The host side of the Laplacian and the Hessian of the density (pybader_amd/laplacian.py, xb_stencil_coeffs) and the plain numpy
restatement of the definition in include/bader_hip.h / DESIGN.md section 18 that tests/test_gpu_laplacian.py compares the
kernels with.

Everything in the restatement is elementwise IEEE float64 in the order the definition writes (np.roll for the wrapped
neighbours), so the values at a voxel are the bits the device forms and the GPU file compares them with ==.  The sums per
label are compared with math.fsum under the bound of tests/test_gpu_multipole.py, per label, for the sum and the sum of
magnitudes alike:

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

test_the_sums_bound_notices_a_voxel_on_the_wrong_label shows for every input of the GPU sums what that bound is worth.

What the restatement itself is checked against: numpy.linalg.inv for the coefficients; a plane wave, of which the stencil is an
eigenfunction with an eigenvalue known in closed form, and that eigenvalue's Taylor distance from the continuum one (the check
that does not rest on the restatement's own coefficients); the vanishing sum of the Laplacian over the cell."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, build, laplacian, synth
from test_multipole_cpu import LATTICES, U, VV, bound, density, label_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))       # the term order 00 11 22 01 02 12
COMPONENTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz
COEFF_SHAPES = [(5, 7, 11), (12, 10, 16)]


def _define(name, text):
    return int(re.search(r'^#define %s (\d+)' % name, text, re.M).group(1))


try:
    with open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_stencil.h')) as _f:
        ST_BINS = _define('ST_BINS', _f.read())
except OSError:         # (the tests below then fail one by one instead of the module failing to import)
    ST_BINS = 0


# ---- the definition, restated -------------------------------------------------------------------------------------------------
def geometry(lattice, shape):
    """(A, M, G) of the definition as nested lists of float64, every operation in the order written there"""
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    A = [[lat[i, j] / np.float64(shape[i]) for j in range(3)] for i in range(3)]
    cof = [[A[(i + 1) % 3][(a + 1) % 3] * A[(i + 2) % 3][(a + 2) % 3] - A[(i + 1) % 3][(a + 2) % 3] * A[(i + 2) % 3][(a + 1) % 3]
            for a in range(3)] for i in range(3)]
    det = (A[0][0] * cof[0][0] + A[0][1] * cof[0][1]) + A[0][2] * cof[0][2]
    M = [[cof[i][a] / det for i in range(3)] for a in range(3)]
    G = [[(M[0][i] * M[0][j] + M[1][i] * M[1][j]) + M[2][i] * M[2][j] for j in range(3)] for i in range(3)]
    return A, M, G


def coefficients(lattice, shape):
    """(t [3, 3], w [6], h [6, 6]) of the definition"""
    _, M, G = geometry(lattice, shape)
    t = np.array([[0.5 * M[a][i] for i in range(3)] for a in range(3)])
    w = np.array([G[i][j] if i == j else 0.5 * G[i][j] for i, j in TERMS])
    h = np.array([[M[a][i] * M[b][i] if i == j else 0.25 * (M[a][i] * M[b][j] + M[a][j] * M[b][i]) for i, j in TERMS]
                  for a, b in COMPONENTS])
    return t, w, h


def by_roll(rho):
    return lambda d: np.roll(rho, (-d[0], -d[1], -d[2]), axis=(0, 1, 2))


def by_modulo(rho):
    p = np.indices(rho.shape)
    return lambda d: rho[tuple((p[j] + d[j]) % rho.shape[j] for j in range(3))]


def step(i, s, j=None, sj=0):
    d = [0, 0, 0]
    d[i] = s
    if j is not None:
        d[j] = sj
    return d


def differences(rho, at=by_roll):
    """(d [6 arrays] in the term order, g [3 arrays]) of the definition"""
    r, c = at(rho), rho
    d = [(r(step(i, 1)) - c) + (r(step(i, -1)) - c) for i in range(3)]
    d += [(r(step(i, 1, j, 1)) - r(step(i, 1, j, -1))) - (r(step(i, -1, j, 1)) - r(step(i, -1, j, -1))) for i, j in TERMS[3:]]
    g = [r(step(i, 1)) - r(step(i, -1)) for i in range(3)]
    return d, g


def dot6(k, d):
    out = k[0] * d[0] + k[1] * d[1]
    for n in range(2, 6):
        out = out + k[n] * d[n]
    return out


def restated_laplacian(rho, lattice, at=by_roll):
    _, w, _ = coefficients(lattice, rho.shape)
    return dot6(w, differences(rho, at)[0])


def restated_values(rho, lattice, at=by_roll):
    """the ten fields of xb_stencil_points, [10, nx, ny, nz]: rho, the gradient, the Hessian"""
    t, _, h = coefficients(lattice, rho.shape)
    d, g = differences(rho, at)
    grad = [((t[a][0] * g[0]) + t[a][1] * g[1]) + t[a][2] * g[2] for a in range(3)]
    return np.stack([rho] + grad + [dot6(h[c], d) for c in range(6)])


def restated_points(rho, lattice, lin):
    return np.ascontiguousarray(restated_values(rho, lattice).reshape(10, -1)[:, np.asarray(lin, dtype=np.int64)].T)


def magnitude(k):
    """S = 4 sum |k|: a bound on the running magnitude of a six-term stencil for |rho| <= 1"""
    return 4.0 * float(np.abs(k).sum())


def grouped(terms, label, n):
    """per label in [0, n): (fsum of the terms, count, fsum of |terms|)"""
    label = np.asarray(label).reshape(-1).astype(np.int64)
    terms = np.asarray(terms).reshape(-1)
    keep = np.flatnonzero((label >= 0) & (label < n))
    order = keep[np.argsort(label[keep], kind='stable')]
    vals, starts = np.unique(label[order], return_index=True)
    s, cnt, mag = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
    for a, lo, hi in zip(vals, starts, list(starts[1:]) + [order.size]):
        x = terms[order[lo:hi]]
        s[a], cnt[a], mag[a] = math.fsum(x), hi - lo, math.fsum(np.abs(x))
    return s, cnt, mag


def sum_bound(cnt, mag, vv=VV):
    return bound(cnt, mag[:, None], vv)[:, 0]


# ---- the inputs of the GPU sums (shared with tests/test_gpu_laplacian.py) --------------------------------------------------------
SUM_SHAPES = [(13, 17, 19), (20, 9, 33)]
N_LABELS = [2, ST_BINS, ST_BINS + 1, 3000]      # both sides of the LDS bin limit, and the global route far above it
COHERENT_SHAPE = (12, 16, 40)


def coherent_maps(shape):
    """the coherent maps of tests/test_gpu_multipole.py: (labels, labels the map uses)"""
    p0, p1, p2 = np.indices(shape)
    return {
        'slabs of two planes (whole waves share a label, it changes between a wave\'s steps)': (p0 // 2, shape[0] // 2 + 1),
        'blocks (runs of 20 voxels: several labels in a wave, each group reduced)': ((p0 // 4) * 4 + (p1 // 8) * 2 + p2 // 20, 16),
        'runs of five (the label changes mid-wave, groups too small to reduce)': (p2 // 5, shape[2] // 5 + 1),
        'one voxel of another label inside a uniform wave': (np.where((p0 == 3) & (p1 == 5) & (p2 == 17), 1, 0), 2),
        'vacuum runs inside uniform waves': (np.where(p2 % 16 < 3, -1, p0 // 6), 3),
    }


NO_VACUUM = 'slabs of two planes (whole waves share a label, it changes between a wave\'s steps)'


@functools.lru_cache(maxsize=None)
def noise(shape, seed=3):
    a = synth.hash_noise(shape, seed)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def sum_field(kind, shape, lname):
    """the restated Laplacian of one density of the GPU sums, computed once"""
    rho = density(shape) if kind == 'decades' else noise(shape)
    lap = restated_laplacian(rho, LATTICES[lname])
    lap.flags.writeable = False
    return rho, lap


def sum_inputs():
    """(what, density kind, shape, lattice name, labels, n) for every sum the GPU file checks"""
    for shape in SUM_SHAPES:
        for lname in LATTICES:
            for n in N_LABELS:
                yield f'{shape} {lname} n {n}', 'decades', shape, lname, label_map(shape, n), n
    for lname in LATTICES:
        for what, (lab, n_own) in coherent_maps(COHERENT_SHAPE).items():
            for n in (n_own, ST_BINS + 1):
                yield f'{what}, {lname}, n {n}', 'noise', COHERENT_SHAPE, lname, np.ascontiguousarray(lab, dtype=np.int32), n


def cell_sum_bound(rho, w):
    return 64 * U * rho.size * magnitude(w) * float(np.abs(rho).max())


# ---- coefficients -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


@pytest.mark.parametrize('shape', COEFF_SHAPES)
@pytest.mark.parametrize('lname', list(LATTICES))
def test_library_coefficients_equal_the_restatement_bit_for_bit(lib, lname, shape):
    t, w, h = _lib.stencil_coeffs(LATTICES[lname], shape)
    rt, rw, rh = coefficients(LATTICES[lname], shape)
    for name, got, want in (('gradient', t, rt), ('laplacian', w, rw), ('hessian', h, rh)):
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, got, want)
    if lname == 'ortho':
        assert not w[3:].any() and w[:3].all(), 'an orthogonal cell has zero mixed coefficients, and they still take part'


@pytest.mark.parametrize('shape', COEFF_SHAPES)
@pytest.mark.parametrize('lname', list(LATTICES))
def test_coefficients_agree_with_numpy_linalg(lname, shape):
    A, M, G = (np.array(x) for x in geometry(LATTICES[lname], shape))
    assert np.array_equal(A, LATTICES[lname] / np.array(shape, dtype=np.float64)[:, None])
    inv, ginv = np.linalg.inv(A), np.linalg.inv(A @ A.T)
    assert np.abs(M - inv).max() <= 1e-12 * np.abs(inv).max()
    assert np.abs(G - ginv).max() <= 1e-12 * np.abs(ginv).max()
    # dp_i / dr_alpha = M[alpha][i]: a step of one voxel along axis i is the Cartesian step A[i], and M maps it back to e_i
    assert np.abs(A @ M - np.eye(3)).max() <= 1e-12
    t, w, h = coefficients(LATTICES[lname], shape)
    assert np.abs(t - 0.5 * inv).max() <= 1e-12 * np.abs(inv).max() and np.abs(w[:3] - np.diag(ginv)).max() <= 1e-12 * np.abs(ginv).max()
    assert np.abs(w[3:] - 0.5 * ginv[[0, 0, 1], [1, 2, 2]]).max() <= 1e-12 * np.abs(ginv).max()
    full = np.einsum('ai,bj->abij', inv, inv)                       # d2/dr_a dr_b = sum_ij M[a][i] M[b][j] d2/dp_i dp_j
    for c, (a, b) in enumerate(COMPONENTS):
        for k, (i, j) in enumerate(TERMS):
            want = full[a, b, i, i] if i == j else 0.25 * (full[a, b, i, j] + full[a, b, j, i])
            assert abs(h[c][k] - want) <= 1e-12 * np.abs(full).max()


def test_coefficient_errors(lib):
    out = (C.c_double * _lib.XB_STENCIL_COEFFS)(*([-7.0] * _lib.XB_STENCIL_COEFFS))
    lat = (C.c_double * 9)(*LATTICES['tric'].reshape(-1))
    flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)                # two parallel rows: the determinant is exactly 0
    assert lib.xb_stencil_coeffs(None, 4, 4, 4, out) == _lib.XB_E_ARG and lib.xb_stencil_coeffs(lat, 4, 4, 4, None) == _lib.XB_E_ARG
    assert lib.xb_stencil_coeffs(lat, 0, 4, 4, out) == _lib.XB_E_ARG and lib.xb_stencil_coeffs(lat, 4, 4, -1, out) == _lib.XB_E_ARG
    assert lib.xb_stencil_coeffs(flat, 4, 4, 4, out) == _lib.XB_E_ARG
    assert list(out) == [-7.0] * _lib.XB_STENCIL_COEFFS, 'a refused call writes nothing'
    assert lib.xb_stencil_coeffs(lat, 1, 2, 9, out) == 0 and all(math.isfinite(v) for v in out)
    with pytest.raises(_lib.BaderHipError) as e:
        _lib.stencil_coeffs(np.zeros((3, 3)), (4, 4, 4))
    assert e.value.code == _lib.XB_E_ARG


# ---- a plane wave is an eigenfunction -----------------------------------------------------------------------------------------
def plane_wave(shape, k):
    """cos(sum x_i p_i), x_i = 2 pi k_i / n_i, the phase of every axis reduced to [0, 2 pi) in integers first"""
    p = np.indices(shape)
    theta = sum(2.0 * np.pi * ((k[i] * p[i]) % shape[i]).astype(np.float64) / shape[i] for i in range(3))
    x = np.array([2.0 * np.pi * k[i] / shape[i] for i in range(3)])
    return np.cos(theta), np.sin(theta), x


@pytest.mark.parametrize('lname,shape,k', [('tric', (12, 10, 16), (1, 2, -1)), ('ortho', (12, 10, 16), (1, 2, -1)),
                                           ('tric', (5, 7, 11), (2, -1, 3)), ('tric', (24, 20, 28), (1, 1, 1))])
def test_a_plane_wave_is_an_eigenfunction(lname, shape, k):
    lat = LATTICES[lname]
    rho, sin_theta, x = plane_wave(shape, k)
    _, M, G = (np.array(a) for a in geometry(lat, shape))
    t, w, h = coefficients(lat, shape)
    c2, s = 2.0 * np.cos(x) - 2.0, np.sin(x)
    # the Laplacian: lambda rho
    lam = sum(G[i, i] * c2[i] for i in range(3)) - sum(2.0 * G[i, j] * s[i] * s[j] for i, j in TERMS[3:])
    err, tol = np.abs(restated_laplacian(rho, lat) - lam * rho).max(), 64 * U * magnitude(w)
    print(f'{lname} {shape} k {k}: laplacian off by {err:.3e}, tolerance {tol:.3e} (S = {magnitude(w):.3g})')
    assert err <= tol
    # ... and lambda is the continuum -x^T G x up to the Taylor remainders of 2 cos x - 2 and sin x sin y
    rem = sum(abs(G[i, i]) * x[i] ** 4 / 12 for i in range(3)) + \
        sum(2 * abs(G[i, j] * x[i] * x[j]) * (x[i] ** 2 + x[j] ** 2) / 6 for i, j in TERMS[3:])
    print(f'  lambda {lam:.6g}, continuum {-(x @ G @ x):.6g}, remainder bound {rem:.3g}')
    assert abs(lam + x @ G @ x) <= rem * (1 + 1e-12)
    # the Hessian: -(M x)(M x)^T rho, the gradient: -(M x) sin(theta), the same way
    vals = restated_values(rho, lat)
    mx = M @ x
    for c, (a, b) in enumerate(COMPONENTS):
        mu = sum(M[a, i] * M[b, i] * c2[i] for i in range(3)) - sum((M[a, i] * M[b, j] + M[a, j] * M[b, i]) * s[i] * s[j] for i, j in TERMS[3:])
        assert np.abs(vals[4 + c] - mu * rho).max() <= 64 * U * magnitude(h[c]), (a, b)
        rem = sum(abs(M[a, i] * M[b, i]) * x[i] ** 4 / 12 for i in range(3)) + \
            sum(abs((M[a, i] * M[b, j] + M[a, j] * M[b, i]) * x[i] * x[j]) * (x[i] ** 2 + x[j] ** 2) / 6 for i, j in TERMS[3:])
        assert abs(mu + mx[a] * mx[b]) <= rem * (1 + 1e-12), (a, b)
    for a in range(3):
        nu = -sum(M[a, i] * s[i] for i in range(3))
        assert np.abs(vals[1 + a] - nu * sin_theta).max() <= 64 * U * 2.0 * np.abs(t[a]).sum(), a     # (|g_i| <= 2)
        assert abs(nu + mx[a]) <= sum(abs(M[a, i]) * abs(x[i]) ** 3 / 6 for i in range(3)) * (1 + 1e-12), a


# ---- the Laplacian sums to zero over the cell ---------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['noise', 'synth'])
@pytest.mark.parametrize('lname', list(LATTICES))
def test_the_laplacian_sums_to_zero_over_the_cell(what, lname):
    shape = (12, 10, 16)
    rho = synth.hash_noise(shape, 3) if what == 'noise' else synth.synth_density(shape, LATTICES[lname])
    _, w, _ = coefficients(LATTICES[lname], shape)
    total, lim = math.fsum(restated_laplacian(rho, LATTICES[lname]).reshape(-1)), cell_sum_bound(rho, w)
    print(f'{what} {lname}: the Laplacian sums to {total:.3e} over the cell, bound {lim:.3e}')
    assert abs(total) <= lim


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
def test_a_constant_field_gives_exactly_zero():
    rho = np.full((5, 6, 7), 0.25)
    for lname in LATTICES:
        vals = restated_values(rho, LATTICES[lname])
        assert not restated_laplacian(rho, LATTICES[lname]).any() and not vals[1:].any() and np.array_equal(vals[0], rho)


@pytest.mark.parametrize('shape', [(1, 2, 9), (2, 2, 2), (3, 3, 3), (5, 7, 11)])
def test_axes_of_one_and_two_need_no_special_case(shape):
    rho = synth.hash_noise(shape, 5)
    for lname in LATTICES:
        a, b = restated_values(rho, LATTICES[lname]), restated_values(rho, LATTICES[lname], by_modulo)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        la, lb = restated_laplacian(rho, LATTICES[lname]), restated_laplacian(rho, LATTICES[lname], by_modulo)
        assert np.array_equal(la.view(np.uint64), lb.view(np.uint64))
    if shape[0] == 1:     # the two neighbours along an axis of one voxel are the voxel itself
        d, g = differences(rho)
        assert not d[0].any() and not g[0].any() and not d[3].any() and not d[4].any()


def test_the_python_layer_forms_the_laplacian_at_a_point_as_the_field_does():
    """laplacian.point_properties has ten values per voxel from the library and forms the Laplacian itself from the densities
    of the 19 stencil points: the same bits as the field, through its own index arithmetic"""
    for shape in [(1, 2, 9), (3, 3, 3), (5, 7, 11)]:
        rho, lat = synth.hash_noise(shape, 8), LATTICES['tric']
        vox = np.stack(np.unravel_index(np.arange(rho.size), shape), axis=1)
        idx = laplacian._neighbour_indices(vox, shape)
        _, w, _ = coefficients(lat, shape)
        got = laplacian._laplacian_at(rho.reshape(-1)[idx], w)
        assert np.array_equal(got.view(np.uint64), restated_laplacian(rho, lat).reshape(-1).view(np.uint64))


def test_point_properties_derives_eigenvalues_ellipticity_and_signature():
    lin = np.arange(4, dtype=np.int64)
    values = np.zeros((4, 10))
    values[:, 0] = [1.0, 2.0, 3.0, 4.0]
    for row, diag in enumerate([(-3.0, -2.0, -1.0), (-4.0, -2.0, 1.0), (-1.0, 2.0, 3.0), (1.0, 2.0, 0.0)]):
        values[row, [4, 7, 9]] = diag
    values[1, 5] = 0.0
    p = laplacian.PointProperties((2, 2, 2), lin, values, np.array([-6.0, -5.0, 4.0, 3.0]))
    assert p.signature.tolist() == [-3, -1, 1, 2] and len(p) == 4 and p.voxels.tolist()[3] == [0, 1, 1]
    assert np.array_equal(p.eigenvalues, [[-3, -2, -1], [-4, -2, 1], [-1, 2, 3], [0, 1, 2]])
    assert p.ellipticity[0] == 0.5 and p.ellipticity[1] == 1.0 and np.isnan(p.ellipticity[2:]).all()
    assert np.array_equal(p.hessian, np.transpose(p.hessian, (0, 2, 1))) and p.laplacian.tolist() == [-6.0, -5.0, 4.0, 3.0]


# ---- what the sums' bound is worth ---------------------------------------------------------------------------------------------
def test_the_sums_bound_notices_a_voxel_on_the_wrong_label():
    """one voxel whose Laplacian lands on another label moves both labels' sums by more than the bound, on every input of the GPU
    sums -- and the voxel is a typical one of its label (the median magnitude), not the largest"""
    seen = 0
    for what, kind, shape, lname, lab, n in sum_inputs():
        _, lap = sum_field(kind, shape, lname)
        terms, label = lap.reshape(-1), lab.reshape(-1).astype(np.int64)
        s, cnt, mag = grouped(terms, label, n)
        lim, lim_abs = sum_bound(cnt, mag), sum_bound(cnt, mag)
        a = int(np.argmax(cnt))                                     # the label with the most voxels: the widest bound
        b = int(next(x for x in np.flatnonzero(cnt > 0) if x != a))    # (every input uses two labels at least)
        mine = np.flatnonzero(label == a)
        v = mine[np.argsort(np.abs(terms[mine]))[mine.size // 2]]
        wrong = label.copy()
        wrong[v] = b
        s2, cnt2, mag2 = grouped(terms, wrong, n)
        for x in (a, b):
            assert abs(s2[x] - s[x]) * VV > lim[x], (what, x)
            assert abs(mag2[x] - mag[x]) * VV > lim_abs[x], (what, x)
        seen += 1
    assert seen == len(list(sum_inputs())) and seen >= 2 * len(SUM_SHAPES) * len(N_LABELS)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_stencil_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_STENCIL_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_STENCIL_')}
    assert declared and declared == mirrored, set(declared.items()) ^ set(mirrored.items())
    assert declared == {'XB_STENCIL_GATHER': 1, 'XB_STENCIL_COEFFS': 51, 'XB_STENCIL_POINT_VALUES': 10}
    want = {
        'xb_stencil_coeffs': ['const double lattice[9]', 'int64_t nx', 'int64_t ny', 'int64_t nz', 'double out[XB_STENCIL_COEFFS]'],
        'xb_laplacian_field': ['xb_ctx *c', 'const double lattice[9]', 'int flags', 'double *out_host', 'void *out_dev'],
        'xb_laplacian_sum': ['xb_ctx *c', 'const double lattice[9]', 'int64_t n', 'double voxel_volume', 'int flags', 'double *sum',
                             'double *abs_sum', 'double *volume'],
        'xb_stencil_points': ['xb_ctx *c', 'const double lattice[9]', 'const int64_t *lin', 'int64_t m', 'double *out'],
    }
    vp, pd, i64, dbl, i = C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_int
    types = {
        'xb_stencil_coeffs': [pd, i64, i64, i64, pd], 'xb_laplacian_field': [vp, pd, i, vp, vp],
        'xb_laplacian_sum': [vp, pd, i64, dbl, i, pd, pd, pd], 'xb_stencil_points': [vp, pd, vp, i64, vp],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, 'include/bader_hip.h does not declare ' + name
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and argtypes == types[name], name
    for method in ('laplacian_field', 'laplacian_sum', 'stencil_points'):
        assert callable(getattr(_lib.Context, method))
    # the definition is written down where the issue asks for it, and no timer slot or option key came with it
    assert 'd_ij = (rho(+i+j) - rho(+i-j)) - (rho(-i+j) - rho(-i-j))' in text and 'M[a][i] = C[i][a] / det' in text
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 18\.', design, flags=re.M)
    assert _lib.XB_TIMER_COUNT == 11 and not any(k.startswith(('XB_OPT_STENCIL', 'XB_OPT_LAPLACIAN', 'XB_TIMER_STENCIL', 'XB_TIMER_LAPLACIAN'))
                                                 for k in dir(_lib))
    assert 1 <= ST_BINS and (10 * 10 * 34 * 8 + ST_BINS * 20) * 5 <= 160 * 1024, 'the tile and the bins of five workgroups fit a compute unit'


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.laplacian_flag is False and callable(Bader.laplacian_analysis)


def test_the_calls_need_the_gpu(lib):
    if lib.xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.ones((4, 4, 4))
    for call in (lambda: laplacian.laplacian(rho, np.eye(3)), lambda: laplacian.basin_laplacian(rho, np.zeros((4, 4, 4), np.int32), np.eye(3), 1, 1.0),
                 lambda: laplacian.point_properties(rho, np.eye(3), [0])):
        with pytest.raises(_lib.BaderHipError):
            call()

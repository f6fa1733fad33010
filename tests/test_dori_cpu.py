"""The host side of DORI (pybader_amd/dori.py) and the plain numpy restatement of the definition in include/bader_hip.h /
DESIGN.md section 26 that tests/test_gpu_dori.py compares the kernels with.

The restatement stands on test_laplacian_cpu.restated_values -- rho, the gradient and the Hessian of the 19-point stencil are not
restated a second time -- and on test_nci_cpu.sigma_of for the sign of lambda2, and adds gg, H g, u, N, D, S and the four cases of
gamma, each operation one elementwise IEEE float64 operation in the order the definition writes.  gamma has no sqrt, no cbrt and
no eigen-solve in it, so EVERYTHING here is the bits the device forms and is compared with ==.  It is written from the
definition, not from pybader_amd.dori: whole [nx, ny, nz] fields, the three components in loops, the cases by masks.

What the restatement itself is checked against: the range [0, 1]; the exact zeros of a constant field and of voxels without
density; an integer density whose eight symmetric voxels are exact critical points (the S == 0 rule, which no synthetic density
reaches); exact invariance under powers of two in the density and in the lattice; a single exponential atom (gamma small in its
tail) and two of them (gamma near 1 between them).

The sums per key 3 a + class are compared with math.fsum under the bound test_laplacian_cpu.sum_bound / test_nci_cpu use:

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

test_the_bound_notices_a_voxel_in_the_wrong_class_or_on_the_wrong_side shows for every input of the GPU sums what it is worth."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, build, dori, nci, synth
from test_laplacian_cpu import grouped, restated_values, sum_bound
from test_multipole_cpu import VV
from test_nci_cpu import LABELS_LDS, LATS, density, invariants, sigma_of, sum_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 6, 7), (13, 17, 19), (20, 9, 33)]
RHO_MINS = [0.0, 1e-3, 0.05]
SUM_CUTS = (0.5, 0.0, 0.03)        # (d_cut, rho_min, rho_split): every class holds >= 57 voxels on every input of the sums
SYMMETRIC_SHAPES = [(8, 8, 8), (6, 10, 12)]


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def restated(rho, lattice, rho_min):
    """every per-voxel value of the definition: rho, r2 = rho rho, N, D, S, gamma, sigma, x"""
    vals = restated_values(np.ascontiguousarray(rho, dtype=np.float64), lattice)
    c, g = vals[0], [vals[1], vals[2], vals[3]]
    xx, xy, xz, yy, yz, zz = vals[4:]
    rows = [(xx, xy, xz), (xy, yy, yz), (xz, yz, zz)]
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        h = [(row[0] * g[0] + row[1] * g[1]) + row[2] * g[2] for row in rows]
        u = [c * h[a] - gg * g[a] for a in range(3)]
        N = 4.0 * ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        D = (gg * gg) * gg
        S = N + D
        gamma = np.zeros(c.shape)
        dense = c > rho_min                                   # (a NaN, +0, -0, a negative density: not)
        regular = dense & (S > 0) & (S < np.inf)
        gamma[regular] = N[regular] / S[regular]
        curved = np.zeros(c.shape, bool)
        for comp in vals[4:]:
            curved |= comp != 0
        critical = dense & (S == 0) & curved
        gamma[critical] = 1.0
    sigma = sigma_of(*invariants(vals[4:]))
    x = np.zeros(c.shape)
    x[dense] = sigma[dense].astype(np.float64) * c[dense]
    out = {'rho': c, 'r2': c * c, 'N': N, 'D': D, 'S': S, 'gamma': gamma, 'sigma': sigma, 'x': x, 'dense': dense, 'critical': critical}
    for a in out.values():
        a.flags.writeable = False
    return out


def classes(v, rho_split):
    return np.where(v['x'] < -rho_split, 0, np.where(v['x'] > rho_split, 2, 1))


def keys(v, labels, n, d_cut, rho_split):
    """3 a + class of the voxels of the region gamma >= d_cut with a label in [0, n), -1 elsewhere (flat, int64)"""
    lab = np.asarray(labels).astype(np.int64)
    ok = (v['gamma'] >= d_cut) & (lab >= 0) & (lab < n)
    return np.where(ok, 3 * lab + classes(v, rho_split), -1).reshape(-1)


@functools.lru_cache(maxsize=None)
def values(kind, shape, lname, rho_min):
    return restated(density(kind, shape, lname), LATS[lname], rho_min)


def ten_of(rho, lattice):
    """the rows of xb_stencil_points for every voxel, [N, 10]"""
    return np.ascontiguousarray(restated_values(np.ascontiguousarray(rho, dtype=np.float64), lattice).reshape(10, -1).T)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def symmetric_density(shape):
    """200 - (d0^2 + d1^2 + d2^2), d_a = min(i_a, n_a - i_a): integers, even about 0 and n_a / 2 along every axis"""
    d = [np.minimum(np.arange(n), n - np.arange(n)).astype(np.float64) for n in shape]
    return 200.0 - (d[0][:, None, None] ** 2 + d[1][None, :, None] ** 2 + d[2][None, None, :] ** 2)


def symmetric_points(shape):
    """the 8 voxels whose coordinates are all in {0, n_a / 2}, as a mask"""
    at = np.zeros(shape, bool)
    at[np.ix_(*[[0, n // 2] for n in shape])] = True
    return at


def model_atoms(centres, n=48, a=12.0):
    """the sum of exp(-2 r) about `centres` on n^3 voxels of the cubic cell of edge a (no periodic images: they are below e^-20)"""
    p = (np.arange(n) * (a / n))
    X, Y, Z = np.meshgrid(p, p, p, indexing='ij')
    rho = np.zeros((n, n, n))
    for cx, cy, cz in centres:
        rho += np.exp(-2.0 * np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    return rho, np.eye(3) * a, (X, Y, Z)


# ---- the comparisons of tests/test_gpu_dori.py -------------------------------------------------------------------------------------
def sum_reference(v, lab, n, cuts=SUM_CUTS):
    """per key 3 a + class: ((fsum, count, fsum of magnitudes) of rho, the same of rho^2)"""
    k = keys(v, lab, n, cuts[0], cuts[2])
    return grouped(v['rho'], k, 3 * n), grouped(v['r2'], k, 3 * n)


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


# ---- 1. pybader_amd.dori against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize('rho_min', RHO_MINS)
@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', ['holes', 'rough', 'synth'])
def test_dori_value_equals_the_restatement_bit_for_bit(kind, shape, lname, rho_min):
    rho, v = density(kind, shape, lname), values(kind, shape, lname, rho_min)
    ten = ten_of(rho, LATS[lname])
    got = dori.dori_value(ten, rho_min)
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(v['gamma'].reshape(-1)))
    assert np.array_equal(bits(dori.colour_value(ten, rho_min)), bits(v['x'].reshape(-1)))
    g = v['gamma']
    assert (g >= 0).all() and (g <= 1).all() and not np.signbit(g).any()
    # gamma == 0 exactly where rho is +0, -0, negative or <= rho_min
    empty = ~(rho > rho_min)
    assert np.array_equal(g == 0, empty), (int((g == 0).sum()), int(empty.sum()))
    if kind == 'holes':
        assert (rho == 0).sum() > 10 and np.signbit(rho[rho == 0]).any() and (rho < 0).any()
    if rho_min == 0.05:      # (the synthetic background lies above 1e-3)
        assert ((rho > 0) & empty).any(), 'rho_min cuts voxels that hold density'
    assert not v['critical'].any(), 'no synthetic density reaches S == 0'
    for cuts in ((0.5, 0.03), (0.9, 0.01), (1.0, 0.0)):
        want = np.where(g >= cuts[0], classes(v, cuts[1]), -1).reshape(-1)
        pc = dori.point_classes(ten, cuts[0], rho_min, cuts[1])
        assert pc.dtype == np.int8 and np.array_equal(pc, want)


def test_a_constant_density_gives_zeros():
    for lname in LATS:
        for value in (0.03125, 7.0):
            rho = np.full((5, 6, 7), value)
            v = restated(rho, LATS[lname], 0.0)
            assert not v['gamma'].any() and not v['x'].any() and not v['S'].any() and not np.signbit(v['gamma']).any()
            assert not dori.dori_value(ten_of(rho, LATS[lname]), 0.0).any()
            assert (dori.point_classes(ten_of(rho, LATS[lname]), 0.5, 0.0, 0.01) == -1).all()


@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', SYMMETRIC_SHAPES)
def test_the_symmetric_integer_density_has_eight_exact_critical_points(shape, lname):
    """g = 0 exactly at the 8 voxels about which the density is even along every axis, and the Hessian is not zero there:
    S == 0, gamma == 1.0 -- and nowhere else"""
    rho = symmetric_density(shape)
    v = restated(rho, LATS[lname], 0.0)
    at = symmetric_points(shape)
    assert at.sum() == 8 and (rho > 0).all()
    assert np.array_equal(v['S'] == 0, at), 'S == 0 at exactly the 8 voxels'
    assert np.array_equal(v['critical'], at) and np.array_equal(v['gamma'] == 1.0, at)
    assert np.array_equal(bits(dori.dori_value(ten_of(rho, LATS[lname]), 0.0)), bits(v['gamma'].reshape(-1)))
    assert not restated(rho, LATS[lname], 200.0)['gamma'].any(), 'rho_min comes before the S == 0 rule'


@pytest.mark.parametrize('lname', list(LATS))
def test_powers_of_two_in_the_density_and_in_the_lattice_change_no_bit(lname):
    shape = (13, 17, 19)
    rho, lat = density('holes', shape, lname), LATS[lname]
    for rho_min in (0.0, 1e-3):
        base = restated(rho, lat, rho_min)
        for k in (-40, 30):
            s = restated(rho * 2.0 ** k, lat, rho_min * 2.0 ** k)
            assert np.array_equal(bits(s['gamma']), bits(base['gamma'])), k
            assert np.array_equal(bits(s['x']), bits(base['x'] * 2.0 ** k)), k
            assert np.array_equal(bits(dori.dori_value(ten_of(rho * 2.0 ** k, lat), rho_min * 2.0 ** k)), bits(base['gamma'].reshape(-1)))
        for k in (-3, 10):
            s = restated(rho, lat * 2.0 ** k, rho_min)
            assert np.array_equal(bits(s['gamma']), bits(base['gamma'])) and np.array_equal(bits(s['x']), bits(base['x'])), k
    assert (base['gamma'] > 0).sum() > 1000


def test_model_atoms():
    """a single exponential has k = grad rho / rho of constant length: theta = 0 in the continuum, and the stencil's gamma stays
    below 0.05 in the shell 1 < r < 3; between two atoms 1.5 apart the densities overlap and gamma is at least 0.9"""
    rho, lat, (X, Y, Z) = model_atoms([(6.1, 6.1, 6.1)])
    r = np.sqrt((X - 6.1) ** 2 + (Y - 6.1) ** 2 + (Z - 6.1) ** 2)
    shell = (r > 1) & (r < 3)
    g = restated(rho, lat, 0.0)['gamma']
    print(f'one atom: gamma <= {g[shell].max():.4f} over {int(shell.sum())} voxels of the shell 1 < r < 3')
    assert shell.sum() > 5000 and g[shell].max() < 0.05
    two, lat, _ = model_atoms([(6.1 - 0.75, 6.1, 6.1), (6.1 + 0.75, 6.1, 6.1)])
    g2 = restated(two, lat, 0.0)['gamma']
    print(f'two atoms: gamma = {g2[24, 24, 24]:.4f} at (24, 24, 24)')
    assert g2[24, 24, 24] >= 0.9
    assert np.array_equal(bits(dori.dori_value(ten_of(two, lat), 0.0)), bits(g2.reshape(-1)))


# ---- 2. what the sums' bound is worth ----------------------------------------------------------------------------------------------
def sum_values(kind, shape, lname):
    return values(kind, shape, lname, SUM_CUTS[1])


def test_every_class_holds_voxels_on_every_input_of_the_sums():
    for what, kind, shape, lname, lab, n in sum_inputs():
        k = keys(sum_values(kind, shape, lname), lab, n, SUM_CUTS[0], SUM_CUTS[2])
        per_class = [int(((k >= 0) & (k % 3 == c)).sum()) for c in range(3)]
        assert min(per_class) >= 57, (what, per_class)


def test_the_bound_notices_a_voxel_in_the_wrong_class_or_on_the_wrong_side():
    """one voxel of the region counted in another class of its label moves both keys' sums of rho and of rho^2 by more than the
    bound, and one voxel dropped from the region (a `>` for the `>=`, a bit of gamma) moves its key's -- on every input of the GPU
    sums, with a typical voxel of its key (the median density), not the largest"""
    seen = 0
    for what, kind, shape, lname, lab, n in sum_inputs():
        v = sum_values(kind, shape, lname)
        k = keys(v, lab, n, SUM_CUTS[0], SUM_CUTS[2])
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
            dropped = k.copy()
            dropped[vox] = -1
            s3, cnt3, _ = grouped(terms, dropped, 3 * n)
            assert abs(s3[a] - s[a]) * VV > lim[a] and cnt3[a] == cnt[a] - 1, (what, a)
        seen += 1
    assert seen == len(list(sum_inputs())) and seen >= 16


# ---- 3. ABI and errors -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


def test_header_and_binding_agree_on_the_dori_calls():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    want = {
        'xb_dori_field': ['xb_ctx *c', 'const double lattice[9]', 'double rho_min', 'int flags', 'double *g_host', 'double *x_host',
                          'void *g_dev', 'void *x_dev'],
        'xb_dori_sum': ['xb_ctx *c', 'const double lattice[9]', 'int64_t n', 'double voxel_volume', 'double d_cut', 'double rho_min',
                        'double rho_split', 'int flags', 'int64_t *count', 'double *charge', 'double *charge2'],
    }
    vp, pd, pi, i64, dbl, i = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int64, C.c_double, C.c_int
    types = {'xb_dori_field': [vp, pd, dbl, i, vp, vp, vp, vp], 'xb_dori_sum': [vp, pd, i64, dbl, dbl, dbl, dbl, i, pi, pd, pd]}
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, 'include/bader_hip.h does not declare ' + name
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and argtypes == types[name], name
    for method in ('dori_field', 'dori_sum'):
        assert callable(getattr(_lib.Context, method))
    # the definition is written down where the issue asks for it; no enumerator, timer slot, option key or block came with it
    assert 'N   = 4.0 * ((u0*u0 + u1*u1) + u2*u2)' in text and 'u_a = c*h_a - gg*g_a' in text and 'D   = (gg*gg)*gg' in text
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 26\.', design, flags=re.M)
    assert _lib.XB_TIMER_COUNT == 11 and not any(k.startswith(('XB_OPT_DORI', 'XB_TIMER_DORI', 'XB_DORI_')) for k in dir(_lib))
    blocks = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'ctx_buffers.h')).read()
    assert 'dori' not in blocks.lower(), 'the sums use the block of the NCI sums'
    assert LABELS_LDS == 85
    assert (dori.D_CUT, dori.RHO_MIN, dori.RHO_SPLIT) == (0.9, 1e-3, nci.RHO_SPLIT) and dori.E_PER_A3 == nci.E_PER_A3


def test_the_library_exports_the_calls_and_refuses_a_null_context(lib):
    lat = (C.c_double * 9)(*synth.CUBIC6.reshape(-1))
    out = np.full(4, -7.0)
    cnt = np.full(6, -7, np.int64)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert lib.xb_dori_field(None, lat, 0.0, 0, out.ctypes.data, out.ctypes.data, None, None) == _lib.XB_E_STATE
    assert lib.xb_dori_sum(None, lat, 2, 1.0, 0.5, 0.0, 0.01, 0, cnt.ctypes.data_as(pi), out.ctypes.data_as(pd),
                           out.ctypes.data_as(pd)) == _lib.XB_E_STATE
    assert (out == -7.0).all() and (cnt == -7).all(), 'a refused call writes nothing'


def test_bader_has_the_flags_and_they_are_off():
    from pybader_amd.interface import Bader
    assert Bader.dori_flag is False and Bader.dori_domains_flag is False
    assert callable(Bader.dori_analysis) and callable(Bader.dori_domain_analysis)
    assert (Bader.dori_cut, Bader.dori_rho_min, Bader.dori_rho_split) == (dori.D_CUT, dori.RHO_MIN, dori.RHO_SPLIT)


def test_the_python_layer_refuses_a_bound_outside_its_range():
    rho = np.full((4, 4, 4), 0.02)
    for bad in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError):
            dori.dori_isosurface(rho, np.eye(3), bad)
        with pytest.raises(ValueError):
            dori.dori_domains(rho, np.eye(3), level=bad)


def test_the_calls_need_the_gpu(lib):
    if lib.xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.full((4, 4, 4), 0.02)
    lab = np.zeros((4, 4, 4), np.int32)
    for call in (lambda: dori.dori_fields(rho, np.eye(3)), lambda: dori.dori_regions(rho, lab, np.eye(3), 1, 1.0),
                 lambda: dori.dori_isosurface(rho, np.eye(3)), lambda: dori.dori_domains(rho, np.eye(3)),
                 lambda: dori.bond_dori(rho, np.eye(3), [0])):
        with pytest.raises(_lib.BaderHipError):
            call()

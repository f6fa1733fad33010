"""The host side of the weight method (pybader_amd/weight.py) and the plain float64 restatement the GPU tests compare with.

voronoi_weights is checked on lattices whose Voronoi cell is known (cubic, orthorhombic, hexagonal, fcc-primitive), on a
generic triclinic one, against the identity  sum_d alpha_d r_d r_d^T = 2 V_voxel I  (every facet of a lattice Voronoi cell is
centred on r_d / 2, so the divergence theorem applied to the cell gives it without any clipping), and against
scipy.spatial.Voronoi where scipy is installed.

`restate` is steps 2-3 of the method as DESIGN.md states them: S in the neighbour order of the alpha table, then one loop over
the voxels in ascending rho with float64 scalars.  libbader_hip must reproduce it bit for bit (tests/test_gpu_weight.py).

THE BOUND of the conservation and symmetry checks, first order in u = 2**-53.  Exactly, sum_j J_ij = 1 for every voxel that is
no maximum, so every q_i ends up in the maxima: sum_m A_m = sum_i q_i.  In floating point a contribution crosses at most D - 1
voxels (D: the number of levels, the longest ascending chain) and at each one
    - S_i, a sum of up to 26 non-negative terms, carries a relative error of at most 25 u, and the division one more: the
      J_ij of a voxel sum to 1 within 26 u;
    - the product J_ji * A_j is rounded once and the running sum of q_i and up to 26 products up to 26 times: 27 u.
That is 53 u per voxel crossed, relative to the magnitude that flows, which never exceeds sum_i |q_i| to first order.  Adding the
M maxima costs (M - 1) u, math.fsum one more:
    |sum_m A_m - fsum(q)| <= (64 (D + 1) + M + 2) u sum_i |q_i|
(64 for 53: room for the second-order terms).  A single basin's A_m obeys the same bound, so two mirror-image basins differ by
at most twice it.  test_the_bound_notices_one_voxel shows what it is worth."""
import functools
import math

import numpy as np
import pytest

from pybader_amd.weight import voronoi_weights

U = 2.0 ** -53
STEP = (0, 1, -1)                       # step of table index 0 / 1 / 2
# voronoi_weights clips a square of half-width 4 max|r| -- some 16 facet diameters -- about 120 times: a vertex carries a few
# hundred u of the facet's size, an area and a weight some 10^3 u = 1e-13; RTOL leaves a factor of ten
RTOL = 1e-12

CUBIC = np.eye(3) * 0.1
ORTHO = np.diag([0.10, 0.16, 0.23])
HEX = np.array([[1.0, 0.0, 0.0], [-0.5, math.sqrt(3.0) / 2.0, 0.0], [0.0, 0.0, 1.3]]) * 0.1
FCC = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]) * 0.05
TRIC = np.array([[1.0, 0.1, 0.05], [0.2, 0.9, 0.1], [-0.1, 0.15, 1.1]]) * 0.1
LATTICES = {'cubic': CUBIC, 'ortho': ORTHO, 'hex': HEX, 'fcc': FCC, 'tric': TRIC}


@functools.lru_cache(maxsize=None)
def weights(name):
    a = voronoi_weights(LATTICES[name])
    a.flags.writeable = False
    return a


def offsets():
    for i in range(3):
        for j in range(3):
            for k in range(3):
                if (i, j, k) != (0, 0, 0):
                    yield (i, j, k), np.array([STEP[i], STEP[j], STEP[k]], dtype=np.float64)


# ---- voronoi_weights -----------------------------------------------------------------------------------------------------
def test_cubic_has_six_faces_of_weight_h():
    a = weights('cubic')
    faces = [(1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2)]
    for f in faces:
        assert abs(a[f] - 0.1) <= RTOL * 0.1, (f, a[f])
    assert np.count_nonzero(a) == 6


def test_orthorhombic_faces_are_area_over_length():
    a = weights('ortho')
    h = np.diag(ORTHO)
    for ax in range(3):
        want = h[(ax + 1) % 3] * h[(ax + 2) % 3] / h[ax]
        for s in (1, 2):
            idx = [0, 0, 0]
            idx[ax] = s
            assert abs(a[tuple(idx)] - want) <= RTOL * want
    assert np.count_nonzero(a) == 6


def test_hexagonal_has_eight_and_fcc_twelve_equal_faces():
    assert np.count_nonzero(weights('hex')) == 8
    f = weights('fcc')
    nz = f[f != 0]
    assert nz.size == 12 and np.ptp(nz) <= RTOL * nz.max()
    # rhombic dodecahedron of the fcc lattice with cubic constant c = 0.1: twelve faces of area c^2 sqrt(2) / 8 at distance c / sqrt(2)
    assert abs(nz[0] - (0.1 ** 2 * math.sqrt(2.0) / 8.0) / (0.1 / math.sqrt(2.0))) <= RTOL * nz[0]


def test_triclinic_has_fourteen_faces():
    assert np.count_nonzero(weights('tric')) == 14          # the generic Voronoi cell of a lattice: a truncated octahedron


@pytest.mark.parametrize('name', sorted(LATTICES))
def test_second_moment_identity_symmetry_and_centre(name):
    a, L = weights(name), LATTICES[name]
    vol = abs(np.linalg.det(L))
    T = np.zeros((3, 3))
    for idx, d in offsets():
        r = d @ L
        T += a[idx] * np.outer(r, r)
        neg = tuple((3 - i) % 3 for i in idx)
        assert a[idx] == a[neg] and a[idx] >= 0.0           # bit for bit: the device relies on it
    assert a[0, 0, 0] == 0.0
    assert np.abs(T - 2.0 * vol * np.eye(3)).max() <= 3 * RTOL * vol


@pytest.mark.parametrize('name', ['ortho', 'hex', 'tric'])
def test_permuting_the_lattice_rows_permutes_the_table(name):
    a, L = weights(name), LATTICES[name]
    for perm in ((1, 2, 0), (2, 1, 0)):
        b = voronoi_weights(L[list(perm)])
        np.testing.assert_allclose(b, np.transpose(a, perm), rtol=1e-12, atol=1e-15 * a.max())


def test_a_strongly_sheared_cell_is_refused():
    with pytest.raises(ValueError):
        voronoi_weights(np.array([[1.0, 0.0, 0.0], [3.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError):
        voronoi_weights(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.4, 1.7, 0.6]]))     # sheared along two axes, volume 0.6


@pytest.mark.parametrize('name', sorted(LATTICES))
def test_facet_areas_match_scipy(name):
    sp = pytest.importorskip('scipy.spatial')
    a, L = weights(name), LATTICES[name]
    pts = np.array([[i, j, k] for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)], dtype=np.float64)
    centre = int(np.flatnonzero((pts == 0).all(axis=1))[0])
    vor = sp.Voronoi(pts @ L)
    got = np.zeros((3, 3, 3))
    for (p, q), verts in zip(vor.ridge_points, vor.ridge_vertices):
        if centre not in (p, q):
            continue
        assert -1 not in verts, 'the central cell is bounded'
        d = pts[q if p == centre else p].astype(int)
        poly = vor.vertices[verts]
        n = (pts[q] - pts[p]) @ L
        n /= np.linalg.norm(n)
        u = np.cross(n, np.eye(3)[np.argmin(np.abs(n))])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        c = poly.mean(axis=0)
        ang = np.argsort(np.arctan2((poly - c) @ v, (poly - c) @ u))
        x, y = ((poly - c) @ u)[ang], ((poly - c) @ v)[ang]
        area = 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))
        if np.abs(d).max() > 1:
            assert area < 1e-10 * abs(np.linalg.det(L)) ** (2 / 3)
            continue
        got[tuple(d % 3)] = area / np.linalg.norm(d @ L)
    got[got < 1e-10 * abs(np.linalg.det(L)) ** (2 / 3) / np.linalg.norm(L, axis=1).max()] = 0.0
    np.testing.assert_allclose(got, a, rtol=1e-9, atol=1e-12 * a.max())


# ---- the restatement of flux and accumulation -------------------------------------------------------------------------------
def neighbour_tables(shape):
    """nb[n]: the linear index of voxel i + d_n for every voxel i (periodic), n the C-order index of the alpha table"""
    idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    nb = [None] * 27
    for n in range(1, 27):
        d = (STEP[n // 9], STEP[(n // 3) % 3], STEP[n % 3])
        nb[n] = np.roll(idx, tuple(-s for s in d), axis=(0, 1, 2)).reshape(-1)
    return nb


def restate(rho, q, alpha, labels=None):
    """(linear indices of the maxima ascending, A, V, number of levels): the weight method in plain float64.
    A voxel whose label is -1 is absent."""
    shape = rho.shape
    r = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
    al = np.asarray(alpha, dtype=np.float64).reshape(27)
    live = np.ones(r.size, bool) if labels is None else (np.asarray(labels).reshape(-1) != -1)
    nb = neighbour_tables(shape)
    used = [n for n in range(1, 27) if al[n] != 0.0]
    S = np.zeros(r.size)
    for n in used:                                           # S_i = sum_d f_ij, one rounding per offset, in table order
        up = r[nb[n]] - r
        S = S + np.where(live[nb[n]], al[n] * np.where(up > 0.0, up, 0.0), 0.0)
    S[~live] = -1.0
    rl, Sl, livel = r.tolist(), S.tolist(), live.tolist()
    A = np.ascontiguousarray(q, dtype=np.float64).reshape(-1).tolist()
    V = [1.0] * r.size
    level = [0] * r.size
    nbl = {n: nb[n].tolist() for n in used}
    all_ = [(n, float(al[n]), nbl[n]) for n in used]
    for i in np.argsort(r, kind='stable').tolist():          # ascending rho: every lower neighbour is finished
        if not livel[i]:
            continue
        acc, vol, lev, ri = A[i], 1.0, 1, rl[i]
        for n, a, tab in all_:
            j = tab[i]
            down = ri - rl[j]
            f = a * (down if down > 0.0 else 0.0)
            if f > 0.0 and livel[j]:
                J = f / Sl[j]
                acc = acc + J * A[j]
                vol = vol + J * V[j]
                lev = max(lev, level[j] + 1)
        A[i], V[i], level[i] = acc, vol, lev
    m = np.flatnonzero(live & (S == 0.0))
    return m, np.array(A)[m], np.array(V)[m], max(level) if level else 0


def bound(levels, n_maxima, mag):
    return (64 * (levels + 1) + n_maxima + 2) * U * mag


# ---- the densities both test files use (built once) -------------------------------------------------------------------------
def gaussians(shape, lattice, centres, widths, heights, background=0.01):
    """a sum of periodic (nearest image) Gaussians at fractional `centres`"""
    f = np.stack(np.meshgrid(*[np.arange(n) / n for n in shape], indexing='ij'), axis=-1)
    rho = np.full(shape, background)
    for c, w, h in zip(centres, widths, heights):
        d = f - np.asarray(c)
        d -= np.rint(d)
        r2 = ((d @ lattice) ** 2).sum(axis=-1)
        rho += h * np.exp(-r2 / (2.0 * w * w))
    return rho


def smooth_noise(shape, seed, passes=3):
    rng = np.random.default_rng(seed)
    a = rng.random(shape)
    for _ in range(passes):
        a = sum(np.roll(a, s, axis=ax) for ax in range(3) for s in (-1, 0, 1)) / 9.0
    return 1.0 + (a - a.min()) / (a.max() - a.min())


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (rho, lattice of the CELL, labels or None); arrays are read-only and shared"""
    labels = None
    if name == 'gauss2':                 # two equal Gaussians mirrored in the plane x = 8 (through voxel centres)
        shape, lat = (16, 16, 16), np.eye(3) * 4.0
        rho = gaussians(shape, lat, [(4 / 16, 0.5, 0.5), (12 / 16, 0.5, 0.5)], [0.5, 0.5], [2.0, 2.0])
        rho = 0.5 * (rho + rho[(-np.arange(16)) % 16])       # the mirror image bit for bit
    elif name == 'tric':
        shape, lat = (10, 12, 9), TRIC * np.array([[10], [12], [9]])
        rho = smooth_noise(shape, 3)
    elif name in ('thin325', 'thin147'):
        shape = (3, 2, 5) if name == 'thin325' else (1, 4, 7)
        lat = TRIC * np.array(shape)[:, None]
        rho = 1.0 + np.random.default_rng(5).random(shape)
    elif name == 'ramp':                 # about 200 levels of at most 16 voxels
        shape, lat = (4, 4, 200), np.diag([0.4, 0.4, 20.0])
        x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
        rho = 1.0 + 0.01 * z + 1e-6 * ((3 * x + 5 * y) % 7)
    elif name == 'vacuum':
        shape, lat = (24, 20, 28), np.diag([6.0, 5.0, 7.0])
        rho = gaussians(shape, lat, [(0.3, 0.4, 0.35), (0.7, 0.55, 0.7)], [0.7, 0.9], [3.0, 2.0], background=0.0)
        rho = rho * (1.0 + 0.05 * (smooth_noise(shape, 9) - 1.5))
        tol = np.quantile(rho, 1.0 / 3.0)
        labels = np.where(rho <= tol, -1, 0).astype(np.int32)
    elif name == 'quant8':
        shape, lat = (26, 25, 27), TRIC * np.array([[26], [25], [27]])
        rho = np.floor((smooth_noise(shape, 11, passes=1) - 1.0) * 7.999) / 8.0 + 0.5
    else:
        raise KeyError(name)
    rho = np.ascontiguousarray(rho)
    rho.flags.writeable = False
    if labels is not None:
        labels.flags.writeable = False
    return rho, lat, labels


def case_alpha(name):
    rho, lat, _ = case(name)
    return voronoi_weights(lat / np.array(rho.shape, dtype=np.float64)[:, None])     # row i of the cell over shape[i]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    rho, _, labels = case(name)
    return restate(rho, rho, case_alpha(name), labels)


def other_field(shape, seed=21):
    """an integrand of mixed sign that is not the partition field (exactly representable in float32)"""
    q = np.random.default_rng(seed).standard_normal(shape).astype(np.float32).astype(np.float64)
    q.flags.writeable = False
    return q


# ---- properties of the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['gauss2', 'tric', 'thin325', 'thin147', 'vacuum', 'quant8'])
def test_restatement_conserves_the_integrand(name):
    rho, _, labels = case(name)
    m, A, V, levels = case_reference(name)
    live = np.ones(rho.shape, bool) if labels is None else labels != -1
    assert m.size >= 1 and levels >= 1
    assert abs(math.fsum(A) - math.fsum(rho[live])) <= bound(levels, m.size, math.fsum(np.abs(rho[live])))
    assert abs(math.fsum(V) - int(live.sum())) <= bound(levels, m.size, float(live.sum()))
    q = other_field(rho.shape)
    m2, A2, _, _ = restate(rho, q, case_alpha(name), labels)
    assert np.array_equal(m, m2)
    assert abs(math.fsum(A2) - math.fsum(q[live])) <= bound(levels, m.size, math.fsum(np.abs(q[live])))


def test_restatement_case_shapes_are_what_the_gpu_tests_need():
    assert case_reference('gauss2')[0].size == 2
    assert case_reference('ramp')[3] >= 200                        # longer than one batch of level launches
    assert case_reference('quant8')[0].size >= 1000                # plateaus: every tied voxel is its own maximum
    _, _, labels = case('vacuum')
    assert 0.30 <= (labels == -1).mean() <= 0.36
    assert np.count_nonzero(case_alpha('tric')) == 14 and np.count_nonzero(case_alpha('gauss2')) == 6


def test_vacuum_voxels_neither_send_nor_receive():
    rho, _, labels = case('vacuum')
    m, A, V, _ = case_reference('vacuum')
    assert not (labels.reshape(-1)[m] == -1).any()
    m0, A0, _, _ = restate(rho, rho, case_alpha('vacuum'), None)
    assert m0.size != m.size or not np.array_equal(A0, A)          # the marks matter


def test_mirror_image_basins_get_equal_charges():
    rho, _, _ = case('gauss2')
    assert np.array_equal(rho, rho[(-np.arange(16)) % 16])
    m, A, V, levels = case_reference('gauss2')
    b = bound(levels, 2, math.fsum(np.abs(rho.reshape(-1))))
    assert abs(A[0] - A[1]) <= 2 * b and abs(V[0] - V[1]) <= 2 * bound(levels, 2, float(rho.size))
    assert abs(V[0] - rho.size / 2) <= 2 * bound(levels, 2, float(rho.size))


def test_the_bound_notices_one_voxel():
    rho, _, _ = case('gauss2')
    m, A, V, levels = case_reference('gauss2')
    b = bound(levels, m.size, math.fsum(np.abs(rho.reshape(-1))))
    assert b < 1e-6 * rho.min()                                    # losing the smallest voxel is a million bounds away

"""The host side of the moments per label (pybader_amd/multipole.py, xb_moment_sum) and the plain numpy restatement of the
definition in include/bader_hip.h / DESIGN.md section 13 that tests/test_gpu_multipole.py compares the kernels with.

`reference_terms` gives, per voxel, the ten terms and the image chosen; everything in it is elementwise IEEE float64 in the
order the definition writes, so the terms are the bits the device forms.  The sums are compared with math.fsum under the bound
of tests/test_gpu_sums.py, per label and component:

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

(count - 1 additions in any order and the multiply on the device, the rounding of fsum and of the reference's multiply).
test_the_bound_notices_a_wrong_image shows for every input of the GPU tests what that bound is worth: one voxel that takes its
second-nearest image moves a sum by more than it."""
import functools
import math
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, multipole
from soak_vs_oracle import ORTHO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
VV = 0.0371             # a voxel volume that is no power of two
TRIC = np.array([[5.0, 0.3, -0.2], [1.4, 6.1, 0.5], [-0.8, 1.2, 6.9]])
LATTICES = {'ortho': ORTHO, 'tric': TRIC}


def _define(name, text):
    return int(re.search(r'^#define %s (\d+)' % name, text, re.M).group(1))


with open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_common.h')) as _f:
    TPB = _define('TPB', _f.read())
try:
    with open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_moments.h')) as _f:
        _src = _f.read()
    MS_BINS, PER_THREAD = _define('MS_BINS', _src), _define('MS_PER_THREAD', _src)
except OSError:         # (the tests below then fail one by one instead of the module failing to import)
    MS_BINS, PER_THREAD = 0, 16
BLOCK = TPB * PER_THREAD        # voxels of one block, of either route


def shape_of(n):
    """the most cube-like (a, b, c) with a * b * c == n and every axis >= 3, or None"""
    best = None
    for a in range(3, int(round(n ** (1 / 3))) + 2):
        if n % a:
            continue
        for b in range(a, int(math.isqrt(n // a)) + 1):
            if (n // a) % b == 0 and (best is None or (a, b) > best[:2]):
                best = (a, b, n // a // b)
    return best


def shape_near(n, step):
    while shape_of(n) is None:
        n += step
    return shape_of(n)


SHORT, PAST = shape_near(BLOCK - 1, -1), shape_near(BLOCK + 1, 1)
SHAPES = [(3, 3, 3), (5, 7, 11), (13, 17, 19), SHORT, PAST]
SLAB = ((7, 11, 13), (2, 5))                 # an owned x-range inside the grid
CASES = [(s, None) for s in SHAPES] + [SLAB]
N_LABELS = [1, 2, MS_BINS - 1, MS_BINS, MS_BINS + 1, 3000]     # both sides of the LDS bin limit, and the global route far above it


# ---- inputs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def density(shape, seed=7):
    """mixed sign over nine decades with exact +0.0, -0.0 and a repeated value (the pattern of tests/test_gpu_sums.py)"""
    rng = np.random.default_rng(seed)
    rho = rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 3, shape)
    flat = rho.reshape(-1)
    idx, k = rng.permutation(flat.size), max(1, flat.size // 16)
    flat[idx[:k]] = 0.0
    flat[idx[k:2 * k]] = -0.0
    flat[idx[2 * k:4 * k]] = flat[idx[4 * k]]
    rho.flags.writeable = False
    return rho


def absent_label(n):
    return n // 2 if n >= 3 else None


@functools.lru_cache(maxsize=None)
def label_map(shape, n, seed=11):
    """int32 labels in [0, n) without absent_label(n), a tenth -1, some n, n + 7 and INT32_MAX"""
    rng = np.random.default_rng(seed + n)
    lab = rng.integers(0, n, shape).astype(np.int32)
    a = absent_label(n)
    if a is not None:
        lab[lab == a] = (a + 1) % n
    r = rng.random(shape)
    lab[r < 0.10] = -1
    lab[(r >= 0.10) & (r < 0.14)] = n
    lab[(r >= 0.14) & (r < 0.16)] = n + 7
    lab[(r >= 0.16) & (r < 0.17)] = np.iinfo(np.int32).max
    flat = lab.reshape(-1)
    flat[:4] = [-1, n, 0, n - 1]
    lab.flags.writeable = False
    return lab


@functools.lru_cache(maxsize=None)
def centres(shape, lname, n, seed=23):
    """n centres inside the cell; the first few on purpose: exactly on a voxel, on the cell corner, half a voxel from a face
    (equidistant from a voxel's two images in x up to rounding: ties and non-zero images occur)"""
    rng = np.random.default_rng(seed + n)
    lat = LATTICES[lname]
    frac = rng.random((n, 3))
    sh = np.array(shape, dtype=np.float64)
    special = [np.array([1, 2, 1]) / sh, np.zeros(3), np.array([0.5 / shape[0], 0.37, 0.61])]
    for k, f in enumerate(special[:n]):
        frac[(k * 7) % n if n > 2 else k] = f
    c = np.ascontiguousarray(frac @ lat)
    c.flags.writeable = False
    return c


# ---- the definition, restated -------------------------------------------------------------------------------------------------
IMAGES = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]     # the nesting order of the definition


def _positions(shape, lat):
    nx, ny, nz = shape
    p0, p1, p2 = (a.reshape(-1).astype(np.float64) for a in np.indices(shape))
    lat = np.asarray(lat, dtype=np.float64).reshape(9)
    pc = []
    for j in range(3):
        c = lat[j] * p0 / np.float64(nx)
        c = c + lat[3 + j] * p1 / np.float64(ny)
        c = c + lat[6 + j] * p2 / np.float64(nz)
        pc.append(c)
    return pc


def _image_vectors(pc, lat, cen, image):
    """e[j] of every voxel for the image index `image` (an int array, one per voxel)"""
    lat = np.asarray(lat, dtype=np.float64).reshape(9)
    xyz = np.array(IMAGES, dtype=np.float64)[image]
    out = []
    for j in range(3):
        pbc = (lat[j] * xyz[:, 0] + lat[3 + j] * xyz[:, 1]) + lat[6 + j] * xyz[:, 2]
        out.append(pc[j] - (cen[:, j] + pbc))
    return out


def _terms(w, d):
    t0, t1, t2 = w * d[0], w * d[1], w * d[2]
    return np.stack([w, t0, t1, t2, t0 * d[0], t0 * d[1], t0 * d[2], t1 * d[1], t1 * d[2], t2 * d[2]], axis=1)


def reference_terms(rho, labels, lattice, centres, second=False):
    """The definition in plain numpy.  -> (terms f64[N, 10], image int[N], label int64[N]) over all voxels in C order; a voxel
    whose label is outside [0, n) has label -1, image -1 and zero terms.  image indexes IMAGES (13 is (0, 0, 0)).
    `second`: every voxel takes its second-nearest image instead (what a wrong search would do; for the check of the check)."""
    shape = rho.shape
    n = centres.shape[0]
    w = np.asarray(rho, dtype=np.float64).reshape(-1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    ok = (lab >= 0) & (lab < n)
    a = np.where(ok, lab, 0)
    cen = np.asarray(centres, dtype=np.float64)[a]
    pc = _positions(shape, lattice)
    best = np.full(w.size, np.finfo(np.float64).max)
    which = np.zeros(w.size, dtype=np.int64)
    all_d2 = np.empty((27, w.size))
    for i in range(27):
        e = _image_vectors(pc, lattice, cen, np.full(w.size, i))
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        all_d2[i] = d2
        upd = d2 < best                      # strictly smaller: a tie keeps the earlier image
        best = np.where(upd, d2, best)
        which = np.where(upd, i, which)
    if second:
        all_d2[which, np.arange(w.size)] = np.inf
        which = np.argmin(all_d2, axis=0)
    terms = _terms(w, _image_vectors(pc, lattice, cen, which))
    terms[~ok] = 0.0
    return terms, np.where(ok, which, -1), np.where(ok, lab, -1)


def grouped(terms, label, n, x_range=None, shape=None):
    """per label and component: (fsum of the terms, count, fsum of |terms|) over the owned voxels"""
    if x_range is not None:
        own = np.zeros(shape, bool)
        own[x_range[0]:x_range[1]] = True
        label = np.where(own.reshape(-1), label, -1)
    keep = np.flatnonzero(label >= 0)
    order = keep[np.argsort(label[keep], kind='stable')]
    vals, starts = np.unique(label[order], return_index=True)
    s, cnt, mag = np.zeros((n, 10)), np.zeros(n, np.int64), np.zeros((n, 10))
    for a, lo, hi in zip(vals, starts, list(starts[1:]) + [order.size]):
        x = terms[order[lo:hi]]
        cnt[a] = hi - lo
        for k in range(10):
            s[a, k], mag[a, k] = math.fsum(x[:, k]), math.fsum(np.abs(x[:, k]))
    return s, cnt, mag


def bound(count, mag, vv=1.0):
    return (np.asarray(count)[..., None] + 2) * U * mag * abs(vv)


@functools.lru_cache(maxsize=None)
def reference(shape, x_range, lname, n):
    """(terms, image, label, fsum, count, magnitude) of one input of the GPU tests, computed once"""
    terms, image, label = reference_terms(density(shape), label_map(shape, n), LATTICES[lname], centres(shape, lname, n))
    s, cnt, mag = grouped(terms, label, n, x_range, shape)
    for a in (terms, image, label, s, cnt, mag):
        a.flags.writeable = False
    return terms, image, label, s, cnt, mag


def inputs():
    for shape, x_range in CASES:
        for lname in LATTICES:
            for n in N_LABELS:
                yield shape, x_range, lname, n


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_moment_sum():
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+xb_moment_sum\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'include/bader_hip.h does not declare xb_moment_sum'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['xb_ctx *c', 'const double lattice[9]', 'const double *centres_cart', 'int64_t n', 'double voxel_volume',
                    'double *moments', 'double *volume']
    res, argtypes = _lib.SYMBOLS['xb_moment_sum']
    pd = C.POINTER(C.c_double)
    assert res is C.c_int and argtypes == [C.c_void_p, pd, pd, C.c_int64, C.c_double, pd, pd]
    assert callable(getattr(_lib.Context, 'moment_sum'))
    assert MS_BINS >= 8 and MS_BINS * 84 * 8 <= 160 * 1024, 'eight blocks of bins fit the LDS of a compute unit'


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.multipole_flag is False and callable(Bader.multipole_moments)


# ---- second_moment, dipole, quadrupole ------------------------------------------------------------------------------------------
def test_matrices_of_hand_made_rows():
    rows = np.array([[2.0, 0.5, -0.25, 0.125, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0],
                     [1.0, 0.0, 0.0, -0.0, 0.1, 0.0, 0.0, 0.1, 0.0, 0.1],
                     [3.0, 1.0, 2.0, 3.0, 1e-3, 7.0, -2.0, 0.3, 0.25, -1e5]])
    m2 = multipole.second_moment(rows)
    assert m2.shape == (3, 3, 3) and np.array_equal(m2, m2.transpose(0, 2, 1))
    assert np.array_equal(m2[0], [[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 5.0, 6.0]])
    d = multipole.dipole(rows)
    assert np.array_equal(d[0], [-0.5, 0.25, -0.125]) and d.shape == (3, 3)        # electrons count positive: -m1
    q = multipole.quadrupole(rows)
    assert np.array_equal(q, q.transpose(0, 2, 1))
    # -(3 m2 - tr I): row 0 has tr = 11
    assert np.array_equal(q[0], -(3.0 * m2[0] - 11.0 * np.eye(3)))
    assert np.array_equal(q[1], np.zeros((3, 3))), 'an isotropic m2 has no quadrupole, to the last bit'
    tr = q[:, 0, 0] + q[:, 1, 1] + q[:, 2, 2]
    assert tr[0] == 0.0 and tr[1] == 0.0
    scale = np.abs(m2[2]).max() * 3
    assert abs(tr[2]) <= 8 * U * scale
    np.testing.assert_allclose(q[2], -(3.0 * m2[2] - np.trace(m2[2]) * np.eye(3)), rtol=0, atol=8 * U * scale)
    one = multipole.second_moment(rows[0])
    assert one.shape == (1, 3, 3)


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
def test_reference_terms_on_a_case_done_by_hand():
    """2 x 1 x 1... too thin for the library, so (3, 3, 3), cubic cell of edge 3 (voxels at integers), one centre at (2.5, 0, 0):
    voxel (0, 0, 0) is nearer to the centre's image at -0.5 (x = -1) than to 2.5; voxel (1, 0, 0) is equally far from both and
    keeps the EARLIER image, x = -1"""
    lat = np.eye(3) * 3.0
    rho = np.arange(1.0, 28.0).reshape(3, 3, 3)
    lab = np.zeros((3, 3, 3), np.int32)
    lab[2, 2, 2] = 5
    terms, image, label = reference_terms(rho, lab, lat, np.array([[2.5, 0.0, 0.0]]))
    assert IMAGES[13] == (0, 0, 0) and IMAGES[4] == (-1, 0, 0)
    assert image[0] == 4 and np.array_equal(terms[0], [1.0, 0.5, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0])
    v = 9                                        # voxel (1, 0, 0), rho 10: d = 1 - (2.5 - 3) = 1.5 (image -1) or 1 - 2.5 = -1.5
    assert image[v] == 4 and np.array_equal(terms[v, :5], [10.0, 15.0, 0.0, 0.0, 22.5])
    v = 18                                       # voxel (2, 0, 0): d = -0.5 in the home image
    assert image[v] == 13 and terms[v, 1] == -0.5 * 19.0
    assert label[26] == -1 and image[26] == -1 and not terms[26].any()
    far, image2, _ = reference_terms(rho, lab, lat, np.array([[2.5, 0.0, 0.0]]), second=True)
    assert image2[0] == 13 and far[0, 1] == -2.5


# ---- the check of the check -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,x_range', CASES)
def test_the_bound_notices_a_wrong_image(shape, x_range):
    """for every input of the GPU tests: the owned labelled voxel of median |rho| (zeros aside), moved to its second-nearest
    image, changes one of its label's ten sums by more than twice that label's bound -- and the voxels are not huddled around
    their centres: a tenth of them and more take an image other than (0, 0, 0)"""
    assert MS_BINS, 'csrc/k_moments.h is missing'
    for lname in LATTICES:
        for n in N_LABELS:
            terms, image, label, s, cnt, mag = reference(shape, x_range, lname, n)
            far, image2, _ = reference_terms(density(shape), label_map(shape, n), LATTICES[lname], centres(shape, lname, n), second=True)
            own = label >= 0
            if x_range is not None:
                mask = np.zeros(shape, bool)
                mask[x_range[0]:x_range[1]] = True
                own &= mask.reshape(-1)
            assert own.sum() == cnt.sum() and own.sum() >= 12
            assert np.all(image2[own] != image[own])
            away = (image[own] != 13).mean()
            assert away >= 0.1, (lname, n, away)
            w = np.abs(density(shape).reshape(-1))
            cand = np.flatnonzero(own & (w > 0))
            v = cand[np.argsort(w[cand], kind='stable')[cand.size // 2]]
            a = label[v]
            shift = np.abs(far[v] - terms[v]) * VV
            lim = bound(cnt[a], mag[a], VV)
            assert np.any(shift > 2 * lim), (lname, n, int(v), shift, lim)
            # and the sums themselves obey the bound against a plain sequential sum (the restatement is self-consistent)
            seq = np.array([np.sum(terms[label == a][:, k]) for k in range(10)]) if x_range is None else None
            if seq is not None:
                assert np.all(np.abs(seq * VV - s[a] * VV) <= lim)


def test_inputs_reach_both_routes_and_the_edges_of_a_block():
    vox = [int(np.prod(s)) for s in SHAPES]
    assert vox[0] == 27 and vox[1] < BLOCK // 4 and vox[2] > BLOCK
    assert BLOCK - 16 <= int(np.prod(SHORT)) < BLOCK < int(np.prod(PAST)) <= BLOCK + 16
    assert {MS_BINS - 1, MS_BINS, MS_BINS + 1} <= set(N_LABELS) and max(N_LABELS) >= 1000
    assert any(v % 64 for v in vox)
    # ties occur: a centre half a voxel from the x = 0 face is as far from plane 0 as its image at +a is from ... plane 1
    _, image, label, *_ = reference((13, 17, 19), None, 'ortho', 2)
    assert len(set(image[label >= 0])) >= 8

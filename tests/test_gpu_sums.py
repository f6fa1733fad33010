"""The kernels of csrc/k_sums.h (and k_vacuum_assign) on inputs the assignment never produces, each against plain numpy restated
here: densities of mixed sign over nine decades with exact +0.0, -0.0 and repeated values, random label maps with -1, labels at
and above n_labels and labels nobody carries, an owned x-range that is not the whole grid, every label dtype in and out.

Sums are compared with math.fsum (correctly rounded) under the first-order bound for adding `count` doubles in ANY order and
one multiply by the voxel volume:

    |got - fsum * vv| <= (count + 2) * 2**-53 * sum(|rho|) * |vv|

(count - 1 additions and the multiply on the device, the rounding of fsum and of the reference's multiply: count + 2
roundings, each at most 2**-53 of a partial result no larger than sum(|rho|) * |vv|).  Counts, volumes, maps and masks are exact.
test_the_bound_notices_one_voxel shows on the CPU what the bound is worth."""
import functools
import math
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform
from soak_vs_oracle import ORTHO

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_common.h')) as _f:
    TPB = int(re.search(r'^#define TPB (\d+)', _f.read(), re.M).group(1))
BLOCK = TPB * 16        # voxels of one block of the LDS route of xb_charge_sum (16 per thread)
CS_BINS = 1024          # n_labels above it: the global-atomics route
U = 2.0 ** -53
VV = 0.0371             # a voxel volume that is no power of two
INTS = (np.int8, np.int16, np.int32, np.int64)


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


SHORT, PAST = shape_near(BLOCK - 1, -1), shape_near(BLOCK + 1, 1)   # one voxel less / more than one full block (TPB 256: 4095, 4100)
SHAPES = [(3, 3, 3), (5, 7, 11), (13, 17, 19), (16, 16, 17), SHORT, PAST]
SLAB = ((7, 11, 13), (2, 5))     # an owned x-range inside the grid
N_LABELS = [1, 2, 1023, 1024, 1025, 5000]


@functools.lru_cache(maxsize=None)
def density(shape, seed=7):
    rng = np.random.default_rng(seed)
    rho = rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 3, shape)
    flat = rho.reshape(-1)
    idx, k = rng.permutation(flat.size), max(1, flat.size // 16)
    flat[idx[:k]] = 0.0
    flat[idx[k:2 * k]] = -0.0
    flat[idx[2 * k:4 * k]] = flat[idx[4 * k]]       # a value that occurs 2k + 1 times
    rho.flags.writeable = False
    return rho


def repeated_value(shape):
    vals, counts = np.unique(density(shape), return_counts=True)
    return float(vals[np.argmax(counts * (vals != 0))])


@functools.lru_cache(maxsize=None)
def label_map(shape, n_labels, seed=11):
    """int32 labels in [0, n_labels) without `absent_label(n_labels)`, a tenth -1, some n_labels, n_labels + 7 and INT32_MAX"""
    rng = np.random.default_rng(seed + n_labels)
    lab = rng.integers(0, n_labels, shape).astype(np.int32)
    a = absent_label(n_labels)
    if a is not None:
        lab[lab == a] = (a + 1) % n_labels
    r = rng.random(shape)
    lab[r < 0.10] = -1
    lab[(r >= 0.10) & (r < 0.14)] = n_labels
    lab[(r >= 0.14) & (r < 0.16)] = n_labels + 7
    lab[(r >= 0.16) & (r < 0.17)] = np.iinfo(np.int32).max
    flat = lab.reshape(-1)
    flat[:4] = [-1, n_labels, 0, n_labels - 1]      # (present in the smallest grid as well)
    lab.flags.writeable = False
    return lab


def absent_label(n_labels):
    return n_labels // 2 if n_labels >= 3 else None


def grouped(rho, lab, n_labels):
    """per label in [0, n_labels): (fsum, count, sum of |rho|) over the voxels that carry it"""
    rho, lab = rho.reshape(-1), lab.reshape(-1)
    keep = np.flatnonzero((lab >= 0) & (lab < n_labels))
    order = keep[np.argsort(lab[keep], kind='stable')]
    vals, starts = np.unique(lab[order], return_index=True)
    s, n, mag = np.zeros(n_labels), np.zeros(n_labels, np.int64), np.zeros(n_labels)
    for a, lo, hi in zip(vals, starts, list(starts[1:]) + [order.size]):
        x = rho[order[lo:hi]]
        s[a], n[a], mag[a] = math.fsum(x), hi - lo, math.fsum(np.abs(x))
    return s, n, mag


def bound(count, mag, vv=1.0):
    return (count + 2) * U * mag * abs(vv)


def setup(ctx, shape, x_range=None):
    vl = np.divide(ORTHO, shape)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl), x_range)
    if x_range is not None:
        ctx.set_halo(2)          # (a logical rank, as pybader_amd.slab.GpuBackend sets one up)
    ctx.upload_density(density(shape))


def owned(a, x_range):
    return a if x_range is None else a[x_range[0]:x_range[1]]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


CASES = [(s, None) for s in SHAPES] + [SLAB]


# ---- the check of the check: CPU only ----------------------------------------------------------------------------------------
def test_the_bound_notices_one_voxel():
    """a label of some 3 600 voxels of (13, 17, 19): the fsum with one voxel left out, or counted twice, violates the bound --
    for the voxel of median magnitude, and for 95% of all voxels that are not an exact zero (the rest are the few whose
    magnitude lies under the rounding of the sum itself)"""
    shape = (13, 17, 19)
    rho, lab = density(shape), label_map(shape, 1)
    s, n, mag = grouped(rho, lab, 1)
    assert n[0] > 3000
    x = rho[lab == 0]
    b = bound(n[0], mag[0], VV)
    assert abs(s[0] * VV - math.fsum(x) * VV) <= b
    nz = np.flatnonzero(x)
    mid = nz[np.argsort(np.abs(x[nz]))[nz.size // 2]]
    assert abs(math.fsum(np.delete(x, mid)) * VV - s[0] * VV) > b
    assert abs(math.fsum(np.append(x, x[mid])) * VV - s[0] * VV) > b
    caught = np.abs(x[nz]) * VV > 2 * b              # (dropping x changes the sum by |x|; 2b: beyond the bound either side)
    assert caught.mean() >= 0.95, caught.mean()
    assert mag[0] / n[0] * VV > 1e5 * b              # a voxel of the label's mean magnitude: five decades above the bound


def test_shapes_reach_the_edges_of_a_block():
    n = [int(np.prod(s)) for s in SHAPES]
    assert n[0] == 27 and n[1] < BLOCK // 4
    assert BLOCK - 16 <= int(np.prod(SHORT)) < BLOCK < int(np.prod(PAST)) <= BLOCK + 16
    if TPB == 256:
        assert n[2] == BLOCK + 103 and n[3] == BLOCK + TPB
    assert any(v % 16 for v in n) and CS_BINS in N_LABELS and CS_BINS + 1 in N_LABELS


# ---- xb_charge_sum -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape,x_range', CASES)
def test_charge_sum(ctx, shape, x_range):
    setup(ctx, shape, x_range)
    rho = density(shape)
    for n_labels in N_LABELS:
        lab = label_map(shape, n_labels)
        ctx.upload_labels(lab)
        charge, volume = ctx.charge_sum(VV, n_labels)
        s, n, mag = grouped(owned(rho, x_range), owned(lab, x_range), n_labels)
        assert np.array_equal(volume, n.astype(np.float64) * VV), f'n_labels {n_labels}: volumes'
        err, lim = np.abs(charge - s * VV), bound(n, mag, VV)
        worst = int(np.argmax(err - lim))
        assert np.all(err <= lim), f'n_labels {n_labels}: label {worst} ({n[worst]} voxels) off by {err[worst]:.3e}, bound {lim[worst]:.3e}'
        a = absent_label(n_labels)
        if a is not None:
            assert n[a] == 0 and charge[a] == 0.0 and volume[a] == 0.0
        assert np.all(charge[n == 0] == 0.0)         # (nothing out of range lands anywhere)


@gpu
def test_charge_sum_of_one_big_label_is_tighter_than_one_voxel(ctx):
    """label 0 of (13, 17, 19) with n_labels = 1, on the card: the kernel's sum lies within the bound, the same sum short of its
    median voxel does not"""
    shape = (13, 17, 19)
    setup(ctx, shape)
    rho, lab = density(shape), label_map(shape, 1)
    ctx.upload_labels(lab)
    charge, _ = ctx.charge_sum(VV, 1)
    s, n, mag = grouped(rho, lab, 1)
    x = rho[lab == 0]
    mid = np.argsort(np.abs(x))[x.size // 2]
    assert abs(charge[0] - s[0] * VV) <= bound(n[0], mag[0], VV) < abs(charge[0] - math.fsum(np.delete(x, mid)) * VV)


# ---- xb_label_sum ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape,x_range', CASES)
def test_label_sum(ctx, shape, x_range):
    setup(ctx, shape, x_range)
    n_labels = 5
    lab = label_map(shape, n_labels)
    ctx.upload_labels(lab)
    rho_o, lab_o = owned(density(shape), x_range), owned(lab, x_range)
    for value in (-1, 0, n_labels - 1, absent_label(n_labels), n_labels, n_labels + 1):
        x = rho_o[lab_o == value]
        got, count = ctx.label_sum(value)
        assert count == x.size, value
        assert abs(got - math.fsum(x)) <= bound(x.size, math.fsum(np.abs(x))), value
        if value in (absent_label(n_labels), n_labels + 1):
            assert count == 0 and got == 0.0


# ---- xb_vacuum_assign --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape,x_range', CASES)
def test_vacuum_assign(ctx, shape, x_range):
    setup(ctx, shape, x_range)
    rho = density(shape)
    for tol in (repeated_value(shape), -abs(repeated_value(shape)), -1e-3, 0.0, None):
        ctx.upload_labels(label_map(shape, 3))       # (something else than the answer)
        charge, volume = ctx.vacuum_assign(tol, VV)
        want = np.where(rho <= (np.nan if tol is None else tol), -1, 0)
        assert np.array_equal(ctx.download_labels(np.int32), want), tol
        x = owned(rho, x_range)[owned(want, x_range) == -1]
        assert volume == float(x.size) * VV, tol
        assert abs(charge - math.fsum(x) * VV) <= bound(x.size, math.fsum(np.abs(x)), VV), tol
        if tol is None:
            assert charge == 0.0 and volume == 0.0
        else:
            assert 0 < np.count_nonzero(want) < want.size      # (both sides of the rule occur)
    t = repeated_value(shape)
    assert np.count_nonzero(rho == t) > 1 and np.any(rho < t) and np.any(rho > t)


# ---- xb_volume_mask ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_volume_mask(ctx, shape):
    setup(ctx, shape)
    rho, lab = density(shape), label_map(shape, 4)
    ctx.upload_labels(lab)
    at_neg0 = int(lab[np.signbit(rho) & (rho == 0)][0])             # the label of a -0.0 voxel: its mask keeps the sign bit
    for k in (at_neg0, 0, 3, absent_label(4), -1, 4, 5):
        want = np.where(lab == k, rho, 0.0)
        assert k != at_neg0 or np.any(want.view(np.uint64) == 1 << 63)
        assert np.array_equal(ctx.volume_mask(k).view(np.uint64), want.view(np.uint64)), k


@gpu
def test_volume_mask_on_a_slab_whose_scratch_is_smaller_than_the_grid(ctx):
    """a logical rank of 8 planes on a grid of 9.4 million voxels: its `stage` (64 MiB) does not hold the grid's 72 MiB of
    doubles -- xb_volume_mask used to write all of them into it; now it goes through `stage` a chunk at a time"""
    shape = (1024, 96, 96)
    rng = np.random.default_rng(5)
    rho = rng.standard_normal(shape)
    lab = rng.integers(-1, 3, shape).astype(np.int8)
    c = _lib.Context(0)
    try:
        vl = np.divide(ORTHO, shape)
        c.set_grid(shape, distance_matrix(vl), gradient_transform(vl), (0, 8))
        c.set_halo(2)
        scratch = c.memory_stats()[2]
        c.upload_density(rho)
        c.upload_labels(lab)
        got = c.volume_mask(1)
    finally:
        c.close()
    assert scratch < rho.nbytes        # (list and stage together: the grid's doubles do not fit)
    assert np.array_equal(got.view(np.uint64), np.where(lab == 1, rho, 0.0).view(np.uint64))


# ---- xb_volume_assign --------------------------------------------------------------------------------------------------------
def swapped(lab, swap):
    hit = (lab >= 0) & (lab < len(swap))
    return np.where(hit, np.asarray(swap)[np.where(hit, lab, 0)], lab)


@gpu
@pytest.mark.parametrize('shape,x_range', CASES)
def test_volume_assign(ctx, shape, x_range):
    """several labels onto one, one onto 0, labels at and above the table's length and -1 untouched -- also after a LONGER
    table has been through the same buffer; outside the owned planes nothing changes"""
    setup(ctx, shape, x_range)
    n_swap = 9
    rng = np.random.default_rng(3)
    lab = rng.integers(-1, n_swap + 3, shape).astype(np.int32)
    lab.reshape(-1)[:5] = [-1, 0, n_swap - 1, n_swap, n_swap + 2]
    long_table = [40 + i for i in range(n_swap + 3)]
    swap = [5, 5, 5, 0, 7, 2, 1, 8, 3]
    for table in (long_table, swap):
        ctx.upload_labels(lab)
        ctx.volume_assign(table)
        want = lab.copy()
        owned(want, x_range)[...] = swapped(owned(lab, x_range), table)
        for dt in INTS:
            assert np.array_equal(ctx.download_labels(dt), want.astype(dt)), (len(table), dt)
    assert np.any(want == n_swap) and np.any(want == n_swap + 2) and np.any(want == -1)


# ---- k_widen / k_narrow / k_narrow_vec ---------------------------------------------------------------------------------------
def page_locked(shape, dtype):
    """an array of `shape` at the front of a pooled page-locked buffer (the pool hands out pageable memory below 1 MiB)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = _lib.pinned_empty((max(nbytes, 1 << 20),), np.uint8)
    assert _lib.pool_owned(buf), 'no page-locked memory from the pool'
    return buf[:nbytes].view(dtype).reshape(shape)


def cast_source(shape, dtype, seed=13):
    """every extreme of every narrower type, the values either side of them, and random values of `dtype` (int64: of int32)"""
    rng = np.random.default_rng(seed)
    info = np.iinfo(np.int32 if dtype == np.int64 else dtype)
    special = [v for t in (np.int8, np.int16, np.int32) for e in (np.iinfo(t).min, np.iinfo(t).max) for v in (e - 1, e, e + 1)]
    special = np.array([v for v in special + [0, -1, 1, 255, 256, 65535, 65536] if info.min <= v <= info.max], np.int64)
    src = rng.integers(info.min, info.max, shape, dtype=np.int64, endpoint=True)
    flat = src.reshape(-1)
    pick = rng.permutation(flat.size)[:flat.size // 2]
    flat[pick] = rng.choice(special, pick.size)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    return src.astype(dtype)


# 27 voxels: the smallest grid there is (one 16-byte group of int8 and 11 behind it; three of int16 and 3 behind them -- no grid
# has fewer than 16 voxels, so "no whole group" cannot occur); 385 = 24 * 16 + 1; 1 113 121 = 16 k + 1 voxels: an int8 map of
# more than 1 MiB, which download_labels(pooled=True) itself puts into page-locked memory
@gpu
@pytest.mark.parametrize('shape', [(3, 3, 3), (5, 7, 11), (101, 103, 107)])
def test_label_casts(ctx, shape):
    n = int(np.prod(shape))
    assert n % 16 and n % 8
    vl = np.divide(ORTHO, shape)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    for st in INTS:
        src = cast_source(shape, st)
        ctx.upload_labels(src)
        for dt in INTS:
            want = src.astype(np.int32).astype(dt)
            assert np.array_equal(ctx.download_labels(dt), want), (st, dt, 'pageable')
            got = ctx.download_labels(dt, pooled=True)
            assert got.dtype == dt and np.array_equal(got, want), (st, dt, 'pooled')
            assert _lib.pool_owned(got) == (want.nbytes >= 1 << 20)
            out = page_locked(shape, dt)
            out[...] = 85
            assert ctx.download_labels(dt, out=out) is out and np.array_equal(out, want), (st, dt, 'page-locked')
            del got, out


# ---- xb_surface_distance -----------------------------------------------------------------------------------------------------
def atom_map(shape, n_atoms, seed):
    """blocky Voronoi cells of n_atoms random sites (atom 0 on a grid point), the cell of atom `n_atoms // 2` handed to the
    vacuum, 5% more -1 voxels; -> labels int32, fractional sites"""
    rng = np.random.default_rng(seed)
    frac = rng.random((n_atoms, 3))
    frac[0] = np.array([1, 2, 1]) / np.array(shape)
    grid = np.stack(np.meshgrid(*[np.arange(s) / s for s in shape], indexing='ij'), -1)
    d = grid[..., None, :] - frac
    d -= np.round(d)
    lab = np.argmin((d ** 2).sum(-1), -1).astype(np.int32)
    lab[lab == n_atoms // 2] = -1
    lab[rng.random(shape) < 0.05] = -1
    return lab, frac


@gpu
@pytest.mark.parametrize('lname', ['orthorhombic', 'triclinic'])
@pytest.mark.parametrize('shape,n_atoms', [((5, 7, 11), 6), ((13, 17, 19), 9), ((16, 16, 17), 4), ((6, 6, 6), 60)])
def test_surface_distance(ctx, shape, n_atoms, lname):
    """(6, 6, 6) with 60 atoms: lattice + atoms + minima are 256 doubles, the grid's worth of `stage` 216 -- the scratch floor of
    need_scratch holds them"""
    from oracle_context import OracleContext
    lat = {'orthorhombic': ORTHO, 'triclinic': synth.TRICLINIC}[lname]
    vl = np.divide(lat, shape)
    dm, tg = distance_matrix(vl), gradient_transform(vl)
    lab, frac = atom_map(shape, n_atoms, 17)
    atoms = frac @ lat
    rho = density(shape)
    if n_atoms == 60:
        assert 16 + 4 * n_atoms > lab.size
    ref = OracleContext()
    ref.set_grid(shape, dm, tg)
    ref.upload_density(rho)
    ref.upload_labels(lab)
    want, want_edges = ref.surface_distance(lat, atoms)
    ctx.set_grid(shape, dm, tg)
    ctx.upload_density(rho)
    ctx.upload_labels(lab)
    got, edges = ctx.surface_distance(lat, atoms)
    assert edges == want_edges and 0 < edges < lab.size
    assert np.isposinf(want[n_atoms // 2]) and np.array_equal(np.isposinf(got), np.isposinf(want))
    fin = np.isfinite(want)
    assert fin.any() and np.all(got[fin] >= 0)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=1e-12 * np.abs(lat).max() ** 2)


@gpu
def test_synth_density_with_more_atoms_than_the_grid_has_room_for(ctx):
    """8 atoms on 3 x 3 x 3: the atom table (56 doubles) is larger than the grid's worth of `stage` (27); the scratch floor holds
    it, and the density equals the oracle's"""
    import oracle
    shape = (3, 3, 3)
    vl = np.divide(synth.TRICLINIC, shape)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    ctx.synth_density(synth.TRICLINIC, synth.ATOMS8, synth.BACKGROUND)
    assert 16 + 5 * len(synth.ATOMS8) > 27
    assert ctx.memory_stats()[2] >= 4 << 20
    assert np.array_equal(ctx.download_density(), oracle.synth_density(shape, synth.TRICLINIC, np.asarray(synth.ATOMS8, np.float64), synth.BACKGROUND))

"""xb_moment_sum and what stands on it (-m gpu) against the numpy restatement of tests/test_multipole_cpu.py.

THE BOUND, per label and component (tests/test_gpu_sums.py gives the reason: count - 1 additions in any order and one multiply
on the device, the rounding of fsum and of the reference's multiply):

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

The terms themselves are bit-defined, so nothing else enters.  Volumes (counts) are exact.
tests/test_multipole_cpu.py::test_the_bound_notices_a_wrong_image shows for every input used here that one voxel with a wrong
image breaks this bound."""
import ctypes as C

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, device, multipole, synth, utils
from pybader_amd.interface import Bader, distance_matrix, gradient_transform
from test_multipole_cpu import (BLOCK, CASES, LATTICES, MS_BINS, N_LABELS, VV, bound, centres, density, grouped, label_map,
                                reference, reference_terms)

pytestmark = pytest.mark.gpu
INTS = (np.int8, np.int16, np.int32, np.int64)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def setup(ctx, shape, lname, x_range=None, rho=None):
    vl = np.divide(LATTICES[lname], shape)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl), x_range)
    if x_range is not None:
        ctx.set_halo(2)          # (a logical rank, as pybader_amd.slab.GpuBackend sets one up)
    ctx.upload_density(density(shape) if rho is None else rho)


def check(got, volume, s, cnt, mag, what):
    """the bound for every label and component (each figure printed before it is asserted), exact volumes"""
    assert got.shape == s.shape and volume.shape == cnt.shape
    assert np.array_equal(volume, cnt.astype(np.float64) * VV), f'{what}: volumes'
    err, lim = np.abs(got - s * VV), bound(cnt, mag, VV)
    a, k = np.unravel_index(int(np.argmax(err - lim)), err.shape)
    print(f'{what}: worst label {a} component {k} ({cnt[a]} voxels): off by {err[a, k]:.3e}, bound {lim[a, k]:.3e}')
    assert np.all(err <= lim), f'{what}: label {a} component {k} ({cnt[a]} voxels) off by {err[a, k]:.3e}, bound {lim[a, k]:.3e}'
    assert not got[cnt == 0].any(), f'{what}: something landed on a label nobody carries'


# ---- against reference_terms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,x_range', CASES)
def test_moment_sum(ctx, shape, x_range):
    for lname in LATTICES:
        setup(ctx, shape, lname, x_range)
        for n in N_LABELS:
            ctx.upload_labels(label_map(shape, n))
            got, volume = ctx.moment_sum(LATTICES[lname], centres(shape, lname, n), VV)
            _, _, _, s, cnt, mag = reference(shape, x_range, lname, n)
            check(got, volume, s, cnt, mag, f'{shape} {x_range} {lname} n {n}')
            a = n // 2 if n >= 3 else None
            if a is not None:
                assert cnt[a] == 0 and volume[a] == 0.0


def test_every_label_dtype_in(ctx):
    shape, lname, n = (5, 7, 11), 'tric', 2
    setup(ctx, shape, lname)
    cen = centres(shape, lname, n)
    for dt in INTS:
        lab = label_map(shape, n).astype(np.int64)
        lab[lab == np.iinfo(np.int32).max] = np.iinfo(dt).max       # the largest label the dtype holds, far above n
        lab = lab.astype(dt)
        ctx.upload_labels(lab)
        got, volume = ctx.moment_sum(LATTICES[lname], cen, VV)
        terms, _, label = reference_terms(density(shape), lab, LATTICES[lname], cen)
        check(got, volume, *grouped(terms, label, n), f'labels as {np.dtype(dt).name}')


# ---- coherent labels: the wave-uniform route -----------------------------------------------------------------------------------
def coherent_maps(shape):
    p0, p1, p2 = np.indices(shape)
    return {
        'slabs of two planes (whole waves share a label, it changes between a wave\'s steps)': (p0 // 2, shape[0] // 2 + 1),
        'blocks (runs of 20 voxels: several labels in a wave, each group reduced)': ((p0 // 4) * 4 + (p1 // 8) * 2 + p2 // 20, 16),
        'runs of five (the label changes mid-wave, groups too small to reduce)': (p2 // 5, shape[2] // 5 + 1),
        'one voxel of another label inside a uniform wave': (np.where((p0 == 3) & (p1 == 5) & (p2 == 17), 1, 0), 2),
        'vacuum runs inside uniform waves': (np.where(p2 % 16 < 3, -1, p0 // 6), 3),
    }


@pytest.mark.parametrize('lname', list(LATTICES))
def test_coherent_labels(ctx, lname):
    shape = (12, 16, 40)                    # 7 680 voxels: two blocks, planes of ten waves
    assert np.prod(shape) > BLOCK
    setup(ctx, shape, lname)
    for what, (lab, n_own) in coherent_maps(shape).items():
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        ctx.upload_labels(lab)
        for n in (n_own, MS_BINS + 1):      # the LDS route, and the same map through the global route
            assert n_own <= MS_BINS
            cen = centres(shape, lname, n)
            got, volume = ctx.moment_sum(LATTICES[lname], cen, VV)
            terms, _, label = reference_terms(density(shape), lab, LATTICES[lname], cen)
            check(got, volume, *grouped(terms, label, n), f'{what}, {lname}, n {n}')


# ---- physics -------------------------------------------------------------------------------------------------------------------
def gaussian(n, h, at, sigma=0.9):
    """exp(-r^2 / 2 sigma^2) about the grid point `at` of an n^3 grid of spacing h (n odd: no voxel lies half a cell away,
    where the two images tie); r^2 is a sum of exact multiples of h^2 = 2^-4, so mirror images and axis permutations of a
    voxel carry the same bits"""
    k = [((np.arange(n) - a + n // 2) % n) - n // 2 for a in at]
    r2 = (k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2) * (h * h)
    return np.ascontiguousarray(np.exp(-r2 / (2.0 * sigma * sigma)))


def test_gaussian_on_an_atom(ctx):
    """a cubic cell whose voxel positions, centre and image vectors are all exact in float64 (spacing 1/4): the terms of a
    voxel and of its mirror image cancel exactly, so fsum gives a dipole of exactly zero and an exactly isotropic m2"""
    n, h = 21, 0.25
    lat = np.eye(3) * (n * h)
    at = (2, 18, 13)
    rho = gaussian(n, h, at)
    shape = (n, n, n)
    vl = lat / n
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    ctx.upload_density(rho)
    lab = np.zeros(shape, np.int32)
    ctx.upload_labels(lab)
    cen = np.array([at], dtype=np.float64) * h
    got, volume = ctx.moment_sum(lat, cen, VV)
    terms, image, label = reference_terms(rho, lab, lat, cen)
    s, cnt, mag = grouped(terms, label, 1)
    check(got, volume, s, cnt, mag, 'gaussian')
    lim = bound(cnt, mag, VV)[0]
    assert not s[0, 1:4].any() and not s[0, [5, 6, 8]].any() and s[0, 4] == s[0, 7] == s[0, 9]
    print('dipole', got[0, 1:4], 'bound', lim[1:4], 'm2', got[0, 4:], 'bound', lim[4:])
    assert np.all(np.abs(got[0, 1:4]) <= lim[1:4]), 'the dipole of a centred Gaussian is zero within the bound'
    assert np.all(np.abs(got[0, [5, 6, 8]]) <= lim[[5, 6, 8]]), 'm2 has no off-diagonal part within the bound'
    assert abs(got[0, 4] - got[0, 7]) <= 2 * lim[4] and abs(got[0, 7] - got[0, 9]) <= 2 * lim[4], 'm2 is isotropic within the bound'
    charge, _ = ctx.charge_sum(VV, 1)
    assert abs(got[0, 0] - charge[0]) <= 2 * lim[0], 'm0 is the charge of xb_charge_sum within the two bounds'
    assert (image != 13).mean() > 0.5         # (the atom sits off-centre: most voxels reach it through an image)
    # the same picture rolled by whole voxels across the cell edge, the atom with it
    shift = (19, -7, 11)
    at2 = tuple((a + d) % n for a, d in zip(at, shift))
    rho2 = np.ascontiguousarray(np.roll(rho, shift, axis=(0, 1, 2)))
    assert np.array_equal(rho2, gaussian(n, h, at2))
    ctx.upload_density(rho2)
    cen2 = np.array([at2], dtype=np.float64) * h
    got2, volume2 = ctx.moment_sum(lat, cen2, VV)
    terms2, _, label2 = reference_terms(rho2, lab, lat, cen2)
    s2, cnt2, mag2 = grouped(terms2, label2, 1)
    check(got2, volume2, s2, cnt2, mag2, 'gaussian, rolled')
    assert np.all(np.abs(got2 - got) <= lim + bound(cnt2, mag2, VV)[0]), 'rolling the grid and the atom moves no moment'


# ---- purity --------------------------------------------------------------------------------------------------------------------
def test_nothing_resident_is_written(ctx):
    shape, lname, n = (13, 17, 19), 'tric', 5
    # a density whose sums are exact in any order (multiples of 2^-10 below 2^10), so that charge_sum repeats bit for bit
    rho = np.round(density(shape) * 1024.0) / 1024.0
    assert np.abs(rho).max() < 1024 and np.array_equal(rho * 1024, np.round(rho * 1024))
    setup(ctx, shape, lname, rho=rho)
    lab = label_map(shape, n)
    ctx.upload_labels(lab)
    before = ctx.charge_sum(VV, n)
    for m in (n, MS_BINS + 1):
        ctx.moment_sum(LATTICES[lname], centres(shape, lname, m), VV)
        assert np.array_equal(ctx.download_labels(np.int32), lab)
        assert np.array_equal(ctx.download_density().view(np.uint64), rho.view(np.uint64))
        after = ctx.charge_sum(VV, n)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- device arrays ---------------------------------------------------------------------------------------------------------------
def device_copy(ctx, rho):
    """`rho` as a device array: a torch tensor where torch sees the GPU, else a device.DeviceArray (filled by the library: the
    masked volume of an all-zero map is the density itself)"""
    if torch is not None and torch.cuda.is_available():
        return torch.as_tensor(rho.copy(), device='cuda')
    ctx.upload_density(rho)
    ctx.upload_labels(np.zeros(rho.shape, np.int8))
    return ctx.export_volume(0)


def test_device_density_and_repeatability():
    ctx = _lib.default_context()
    shape, lname = (13, 17, 19), 'tric'
    lat = LATTICES[lname]
    rho = density(shape)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    dev = device_copy(ctx, rho)
    assert device.is_device_array(dev)
    # every voxel a label of its own: each sum is ONE term, no order is left, the bytes are defined
    nvox = int(np.prod(shape))
    own = np.arange(nvox, dtype=np.int32).reshape(shape)
    cen = centres(shape, lname, nvox)
    host, host_v = multipole.moment_sum(rho, own, lat, cen, VV)
    terms, _, _ = reference_terms(rho, own, lat, cen)
    # (0 + t on the device: a term of -0.0 arrives as +0.0)
    assert np.array_equal(host.view(np.uint64), ((terms + 0.0) * VV).view(np.uint64)), 'single-term sums are the terms times vv, bit for bit'
    assert np.array_equal(host_v, np.full(nvox, VV))
    got, got_v = multipole.moment_sum(dev, own, lat, cen, VV)
    assert np.array_equal(got.view(np.uint64), host.view(np.uint64)) and np.array_equal(got_v, host_v)
    # inside resident() a device density and a host map work without further code, and two calls agree within twice the bound
    n = 5
    lab = label_map(shape, n)
    _, _, _, s, cnt, mag = reference(shape, None, lname, n)
    with utils.resident(dev):
        a, av = multipole.moment_sum(dev, lab, lat, centres(shape, lname, n), VV)
        b, bv = multipole.moment_sum(dev, lab, lat, centres(shape, lname, n), VV)
    check(a, av, s, cnt, mag, 'device density, first call')
    check(b, bv, s, cnt, mag, 'device density, second call')
    assert np.all(np.abs(a - b) <= 2 * bound(cnt, mag, VV))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_bader_with_the_flag():
    """two unequal atoms at 24^3.  The synthetic density is rounded to multiples of 2^-20, which makes every charge sum exact
    in any order: the flag-off attributes (float atomics otherwise) can then be compared bit for bit between two runs"""
    shape, lat = (24, 24, 24), synth.CUBIC6
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(atoms5, lat)
    off = Bader({'charge': rho.copy()}, lat, atoms)
    off()
    on = Bader({'charge': rho.copy()}, lat, atoms, multipole_flag=True)
    on()
    new = {'atoms_moments', 'atoms_dipole', 'atoms_quadrupole', 'bader_moments'}
    assert set(vars(on)) - set(vars(off)) == new | {'multipole_flag'}
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference'):
            continue
        got = getattr(on, key)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert got == want, key
    n = atoms.shape[0]
    assert on.atoms_moments.shape == (n, 10) and on.atoms_dipole.shape == (n, 3) and on.atoms_quadrupole.shape == (n, 3, 3)
    assert on.bader_moments.shape == (on.bader_maxima.shape[0], 10)
    terms, _, label = reference_terms(rho, on.atoms_volumes, lat, atoms - on.voxel_offset)
    s, cnt, mag = grouped(terms, label, n)
    vv = on.voxel_volume
    lim = (cnt[:, None] + 2) * 2.0 ** -53 * mag * vv
    print('atoms_moments', on.atoms_moments, 'bound', lim)
    assert np.all(np.abs(on.atoms_moments - s * vv) <= lim)
    assert np.all(np.abs(on.atoms_moments[:, 0] - on.atoms_charge) <= 2 * lim[:, 0])
    assert np.all(np.abs(on.atoms_dipole + s[:, 1:4] * vv) <= lim[:, 1:4])
    assert np.abs(on.atoms_dipole).max() > 1e3 * lim[:, 1:4].max(), 'unequal neighbours polarise each other'
    assert np.array_equal(on.atoms_quadrupole, multipole.quadrupole(on.atoms_moments))


# ---- error codes, timer, memory ----------------------------------------------------------------------------------------------------
def test_error_codes_and_bookkeeping():
    c = _lib.Context(0)
    try:
        shape, lname, n = (5, 7, 11), 'ortho', 2
        lat, cen = LATTICES[lname], centres(shape, lname, n)
        with pytest.raises(_lib.BaderHipError) as e:
            c.moment_sum(lat, cen, VV)
        assert e.value.code == _lib.XB_E_STATE                      # no grid
        vl = np.divide(lat, shape)
        c.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
        with pytest.raises(_lib.BaderHipError) as e:
            c.moment_sum(lat, cen, VV)
        assert e.value.code == _lib.XB_E_STATE                      # no density
        c.upload_density(density(shape))
        with pytest.raises(_lib.BaderHipError) as e:
            c.moment_sum(lat, cen, VV)
        assert e.value.code == _lib.XB_E_STATE                      # no labels
        c.upload_labels(label_map(shape, n))
        pd = C.POINTER(C.c_double)
        l9, ce = np.ascontiguousarray(lat).reshape(9), np.ascontiguousarray(cen)
        mo, vo = np.zeros((n, 10)), np.zeros(n)
        args = [l9.ctypes.data_as(pd), ce.ctypes.data_as(pd), n, VV, mo.ctypes.data_as(pd), vo.ctypes.data_as(pd)]
        for bad in (dict(k=2, v=0), dict(k=2, v=-3), dict(k=0, v=None), dict(k=1, v=None), dict(k=4, v=None), dict(k=5, v=None)):
            a = list(args)
            a[bad['k']] = bad['v']
            assert c.lib.xb_moment_sum(c.h, *a) == _lib.XB_E_ARG, bad
        assert not mo.any() and not vo.any()
        # the context works on
        before = c.memory_stats()
        c.enable_timing(only=[_lib.XB_TIMER_MOMENTS])
        c.kernel_time_reset()
        got, volume = c.moment_sum(lat, cen, VV)
        _, _, _, s, cnt, mag = reference(shape, None, lname, n)
        check(got, volume, s, cnt, mag, 'after the refused calls')
        ms, launches = c.kernel_time(_lib.XB_TIMER_MOMENTS)
        assert launches == 1 and ms > 0.0
        c.enable_timing(False)
        big = MS_BINS + 1000
        c.moment_sum(lat, centres(shape, lname, big), VV)
        after = c.memory_stats()
        assert after[2] - before[2] >= 14 * 8 * big - 14 * 8 * n and after[0] - before[0] == after[2] - before[2]
        # another grid forgets the old density and labels
        c.set_grid((6, 5, 4), np.zeros(27), np.zeros(9))
        with pytest.raises(_lib.BaderHipError) as e:
            c.moment_sum(lat, cen, VV)
        assert e.value.code == _lib.XB_E_STATE
    finally:
        c.close()

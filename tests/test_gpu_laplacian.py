"""xb_laplacian_field / xb_laplacian_sum / xb_stencil_points and what stands on them (-m gpu) against the numpy restatement of
tests/test_laplacian_cpu.py.

The field and the ten values at a point are compared with == : every operation of the definition is bit-defined
(include/bader_hip.h).  XB_STENCIL_GATHER is the second implementation: every field and every sum runs through the tiles and
through the gather, and both must agree with the restatement.  THE BOUND of the sums, per label, for the sum and the sum of
magnitudes alike (tests/test_gpu_multipole.py, taken from there):

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

Volumes (counts) are exact.  tests/test_laplacian_cpu.py::test_the_sums_bound_notices_a_voxel_on_the_wrong_label shows for
every input used here that one voxel on the wrong label breaks this bound."""
import ctypes as C
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, critical, device, laplacian, synth, utils
from pybader_amd.interface import Bader
from test_critical_cpu import FULL, case
from test_critical_cpu import reference as critical_reference
from test_laplacian_cpu import (COHERENT_SHAPE, NO_VACUUM, ST_BINS, cell_sum_bound, coefficients, coherent_maps, grouped, noise,
                                restated_laplacian, restated_points, sum_bound, sum_field, sum_inputs)
from test_multipole_cpu import LATTICES, VV, density, label_map

pytestmark = pytest.mark.gpu
INTS = (np.int8, np.int16, np.int32, np.int64)
TRIC24 = synth.TRICLINIC

# name -> (the density's case in tests/test_critical_cpu.py, the cell): the inputs of the field
FIELD_CASES = {
    'synth8': synth.CUBIC6, 'synth40x36x44': synth.CUBIC6, 'tric24': TRIC24, 'rough': synth.CUBIC6,
    'noise20x9x33': LATTICES['tric'], 'noise3': LATTICES['tric'], 'noise2': LATTICES['tric'], 'noise1x2x9': LATTICES['tric'],
    'constant': LATTICES['tric'],
}


@functools.lru_cache(maxsize=None)
def field_case(name):
    """(density, cell, restated Laplacian) of one input of the field, computed once and never written"""
    rho = noise((9, 7, 33), 2) if name == 'noise9x7x33' else case(name)
    lat = FIELD_CASES.get(name, LATTICES['tric'])
    want = restated_laplacian(rho, lat)
    want.flags.writeable = False
    return rho, lat, want


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    diff = got.view(np.uint64) != want.view(np.uint64)
    # (+0.0 and -0.0 are one value of the definition's arithmetic only where both sides formed them alike: compare bits)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ from the restatement, first at {np.argwhere(diff)[0].tolist()}'


# ---- the field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELD_CASES) + ['noise9x7x33'])
def test_field_equals_the_restatement_through_both_routes(ctx, name):
    rho, lat, want = field_case(name)
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    same_bits(ctx.laplacian_field(lat), want, name + ' (tiles, host output)')
    same_bits(ctx.laplacian_field(lat, gather=True), want, name + ' (gather, host output)')
    for gather in (False, True):
        dev = ctx.laplacian_field(lat, gather=gather, on_device=True)
        assert isinstance(dev, device.DeviceArray) and dev.shape == rho.shape and dev.dtype == np.float64
        same_bits(dev.to_host(), want, f'{name} (gather {gather}, device output)')
    assert np.array_equal(ctx.download_density(), rho), 'the resident density is not written'
    if name == 'constant':
        assert not want.any()


def test_field_of_a_float32_device_tensor():
    if torch is None or not torch.cuda.is_available():
        pytest.skip('torch with a GPU is needed for a device tensor')
    rho32 = case('rough').astype(np.float32)
    t = torch.as_tensor(rho32.copy(), device='cuda')
    want = restated_laplacian(rho32.astype(np.float64), synth.CUBIC6)
    for gather in (False, True):
        got = laplacian.laplacian(t, synth.CUBIC6, gather=gather)
        assert isinstance(got, device.DeviceArray)
        same_bits(got.to_host(), want, f'float32 tensor, gather {gather}')
        back = torch.as_tensor(got, device='cuda')        # (the result publishes the interface: no copy)
        assert back.dtype == torch.float64 and tuple(back.shape) == rho32.shape


def test_field_through_the_python_layer_and_resident():
    rho, lat, want = field_case('tric24')
    got = laplacian.laplacian(rho, lat)
    assert isinstance(got, np.ndarray)
    same_bits(got, want, 'host array')
    with utils.resident(rho):
        same_bits(laplacian.laplacian(rho, lat, gather=True), want, 'resident, gather')
        same_bits(laplacian.laplacian(rho, lat), want, 'resident, tiles')


# ---- the sums -------------------------------------------------------------------------------------------------------------------
def check_sums(got, lap, lab, n, what):
    """the bound for the sum and the sum of magnitudes of every label (each figure printed before it is asserted), exact volumes"""
    s, cnt, mag = grouped(lap, lab, n)
    L, L_abs, volume = got
    assert L.shape == L_abs.shape == volume.shape == (n,)
    assert np.array_equal(volume, cnt.astype(np.float64) * VV), f'{what}: volumes'
    lim = sum_bound(cnt, mag)
    for name, g, w in (('sum', L, s), ('sum of magnitudes', L_abs, mag)):
        err = np.abs(g - w * VV)
        a = int(np.argmax(err - lim))
        print(f'{what}: {name}, worst label {a} ({cnt[a]} voxels): off by {err[a]:.3e}, bound {lim[a]:.3e}')
        assert np.all(err <= lim), f'{what}: {name} of label {a} ({cnt[a]} voxels) off by {err[a]:.3e}, bound {lim[a]:.3e}'
    assert not L[cnt == 0].any() and not L_abs[cnt == 0].any(), f'{what}: something landed on a label nobody carries'
    return s, cnt, mag


def test_sums_on_every_input_through_both_routes(ctx):
    assert ST_BINS > 2
    resident = None
    for what, kind, shape, lname, lab, n in sum_inputs():
        rho, lap = sum_field(kind, shape, lname)
        if resident != (kind, shape):
            ctx.set_grid(shape, np.zeros(27), np.zeros(9))
            ctx.upload_density(rho)
            resident = (kind, shape)
        ctx.upload_labels(lab)
        for gather in (False, True):
            _, cnt, _ = check_sums(ctx.laplacian_sum(LATTICES[lname], n, VV, gather), lap, lab, n, f'{what}, gather {gather}')
        if kind == 'decades' and n >= 3:
            assert cnt[n // 2] == 0, 'the label map leaves one label empty'
        assert (lab < 0).any() or kind == 'noise'
    assert np.array_equal(ctx.download_labels(np.int32), lab) and np.array_equal(ctx.download_density(), rho), 'nothing resident is written'


def test_every_label_dtype_in(ctx):
    shape, lname, n = (13, 17, 19), 'tric', 2
    rho, lap = sum_field('decades', shape, lname)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    for dt in INTS:
        lab = label_map(shape, n).astype(np.int64)
        lab[lab == np.iinfo(np.int32).max] = np.iinfo(dt).max       # the largest label the dtype holds, far above n
        lab = lab.astype(dt)
        ctx.upload_labels(lab)
        for gather in (False, True):
            check_sums(ctx.laplacian_sum(LATTICES[lname], n, VV, gather), lap, lab, n, f'labels as {np.dtype(dt).name}, gather {gather}')
    got = laplacian.basin_laplacian(rho, label_map(shape, n).astype(np.int8), LATTICES[lname], n, VV)
    check_sums(got, lap, label_map(shape, n), n, 'through laplacian.basin_laplacian')
    assert all(a.shape == (0,) for a in laplacian.basin_laplacian(rho, label_map(shape, n), LATTICES[lname], 0, VV))


@pytest.mark.parametrize('lname', list(LATTICES))
def test_basin_sums_of_a_map_without_vacuum_add_up_to_the_cells_zero(ctx, lname):
    """every voxel carries a label in [0, n): the sum of L over the labels is the Laplacian summed over the cell, which vanishes
    within the bound of tests/test_laplacian_cpu.py::test_the_laplacian_sums_to_zero_over_the_cell (times the voxel volume)"""
    lab, n = coherent_maps(COHERENT_SHAPE)[NO_VACUUM]
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    rho, _ = sum_field('noise', COHERENT_SHAPE, lname)
    assert lab.min() == 0 and lab.max() < n
    ctx.set_grid(COHERENT_SHAPE, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    ctx.upload_labels(lab)
    _, w, _ = coefficients(LATTICES[lname], COHERENT_SHAPE)
    lim = cell_sum_bound(rho, w) * VV
    for gather in (False, True):
        L, _, volume = ctx.laplacian_sum(LATTICES[lname], n, VV, gather)
        print(f'{lname}, gather {gather}: L sums to {L.sum():.3e} over {n} labels, bound {lim:.3e}')
        assert abs(L.sum()) <= lim and volume.sum() == rho.size * VV


def test_the_sums_buffer_is_counted():
    shape = (13, 17, 19)
    c = _lib.Context(0)
    try:
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(density(shape))
        c.upload_labels(label_map(shape, 2))
        before = c.memory_stats()
        c.laplacian_sum(LATTICES['tric'], 3000, VV)
        after = c.memory_stats()
        assert after[2] - before[2] == 24 * 3000 and after[0] - before[0] == after[2] - before[2]
        c.laplacian_sum(LATTICES['tric'], 2, VV)                  # (a smaller n fits the buffer)
        c.laplacian_field(LATTICES['tric'])                        # (the field goes through the scratch the context has)
        c.stencil_points(LATTICES['tric'], [0, 1])
        assert c.memory_stats() == after
    finally:
        c.close()


# ---- listed voxels ----------------------------------------------------------------------------------------------------------------
def test_points_at_every_critical_point_of_the_2x2x2_arrangement(ctx):
    rho = case('grid2x2x2')
    counts, lin, masks, ring, bond = critical_reference('grid2x2x2')
    assert counts.tolist() == [8, 24, 24, 24, 24, 8]
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    same_bits(ctx.stencil_points(synth.CUBIC6, lin), restated_points(rho, synth.CUBIC6, lin), 'the ten values')
    # the physics, through the Python layer
    p = laplacian.point_properties(rho, synth.CUBIC6, lin)
    same_bits(p.laplacian, restated_laplacian(rho, synth.CUBIC6).reshape(-1)[lin], 'the Laplacian at the points')
    assert np.array_equal(p.rho, rho.reshape(-1)[lin]) and np.array_equal(p.voxels, np.stack(np.unravel_index(lin, rho.shape), axis=1))
    nuclear, bonds = masks == FULL, bond > 0
    print('largest eigenvalue at the nuclear points', p.eigenvalues[nuclear, 2].tolist())
    print('signature at the bond voxels', p.signature[bonds].tolist(), 'ellipticity', np.round(p.ellipticity[bonds], 4).tolist())
    assert nuclear.sum() == 8 and (p.eigenvalues[nuclear] < 0).all(), 'every nuclear point has three negative eigenvalues'
    assert bonds.sum() == 24 and (p.signature[bonds] == -1).all(), 'every bond voxel has signature -1'
    assert (p.ellipticity[bonds] >= 0).all() and np.isnan(p.ellipticity[masks == 0]).all()
    by_voxel = laplacian.point_properties(rho, synth.CUBIC6, p.voxels)
    assert np.array_equal(by_voxel.lin, lin) and np.array_equal(by_voxel.hessian, p.hessian)


@pytest.mark.parametrize('name', ['noise20x9x33', 'noise9x7x33', 'noise3', 'noise2', 'noise1x2x9'])
def test_points_at_hashed_voxels_of_the_noise_grids(ctx, name):
    rho, lat, want_lap = field_case(name)
    nx, ny, nz = rho.shape
    faces = [(0, ny // 2, nz // 2), (nx - 1, ny // 2, nz // 2), (nx // 2, 0, nz // 2), (nx // 2, ny - 1, nz // 2),
             (nx // 2, ny // 2, 0), (nx // 2, ny // 2, nz - 1), (0, 0, 0), (nx - 1, ny - 1, nz - 1)]
    lin = np.concatenate([np.ravel_multi_index(np.array(faces).T, rho.shape),
                          np.floor(synth.hash_noise((56,), 17) * rho.size).astype(np.int64)])       # (repeats allowed)
    assert lin.size == 64
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    same_bits(ctx.stencil_points(lat, lin), restated_points(rho, lat, lin), name)
    same_bits(laplacian.point_properties(rho, lat, lin).laplacian, want_lap.reshape(-1)[lin], name + ', the Laplacian')


def test_no_points(ctx):
    rho, lat, _ = field_case('noise3')
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    assert ctx.stencil_points(lat, []).shape == (0, 10)
    assert ctx.lib.xb_stencil_points(ctx.h, (C.c_double * 9)(*lat.reshape(-1)), None, 0, None) == 0
    p = laplacian.point_properties(rho, lat, np.zeros((0, 3), np.int64))
    assert len(p) == 0 and p.hessian.shape == (0, 3, 3) and p.eigenvalues.shape == (0, 3) and p.laplacian.shape == (0,)


# ---- error codes --------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        rho = case('synth8')
        lat = synth.CUBIC6
        n_vox = rho.size
        for call in (lambda: c.laplacian_field(lat), lambda: c.laplacian_sum(lat, 2, VV), lambda: c.stencil_points(lat, [0])):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no grid
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9))
        for call in (lambda: c.laplacian_field(lat), lambda: c.laplacian_sum(lat, 2, VV), lambda: c.stencil_points(lat, [0])):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no density
        c.upload_density(rho)
        with pytest.raises(_lib.BaderHipError) as e:
            c.laplacian_sum(lat, 2, VV)
        assert e.value.code == _lib.XB_E_STATE                      # no labels
        c.upload_labels(np.zeros(rho.shape, np.int32))
        lp = (C.c_double * 9)(*lat.reshape(-1))
        flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)          # a singular lattice
        out = np.full(n_vox, -7.0)
        dev = device.DeviceArray(c, rho.shape, np.float64)
        lib, h, arg = c.lib, c.h, _lib.XB_E_ARG
        # the field: a null lattice, both outputs, neither, unknown flag bits, a singular lattice, a host pointer as the device
        # output, a device output that reaches one element past its allocation, one that is not aligned
        assert lib.xb_laplacian_field(h, None, 0, out.ctypes.data, None) == arg
        assert lib.xb_laplacian_field(h, lp, 0, out.ctypes.data, C.c_void_p(dev.ptr)) == arg
        assert lib.xb_laplacian_field(h, lp, 0, None, None) == arg
        assert lib.xb_laplacian_field(h, lp, 2, out.ctypes.data, None) == arg
        assert lib.xb_laplacian_field(h, flat, 0, out.ctypes.data, None) == arg
        assert lib.xb_laplacian_field(h, lp, 0, None, out.ctypes.data) == arg
        assert n_vox * 8 == dev.nbytes == 4096
        assert lib.xb_laplacian_field(h, lp, 0, None, C.c_void_p(dev.ptr + 8)) == arg
        assert lib.xb_laplacian_field(h, lp, 0, None, C.c_void_p(dev.ptr + 4)) == arg
        assert (out == -7.0).all(), 'a refused call writes nothing'
        # the sums: null pointers, unknown flag bits, n < 1, a singular lattice
        s, m, v = (np.full(2, -7.0) for _ in range(3))
        ps, pm, pv = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (s, m, v))
        assert lib.xb_laplacian_sum(h, None, 2, VV, 0, ps, pm, pv) == arg
        assert lib.xb_laplacian_sum(h, lp, 2, VV, 0, None, pm, pv) == arg
        assert lib.xb_laplacian_sum(h, lp, 2, VV, 0, ps, None, pv) == arg
        assert lib.xb_laplacian_sum(h, lp, 2, VV, 0, ps, pm, None) == arg
        assert lib.xb_laplacian_sum(h, lp, 2, VV, 4, ps, pm, pv) == arg
        assert lib.xb_laplacian_sum(h, lp, 0, VV, 0, ps, pm, pv) == arg
        assert lib.xb_laplacian_sum(h, flat, 2, VV, 0, ps, pm, pv) == arg
        assert (s == -7.0).all() and (m == -7.0).all() and (v == -7.0).all()
        # the points: null pointers with m > 0, m < 0, an index outside [0, N), a singular lattice
        idx, vals = np.array([0, n_vox - 1], np.int64), np.full(20, -7.0)
        assert lib.xb_stencil_points(h, None, idx.ctypes.data, 2, vals.ctypes.data) == arg
        assert lib.xb_stencil_points(h, lp, None, 2, vals.ctypes.data) == arg
        assert lib.xb_stencil_points(h, lp, idx.ctypes.data, 2, None) == arg
        assert lib.xb_stencil_points(h, lp, idx.ctypes.data, -1, vals.ctypes.data) == arg
        assert lib.xb_stencil_points(h, flat, idx.ctypes.data, 2, vals.ctypes.data) == arg
        for bad in (-1, n_vox, 2 ** 40):
            idx[1] = bad
            assert lib.xb_stencil_points(h, lp, idx.ctypes.data, 2, vals.ctypes.data) == arg
        assert (vals == -7.0).all()
        with pytest.raises(_lib.BaderHipError) as e:
            laplacian.point_properties(rho, lat, [n_vox])
        assert e.value.code == arg
        # a slab is refused; the whole grid works again
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(rho)
        c.upload_labels(np.zeros(rho.shape, np.int32))
        for call in (lambda: c.laplacian_field(lat), lambda: c.laplacian_sum(lat, 2, VV), lambda: c.stencil_points(lat, [0])):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        same_bits(c.laplacian_field(lat), restated_laplacian(rho, lat), 'synth8 again')
    finally:
        c.close()


# ---- Bader(laplacian_flag=True) -------------------------------------------------------------------------------------------------------
def _host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


def _same_attributes(on, off, new):
    assert set(vars(on)) - set(vars(off)) == new, set(vars(on)) - set(vars(off)) ^ new
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference', 'laplacian_flag'):
            continue
        got, want = _host(getattr(on, key)), _host(want)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        elif isinstance(want, (critical.CriticalPoints, critical.BondGraph)):
            for k, w in vars(want).items():
                assert np.array_equal(getattr(got, k), w), (key, k)
        else:
            assert got == want, key


@pytest.mark.parametrize('on_device', [False, True], ids=['host density', 'device density'])
def test_bader_with_the_flag(on_device):
    """two unequal atoms at 24^3 with a vacuum tolerance.  The synthetic density is rounded to multiples of 2^-20, which makes
    every charge sum exact in any order: the attributes that exist without the flag can be compared bit for bit between runs"""
    shape, lat = (24, 24, 24), synth.CUBIC6
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5, 0.0) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(atoms5, lat)
    tol = 2.0 ** -10
    ctx = _lib.default_context()

    def charge():
        if not on_device:
            return rho.copy()
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        ctx.upload_density(rho)
        ctx.upload_labels(np.zeros(shape, np.int8))
        return ctx.export_volume(0)          # a library-owned device array holding the density

    sums = {'atoms_laplacian', 'atoms_laplacian_abs', 'bader_laplacian', 'bader_laplacian_abs'}
    points = {'critical_properties', 'critical_laplacian', 'critical_hessian', 'critical_eigenvalues', 'critical_ellipticity',
              'atoms_bond_laplacian', 'atoms_bond_ellipticity'}
    for crit in (False, True):
        off = Bader({'charge': charge()}, lat, atoms, vacuum_tol=tol, critical_flag=crit)
        off()
        on = Bader({'charge': charge()}, lat, atoms, vacuum_tol=tol, critical_flag=crit, laplacian_flag=True)
        on()
        _same_attributes(on, off, sums | (points if crit else set()) | {'laplacian_flag'})
        vv = on.voxel_volume
        lap = restated_laplacian(rho, lat)
        for what, lab, n, got in (('atoms', on.atoms_volumes, 2, (on.atoms_laplacian, on.atoms_laplacian_abs)),
                                  ('volumes', on.bader_volumes, on.bader_maxima.shape[0], (on.bader_laplacian, on.bader_laplacian_abs))):
            lab = np.asarray(_host(lab))
            want = laplacian.basin_laplacian(on.reference, lab, lat, n, vv)
            s, cnt, mag = grouped(lap, lab, n)
            lim = sum_bound(cnt, mag, vv)
            for g, w, ref in zip(got, want, (s, mag)):
                # (two runs of float atomics: each within the bound of the restatement, so within twice it of each other)
                assert g.shape == (n,) and np.all(np.abs(g - ref * vv) <= lim) and np.all(np.abs(g - w) <= 2 * lim), what
            print(what, 'L', got[0].tolist(), 'L_abs', got[1].tolist())
        if crit:
            p = on.critical_properties
            q = laplacian.point_properties(on.reference, lat, on.critical_points.lin)
            for k in ('rho', 'gradient', 'hessian', 'laplacian', 'eigenvalues', 'ellipticity', 'signature', 'lin'):
                assert np.array_equal(getattr(p, k), getattr(q, k), equal_nan=True), k
            same_bits(np.ascontiguousarray(p.hessian[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]),
                      np.ascontiguousarray(restated_points(rho, lat, p.lin)[:, 4:]), 'the Hessian at the critical points')
            assert on.critical_laplacian is p.laplacian and on.critical_hessian is p.hessian
            assert on.critical_eigenvalues is p.eigenvalues and on.critical_ellipticity is p.ellipticity
            b = laplacian.point_properties(on.reference, lat, on.atoms_bond_graph.voxels)
            assert np.array_equal(on.atoms_bond_laplacian, b.laplacian) and np.array_equal(on.atoms_bond_ellipticity, b.ellipticity, equal_nan=True)
            assert on.atoms_bond_laplacian.shape == (len(on.atoms_bond_graph),)

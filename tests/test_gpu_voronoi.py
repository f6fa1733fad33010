"""xb_voronoi_assign and what stands on it (-m gpu) against the numpy restatement of tests/test_voronoi_cpu.py.

Every map is compared with == : the definition is bit-defined (include/bader_hip.h), so there is no tolerance anywhere.  The
forced full search (XB_VORONOI_FULL_SEARCH) is the second implementation: every case runs through both and the two maps must be
equal to the restatement and to each other.  Which route the tiles took is asserted from the call's statistics;
tests/test_voronoi_cpu.py::test_the_inputs_of_the_gpu_tests_reach_both_routes says why these inputs take them."""
import ctypes as C

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, device, synth, utils, voronoi
from pybader_amd.interface import Bader
from pybader_amd.utils import dtype_calc
from test_voronoi_cpu import (CANDIDATE_CASES, LATTICES, MIXED_N, MIXED_SHAPE, OVERFLOW_CASE, THIN_CASE, TIE_ATOMS, TIE_COUNTS,
                              TIE_LATTICE, TIE_SHAPE, TILE, candidate_counts, physics_case, random_atoms, reference,
                              reference_labels)

pytestmark = pytest.mark.gpu
CAP = _lib.XB_VORONOI_CAND_MAX
U = 2.0 ** -53


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def n_tiles(shape):
    return int(np.prod([-(-s // TILE) for s in shape]))


def both_routes(ctx, shape, lattice, atoms, want, what):
    """the map by the default route and by the forced full search, each == want; -> the default route's statistics"""
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    stats = ctx.voronoi_assign(lattice, atoms)
    got = ctx.download_labels(np.int32)
    print(f'{what}: {stats} of {n_tiles(shape)} tiles, {27 * len(atoms)} images')
    assert stats['candidate_tiles'] + stats['full_tiles'] == n_tiles(shape)
    bad = int((got != want).sum())
    assert bad == 0, f'{what}: {bad} voxels differ from the restatement'
    forced = ctx.voronoi_assign(lattice, atoms, full_search=True)
    assert forced == {'candidate_tiles': 0, 'full_tiles': n_tiles(shape), 'max_candidates': 0}
    full = ctx.download_labels(np.int32)
    assert np.array_equal(full, want), f'{what}: the forced full search differs from the restatement'
    assert np.array_equal(full, got)
    return stats


# ---- the routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,lname,n', CANDIDATE_CASES)
def test_candidate_route(ctx, shape, lname, n):
    atoms = random_atoms(lname, n)
    stats = both_routes(ctx, shape, LATTICES[lname], atoms, reference(shape, lname, n), f'{shape} {lname} n {n}')
    kept = candidate_counts(shape, LATTICES[lname], atoms)
    print('the restatement of phase 1 keeps at most', kept.max())
    assert stats['full_tiles'] == 0 and stats['candidate_tiles'] == n_tiles(shape)
    assert 0 < stats['max_candidates'] < 27 * n and stats['max_candidates'] <= CAP
    assert len(set(reference(shape, lname, n).reshape(-1))) == n, 'every atom owns voxels'


def test_overflow_route(ctx):
    shape, lname, n = OVERFLOW_CASE
    assert 27 * n > CAP
    stats = both_routes(ctx, shape, LATTICES[lname], random_atoms(lname, n), reference(shape, lname, n), f'overflow {shape} n {n}')
    assert stats['full_tiles'] > 0 and stats['max_candidates'] > CAP


@pytest.mark.parametrize('lname', list(LATTICES))
def test_mixed_routes_on_a_grid_with_partial_tiles(ctx, lname):
    shape, n = MIXED_SHAPE, MIXED_N
    assert all(s % TILE for s in shape)
    stats = both_routes(ctx, shape, LATTICES[lname], random_atoms(lname, n), reference(shape, lname, n), f'mixed {shape} {lname} n {n}')
    assert stats['full_tiles'] > 0 and stats['candidate_tiles'] > 0 and stats['max_candidates'] > CAP


def test_an_axis_of_length_one(ctx):
    shape, lname, n = THIN_CASE
    stats = both_routes(ctx, shape, LATTICES[lname], random_atoms(lname, n), reference(shape, lname, n), f'thin {shape}')
    assert stats['full_tiles'] == 0


def test_one_atom_and_one_voxel(ctx):
    lat = LATTICES['tric']
    both_routes(ctx, (9, 10, 11), lat, random_atoms('tric', 1), np.zeros((9, 10, 11), np.int32), 'one atom')
    atoms = random_atoms('tric', 8)
    both_routes(ctx, (1, 1, 1), lat, atoms, reference_labels((1, 1, 1), lat, atoms), 'one voxel')


def test_ties_do_not_depend_on_the_route(ctx):
    want = reference_labels(TIE_SHAPE, TIE_LATTICE, TIE_ATOMS)
    assert np.bincount(want.reshape(-1), minlength=5).tolist() == TIE_COUNTS
    stats = both_routes(ctx, TIE_SHAPE, TIE_LATTICE, TIE_ATOMS, want, 'ties')
    assert stats['full_tiles'] == 0
    # the same atoms in another order: the rule, not the order of the search, decides
    perm = [4, 2, 0, 3, 1]
    both_routes(ctx, TIE_SHAPE, TIE_LATTICE, TIE_ATOMS[perm], reference_labels(TIE_SHAPE, TIE_LATTICE, TIE_ATOMS[perm]), 'ties, permuted')


def test_physics_every_atom_gets_an_eighth(ctx):
    shape, lat, atoms = physics_case()
    both_routes(ctx, shape, lat, atoms, reference_labels(shape, lat, atoms), 'eight atoms')
    got = ctx.download_labels(np.int32)
    assert np.bincount(got.reshape(-1), minlength=8).tolist() == [int(np.prod(shape)) // 8] * 8


# ---- vacuum --------------------------------------------------------------------------------------------------------------------
def vacuum_density(shape, tol):
    """positive noise with a slab and scattered voxels at or below `tol`, some exactly at it, some zero and negative"""
    rng = np.random.default_rng(3)
    rho = tol + 0.5 + rng.random(shape)
    rho[shape[0] // 3: shape[0] // 3 + 5] = tol * rng.random((5,) + shape[1:])
    r = rng.random(shape)
    rho[r < 0.02] = tol
    rho[(r >= 0.02) & (r < 0.03)] = 0.0
    rho[(r >= 0.03) & (r < 0.04)] = -1.0
    rho[(r >= 0.04) & (r < 0.05)] = np.nextafter(tol, 1.0)
    return np.ascontiguousarray(rho)


def test_vacuum(ctx):
    shape, lname, n = CANDIDATE_CASES[1]
    lat, atoms, want = LATTICES[lname], random_atoms(lname, n), reference(shape, lname, n)
    tol = 0.125
    rho = vacuum_density(shape, tol)
    vac = rho <= tol
    assert 0.1 < vac.mean() < 0.5 and (rho == tol).sum() > 100
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    for full in (False, True):
        ctx.voronoi_assign(lat, atoms, vac_tol=tol, full_search=full)
        got = ctx.download_labels(np.int32)
        assert np.array_equal(got == -1, vac), 'the -1 labels sit exactly where rho <= tol'
        assert np.array_equal(got, np.where(vac, -1, want))
    # without a tolerance the density is not read: a context that never received one is accepted, with one it is refused
    c = _lib.Context(0)
    try:
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        with pytest.raises(_lib.BaderHipError) as e:
            c.voronoi_assign(lat, atoms, vac_tol=tol)
        assert e.value.code == _lib.XB_E_STATE
        c.voronoi_assign(lat, atoms)
        assert np.array_equal(c.download_labels(np.int32), want)
    finally:
        c.close()


def test_label_writer_hygiene(ctx):
    """xb_vacuum_assign(tol) marks the context "-1 means rho <= tol"; the Voronoi map written over it has no -1, and what follows
    must see that map: charge_sum sums it, every voxel counted"""
    shape, lname, n = CANDIDATE_CASES[1]
    lat, atoms, want = LATTICES[lname], random_atoms(lname, n), reference(shape, lname, n)
    tol = 0.125
    rho = vacuum_density(shape, tol)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    _, vac_volume = ctx.vacuum_assign(tol, 1.0)
    assert vac_volume == float((rho <= tol).sum())
    ctx.voronoi_assign(lat, atoms)
    got = ctx.download_labels(np.int32)
    assert np.array_equal(got, want) and got.min() == 0
    charge, volume = ctx.charge_sum(1.0, n)
    counts = np.bincount(want.reshape(-1), minlength=n)
    assert np.array_equal(volume, counts.astype(np.float64)) and volume.sum() == float(np.prod(shape))
    flat, lab = rho.reshape(-1), want.reshape(-1)
    for a in range(n):
        x = flat[lab == a]
        s, mag = float(np.sum(x)), float(np.abs(x).sum())
        assert abs(charge[a] - s) <= 2 * (x.size + 2) * U * mag, a
    # the deferred "labels := 0" of a vacuum sweep without a tolerance must not land on the map either
    ctx.vacuum_assign(None, 1.0)
    ctx.voronoi_assign(lat, atoms, full_search=True)
    _, again = ctx.charge_sum(1.0, n)
    assert np.array_equal(again, volume) and np.array_equal(ctx.download_labels(np.int32), want)
    # with a tolerance the vacuum voxels leave the sums
    ctx.voronoi_assign(lat, atoms, vac_tol=tol)
    _, volume = ctx.charge_sum(1.0, n)
    assert volume.sum() == float((rho > tol).sum())


# ---- error codes and bookkeeping ---------------------------------------------------------------------------------------------------
def test_error_codes_and_memory():
    c = _lib.Context(0)
    try:
        shape, lname, n = (9, 10, 11), 'tric', 8
        lat, atoms = LATTICES[lname], random_atoms(lname, n)
        with pytest.raises(_lib.BaderHipError) as e:
            c.voronoi_assign(lat, atoms)
        assert e.value.code == _lib.XB_E_STATE                      # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        with pytest.raises(_lib.BaderHipError) as e:
            c.voronoi_assign(lat, atoms, vac_tol=0.5)
        assert e.value.code == _lib.XB_E_STATE                      # a tolerance and no density
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        l9, at = np.ascontiguousarray(lat).reshape(9), np.ascontiguousarray(atoms)
        st = (C.c_int64 * 3)(-7, -7, -7)
        nan = float('nan')
        call = lambda *a: c.lib.xb_voronoi_assign(c.h, *a)
        good = [l9.ctypes.data_as(pd), at.ctypes.data_as(pd), n, nan, 0, st]
        for k, v in ((2, 0), (2, -1), (0, None), (1, None), (4, 2), (4, 3), (4, -1)):
            a = list(good)
            a[k] = v
            assert call(*a) == _lib.XB_E_ARG, (k, v)
        a = list(good)
        a[2] = (2 ** 31 - 1) // 27 + 1
        assert call(*a) == _lib.XB_E_LIMIT
        bad = at.copy()
        bad[3, 1] = np.inf
        a = list(good)
        a[1] = bad.ctypes.data_as(pd)
        assert call(*a) == _lib.XB_E_ARG
        assert list(st) == [-7, -7, -7], 'a refused call writes nothing'
        # a slab is refused, the whole grid works on; stats may be NULL
        c.set_grid(shape, np.zeros(27), np.zeros(9), (2, 5))
        with pytest.raises(_lib.BaderHipError) as e:
            c.voronoi_assign(lat, atoms)
        assert e.value.code == _lib.XB_E_STATE
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        before = c.memory_stats()
        assert c.voronoi_assign(lat, atoms, want_stats=False) is None
        assert np.array_equal(c.download_labels(np.int32), reference_labels(shape, lat, atoms))
        many = 5000
        c.voronoi_assign(lat, random_atoms(lname, many))
        after = c.memory_stats()
        assert after[2] - before[2] >= 24 * many and after[0] - before[0] == after[2] - before[2]
        assert c.download_labels(np.int32).max() < many
    finally:
        c.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
def device_copy(ctx, rho):
    """`rho` as a library-owned device array (the masked volume of an all-zero map is the density itself)"""
    ctx.upload_density(rho)
    ctx.upload_labels(np.zeros(rho.shape, np.int8))
    return ctx.export_volume(0)


def test_input_kinds_and_dtype():
    ctx = _lib.default_context()
    shape, lname = CANDIDATE_CASES[1][:2]
    lat = LATTICES[lname]
    rho = vacuum_density(shape, 0.125)
    for n in (8, 200):
        atoms = random_atoms(lname, n)
        want = reference_labels(shape, lat, atoms)
        dtype = np.dtype(dtype_calc(-n))
        assert dtype == (np.int8 if n == 8 else np.int16)
        host, stats = voronoi.voronoi_assign(rho, lat, atoms)
        assert isinstance(host, np.ndarray) and host.dtype == dtype and np.array_equal(host, want)
        assert set(stats) == {'candidate_tiles', 'full_tiles', 'max_candidates'}
        full, _ = voronoi.voronoi_assign(rho, lat, atoms, full_search=True)
        assert np.array_equal(full, want)
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        kinds = [device_copy(ctx, rho)]
        if torch is not None and torch.cuda.is_available():
            kinds.append(torch.as_tensor(rho.copy(), device='cuda'))
        for dev in kinds:
            got, _ = voronoi.voronoi_assign(dev, lat, atoms, vacuum_tol=0.125)
            assert device.is_device_array(got) and device.describe(got).dtype == dtype
            assert np.array_equal(device.to_host(got), np.where(rho <= 0.125, -1, want))
    # tracked inside resident() like any fetched label map: the sums that follow upload nothing
    atoms = random_atoms(lname, 8)
    want = reference_labels(shape, lat, atoms)
    with utils.resident(rho):
        volumes, _ = voronoi.voronoi_assign(rho, lat, atoms, vacuum_tol=0.125)
        assert utils.labels_resident(ctx, volumes) and not volumes.flags.writeable
        charge, volume = np.zeros(8), np.zeros(8)
        utils.charge_sum(charge, volume, 1.0, rho, volumes)
        assert utils.labels_resident(ctx, volumes)
    assert np.array_equal(volume, np.bincount(want[rho > 0.125], minlength=8).astype(np.float64))
    ch, vo, vols = voronoi.voronoi_charges(rho, lat, atoms, 1.0, vacuum_tol=0.125)
    assert np.array_equal(vols, volumes) and np.array_equal(vo, volume)
    assert np.all(np.abs(ch - charge) <= 2 * (vo + 2) * U * np.abs(rho).sum())


def test_bader_with_the_flag():
    """two unequal atoms at 24^3 with a vacuum tolerance.  The synthetic density is rounded to multiples of 2^-20, which makes
    every charge sum exact in any order: the flag-off attributes can then be compared bit for bit between two runs, and
    voronoi_charge with a host sum"""
    shape, lat = (24, 24, 24), synth.CUBIC6
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5, 0.0) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(atoms5, lat)
    tol = 2.0 ** -10
    assert 0.05 < (rho <= tol).mean() < 0.95
    off = Bader({'charge': rho.copy()}, lat, atoms, vacuum_tol=tol)
    off()
    on = Bader({'charge': rho.copy()}, lat, atoms, vacuum_tol=tol, voronoi_flag=True)
    on()
    new = {'voronoi_volumes', 'voronoi_charge', 'voronoi_volume', 'voronoi_stats'}
    assert set(vars(on)) - set(vars(off)) == new | {'voronoi_flag'}
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference'):
            continue
        got = getattr(on, key)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert got == want, key
    n = atoms.shape[0]
    want = np.where(rho <= tol, -1, reference_labels(shape, lat, atoms - on.voxel_offset))
    assert on.voronoi_volumes.dtype == on.atoms_volumes.dtype == np.dtype(dtype_calc(-n))
    assert np.array_equal(on.voronoi_volumes, want)
    counts = np.bincount(want[want >= 0], minlength=n)
    vv = on.voxel_volume
    assert np.array_equal(on.voronoi_volume, counts.astype(np.float64) * vv)
    total = on.lattice_volume - on.vacuum_volume
    lim = (counts.sum() + 2) * U * counts.sum() * vv
    print('voronoi volume', on.voronoi_volume.sum(), 'cell minus vacuum', total, 'bound', lim)
    assert abs(on.voronoi_volume.sum() - total) <= lim
    charge, volume = np.zeros(n), np.zeros(n)
    utils.charge_sum(charge, volume, vv, rho, on.voronoi_volumes)
    assert np.array_equal(on.voronoi_charge, charge) and np.array_equal(on.voronoi_volume, volume)
    host = np.array([rho[want == a].sum() for a in range(n)]) * vv      # (exact sums of multiples of 2^-20, one multiply)
    assert np.array_equal(on.voronoi_charge, host)
    # with a spin density the third sum appears, and nothing else
    spin = Bader({'charge': rho.copy(), 'spin': (rho * 0.5).copy()}, lat, atoms, vacuum_tol=tol, voronoi_flag=True, spin_flag=True)
    spin()
    assert np.array_equal(spin.voronoi_spin, on.voronoi_charge * 0.5) and np.array_equal(spin.voronoi_charge, on.voronoi_charge)
    assert np.array_equal(spin.voronoi_volume, on.voronoi_volume)

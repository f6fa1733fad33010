"""xb_critical_points / xb_critical_bonds and what stands on them (-m gpu) against the numpy restatement of
tests/test_critical_cpu.py.

Every list, count and pair is compared with == : the definition is combinatorial (include/bader_hip.h), so there is no
tolerance anywhere.  XB_CRITICAL_FLOOD is the second implementation: every case runs through the table and through the flood
fill, and both must equal the restatement.  tests/test_critical_cpu.py::test_the_inputs_exercise_what_they_are_for says
what each input is there for."""
import ctypes as C

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, critical, device, synth, utils
from pybader_amd.interface import Bader
from test_critical_cpu import (ATOMS_2X2X2, GPU_CASES, VACUUM_CASE, VACUUM_TOL, case, euler_sum, noise_labels, reference,
                               reference_bonds, reference_points)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_points(got, want, what):
    for name, g, w in zip(('counts', 'lin', 'lower mask', 'ring', 'bond'), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), f'{what}: {name} differs from the restatement'


def same_bonds(got, want, what):
    for name, g, w in zip(('pairs', 'saddles', 'rho_b', 'voxel'), got[:4], want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if name == 'rho_b':
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), f'{what}: {name} differs from the restatement'
    assert got[4] == want[4], f'{what}: same_basin {got[4]} != {want[4]}'


# ---- the list and the counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GPU_CASES)
def test_points_equal_the_restatement_through_both_implementations(ctx, name):
    rho = case(name)
    want = reference(name)
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    table = ctx.critical_points()
    print(name, rho.shape, 'counts', table[0].tolist(), 'list', table[1].size, 'euler', euler_sum(table[0]))
    same_points(table, want, name + ' (table)')
    same_points(ctx.critical_points(flood=True), want, name + ' (flood fill)')
    if min(rho.shape) >= 4:
        assert euler_sum(table[0]) == 0


def test_a_list_longer_than_the_first_allocation_is_not_cut(ctx):
    """pure noise: more than a third of the voxels are critical, far beyond N / 64 + 4096 records"""
    rho = synth.hash_noise((40, 33, 37), 9)
    want = reference_points(rho)
    assert want[1].size > rho.size // 64 + 4096
    ctx.critical_release()
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    before = ctx.memory_stats()
    same_points(ctx.critical_points(), want, 'noise, first call')
    after = ctx.memory_stats()
    assert after[2] - before[2] == 8 * want[1].size + 16384 and after[0] - before[0] == after[2] - before[2]
    same_points(ctx.critical_points(), want, 'noise, second call')       # (the list now fits: one pass)
    assert ctx.memory_stats() == after
    ctx.critical_release()
    assert ctx.memory_stats() == before


def test_vacuum(ctx):
    rho = case(VACUUM_CASE)
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    want = reference(VACUUM_CASE, VACUUM_TOL)
    same_points(ctx.critical_points(VACUUM_TOL), want, 'vacuum (table)')
    same_points(ctx.critical_points(VACUUM_TOL, flood=True), want, 'vacuum (flood fill)')
    assert want[1].size < reference(VACUUM_CASE)[1].size


def test_a_float32_device_tensor(ctx):
    if torch is None or not torch.cuda.is_available():
        pytest.skip('torch with a GPU is needed for a device tensor')
    rho32 = case('rough').astype(np.float32)
    t = torch.as_tensor(rho32.copy(), device='cuda')
    cp = critical.critical_points(t)
    want = reference_points(rho32.astype(np.float64))
    same_points((cp.counts, cp.lin, cp.masks, cp.ring, cp.bond), want, 'float32 tensor')
    assert np.array_equal(cp.voxels, np.stack(np.unravel_index(want[1], rho32.shape), axis=1))


# ---- the bond graph ------------------------------------------------------------------------------------------------------------
def library_maps(name, atoms5):
    """the library's own Bader map (bader_calc + refine) and atom map of a density"""
    rho = case(name)
    b = Bader({'charge': rho.copy()}, synth.CUBIC6, synth.atoms_cartesian(atoms5, synth.CUBIC6))
    b()
    return rho, np.asarray(b.bader_volumes), int(b.bader_maxima.shape[0]), np.asarray(b.atoms_volumes)


def test_bond_graph_on_the_librarys_own_maps():
    rho, bader, n_max, atoms = library_maps('atoms8_24', synth.ATOMS8)
    for what, lab, n in (('bader volumes', bader, n_max), ('atom map', atoms, 8)):
        g = critical.bond_graph(rho, lab, n)
        want = reference_bonds(rho, lab, n)
        print(what, 'n', n, 'pairs', len(g), 'saddles', g.saddles.tolist(), 'same_basin', g.same_basin)
        same_bonds((g.pairs, g.saddles, g.rho_b, g.voxel, g.same_basin), want, what)
        assert len(g) > 0 and np.array_equal(g.voxels, np.stack(np.unravel_index(g.voxel, rho.shape), axis=1))


def test_the_2x2x2_arrangement_has_its_twelve_bonds_twice():
    rho, bader, n_max, atoms = library_maps('grid2x2x2', ATOMS_2X2X2)
    g = critical.bond_graph(rho, atoms, 8)
    same_bonds((g.pairs, g.saddles, g.rho_b, g.voxel, g.same_basin), reference_bonds(rho, atoms, 8), 'atom map')
    cells = np.rint(ATOMS_2X2X2[:, :3] * 2 - 0.5).astype(int)
    nearest = sorted((a, b) for a in range(8) for b in range(a + 1, 8) if np.abs(cells[a] - cells[b]).sum() == 1)
    print('pairs', g.pairs.tolist(), 'saddles', g.saddles.tolist(), 'same_basin', g.same_basin)
    assert [tuple(p) for p in g.pairs.tolist()] == nearest and len(nearest) == 12
    assert g.saddles.tolist() == [2] * 12 and g.same_basin == 0
    cp = critical.critical_points(rho)
    assert cp.counts.tolist() == [8, 24, 24, 24, 24, 8] and cp.euler == 0
    assert sorted(g.neighbours(0).tolist()) == [b for a, b in nearest if a == 0]


def test_bond_graph_on_noise_labels(ctx):
    """labels -1 .. 5 in blobs on the noisy grid with n = 5: many pairs, bond voxels inside one basin, labels that count for nothing"""
    rho = case('rough')
    lab = noise_labels(rho.shape, 5)
    assert lab.min() == -1 and lab.max() == 5
    want = reference_bonds(rho, lab, 5)
    assert len(want[0]) == 10 and want[4] > 0 and want[1].max() > 2
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    ctx.upload_labels(lab)
    before = ctx.download_labels(np.int32)
    ctx.critical_points()
    same_bonds(ctx.critical_bonds(5), want, 'noise labels')
    assert np.array_equal(ctx.download_labels(np.int32), before) and np.array_equal(ctx.download_density(), rho), 'nothing resident is written'
    # the vacuum carries over from the list, and a smaller n drops the pairs of the labels it leaves out
    ctx.critical_points(VACUUM_TOL)
    same_bonds(ctx.critical_bonds(3), reference_bonds(rho, lab, 3, VACUUM_TOL), 'noise labels, vacuum, n = 3')
    g = critical.bond_graph(rho, lab.astype(np.int8), 5)
    same_bonds((g.pairs, g.saddles, g.rho_b, g.voxel, g.same_basin), want, 'through critical.bond_graph')


# ---- error codes and bookkeeping ---------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        rho = case('synth8')
        for call in (c.critical_points, lambda: c.critical_bonds(2)):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no grid
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9))
        with pytest.raises(_lib.BaderHipError) as e:
            c.critical_points()
        assert e.value.code == _lib.XB_E_STATE                      # no density
        c.upload_density(rho)
        counts, n = (C.c_int64 * 6)(*([-7] * 6)), C.c_int64(-7)
        nan = float('nan')
        assert c.lib.xb_critical_points(c.h, nan, 2, counts, C.byref(n)) == _lib.XB_E_ARG
        assert c.lib.xb_critical_points(c.h, nan, 0, None, C.byref(n)) == _lib.XB_E_ARG
        assert c.lib.xb_critical_points(c.h, nan, 0, counts, None) == _lib.XB_E_ARG
        assert list(counts) == [-7] * 6 and n.value == -7, 'a refused call writes nothing'
        buf = np.zeros(64, np.int64)
        assert c.lib.xb_critical_fetch(c.h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 64) == _lib.XB_E_STATE
        with pytest.raises(_lib.BaderHipError) as e:
            c.critical_bonds(2)
        assert e.value.code == _lib.XB_E_STATE                      # no labels
        c.upload_labels(np.zeros(rho.shape, np.int32))
        with pytest.raises(_lib.BaderHipError) as e:
            c.critical_bonds(2)
        assert e.value.code == _lib.XB_E_STATE                      # no list
        got = c.critical_points()
        same_points(got, reference('synth8'), 'synth8')
        p = got[1].size
        assert p > 1
        assert c.lib.xb_critical_fetch(c.h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, p - 1) == _lib.XB_E_ARG
        assert c.lib.xb_critical_fetch(c.h, None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, p) == _lib.XB_E_ARG
        a, b = C.c_int64(-7), C.c_int64(-7)
        assert c.lib.xb_critical_bonds(c.h, 0, C.byref(a), C.byref(b)) == _lib.XB_E_ARG
        assert c.lib.xb_critical_bonds(c.h, 2, None, C.byref(b)) == _lib.XB_E_ARG
        assert (a.value, b.value) == (-7, -7)
        assert c.lib.xb_critical_bonds_fetch(c.h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 64) == _lib.XB_E_STATE
        pairs, saddles, rho_b, voxel, same = c.critical_bonds(1)
        assert pairs.shape == (0, 2) and same == got[0][_lib.XB_CRITICAL_BOND_VOXELS]      # one basin everywhere
        assert c.lib.xb_critical_bonds_fetch(c.h, None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 64) == _lib.XB_E_ARG
        # a new density discards the list; a slab is refused
        c.upload_density(rho)
        with pytest.raises(_lib.BaderHipError) as e:
            c.critical_bonds(1)
        assert e.value.code == _lib.XB_E_STATE
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(rho)
        with pytest.raises(_lib.BaderHipError) as e:
            c.critical_points()
        assert e.value.code == _lib.XB_E_STATE
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9))
        same_points(c.critical_points(), reference('synth8'), 'synth8 again')
    finally:
        c.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
def test_host_and_device_inputs_and_resident():
    ctx = _lib.default_context()
    rho = case('tric24')
    want = reference('tric24')
    cp = critical.critical_points(rho)
    same_points((cp.counts, cp.lin, cp.masks, cp.ring, cp.bond), want, 'host array')
    assert cp.kinds.dtype == np.uint8 and len(cp) == want[1].size and cp.euler == 0
    assert ((cp.kinds & critical.NUCLEAR) > 0).sum() == want[0][0] and ((cp.kinds & critical.CAGE) > 0).sum() == want[0][5]
    assert ((cp.kinds & critical.BOND) > 0).sum() == want[0][1] and ((cp.kinds & critical.RING) > 0).sum() == want[0][3]
    flood = critical.critical_points(rho, flood=True)
    assert np.array_equal(flood.lin, cp.lin) and np.array_equal(flood.kinds, cp.kinds)
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    ctx.upload_labels(np.zeros(rho.shape, np.int8))
    dev = ctx.export_volume(0)          # a library-owned device array holding the density
    assert device.is_device_array(dev)
    cd = critical.critical_points(dev, vacuum_tol=0.05)
    same_points((cd.counts, cd.lin, cd.masks, cd.ring, cd.bond), reference_points(rho, 0.05), 'device array, vacuum')
    with utils.resident(rho):
        a = critical.critical_points(rho)
        lab = noise_labels(rho.shape, 4)
        g = critical.bond_graph(rho, lab, 4)
    assert np.array_equal(a.lin, cp.lin)
    same_bonds((g.pairs, g.saddles, g.rho_b, g.voxel, g.same_basin), reference_bonds(rho, lab, 4), 'resident')
    empty = critical.bond_graph(rho, lab, 0)
    assert len(empty) == 0 and empty.same_basin == 0


def test_bader_with_the_flag():
    """two unequal atoms at 24^3 with a vacuum tolerance.  The synthetic density is rounded to multiples of 2^-20, which makes
    every charge sum exact in any order: the flag-off attributes can then be compared bit for bit between two runs"""
    shape, lat = (24, 24, 24), synth.CUBIC6
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5, 0.0) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(atoms5, lat)
    tol = 2.0 ** -10
    off = Bader({'charge': rho.copy()}, lat, atoms, vacuum_tol=tol)
    off()
    on = Bader({'charge': rho.copy()}, lat, atoms, vacuum_tol=tol, critical_flag=True)
    on()
    new = {'critical_points', 'critical_counts', 'critical_voxels', 'critical_kinds', 'critical_positions', 'atoms_bond_graph',
           'atoms_bonds', 'atoms_bond_saddles', 'atoms_bond_density', 'atoms_bond_position', 'bader_bond_graph', 'bader_bonds'}
    assert set(vars(on)) - set(vars(off)) == new | {'critical_flag'}
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference'):
            continue
        got = getattr(on, key)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert got == want, key
    want = reference_points(rho, tol)
    cp = on.critical_points
    same_points((cp.counts, cp.lin, cp.masks, cp.ring, cp.bond), want, 'Bader')
    assert np.array_equal(on.critical_counts, want[0]) and np.array_equal(on.critical_kinds, cp.kinds)
    assert np.array_equal(on.critical_voxels, np.stack(np.unravel_index(want[1], shape), axis=1))
    assert np.array_equal(on.critical_positions, critical.positions(on.critical_voxels, shape, lat) + on.voxel_offset)
    ab = reference_bonds(rho, on.atoms_volumes, 2, tol)
    same_bonds((on.atoms_bonds, on.atoms_bond_saddles, on.atoms_bond_density, on.atoms_bond_graph.voxel, on.atoms_bond_graph.same_basin),
               ab, 'Bader, atoms')
    g = on.atoms_bond_graph
    assert np.array_equal(on.atoms_bond_position, critical.positions(g.voxels, shape, lat) + on.voxel_offset)
    # (between these two narrow atoms the bond point lies in the vacuum, which keeps it off the list; without the tolerance it is there)
    free = critical.bond_graph(rho, on.atoms_volumes, 2)
    same_bonds((free.pairs, free.saddles, free.rho_b, free.voxel, free.same_basin), reference_bonds(rho, on.atoms_volumes, 2), 'no vacuum')
    bb = reference_bonds(rho, on.bader_volumes, on.bader_maxima.shape[0], tol)
    g = on.bader_bond_graph
    same_bonds((on.bader_bonds, g.saddles, g.rho_b, g.voxel, g.same_basin), bb, 'Bader, volumes')
    # with adjacency_flag as well, bond_surfaces() keeps its three attributes and the bond graph stays in atoms_bond_graph
    both = Bader({'charge': rho.copy()}, lat, atoms, vacuum_tol=tol, critical_flag=True, adjacency_flag=True)
    both()
    assert both.atoms_bond_density.shape == both.atoms_bond_area.shape and np.array_equal(both.atoms_bond_graph.rho_b, on.atoms_bond_density)

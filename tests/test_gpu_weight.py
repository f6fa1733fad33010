"""The weight method on the GPU (csrc/k_weight.h, host_weight.h) against the plain float64 restatement of
tests/test_weight_cpu.py: the same maxima in the same order, charge and volume EQUAL (np.array_equal) -- every A_i has one
writer, a fixed neighbour order and no contracted multiply-add, so there is nothing to tolerate.

Shapes, the smallest that reach each mechanism: a two-basin cubic cell; a triclinic grid no axis of which is a multiple of the
4 x 4 x 16 tile and whose edge / corner neighbours carry weight; axes of one, two and three voxels (the wrap makes +1 and -1 the
same voxel, or the voxel itself); a ramp whose ascending chain is longer than one batch of level launches and ends in the
single-workgroup tail; a third of the voxels vacuum; a density quantised to eight values (plateaus, well over a thousand
maxima).  The sums of the Bader run are compared under the bound derived in tests/test_weight_cpu.py."""
import math

import numpy as np
import pytest

from pybader_amd import _lib, interface, utils, weight
from test_weight_cpu import bound, case, case_alpha, case_reference, gaussians, other_field, restate

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def voxel_volume(name):
    rho, lat, _ = case(name)
    return abs(np.linalg.det(lat)) / rho.size


def run(ctx, name, q=None):
    rho, lat, labels = case(name)
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    if labels is None:
        ctx.vacuum_assign(None, 1.0)
    else:
        ctx.upload_labels(labels)
    return ctx.weight_sum(case_alpha(name), voxel_volume(name), q)


def same(got, want, vv):
    idx, ch, vo = got
    m, A, V, _ = want
    assert idx.shape == m.shape, (idx.size, m.size)            # n_maxima
    assert np.array_equal(idx, m)
    assert np.array_equal(ch, A * vv)
    assert np.array_equal(vo, V * vv)


@pytest.mark.parametrize('name', ['gauss2', 'tric', 'thin325', 'thin147', 'vacuum', 'quant8'])
def test_equals_the_restatement(ctx, name):
    same(run(ctx, name), case_reference(name), voxel_volume(name))
    st = ctx.weight_stats()
    rho, _, labels = case(name)
    assert st['levels'] == case_reference(name)[3]
    assert st['voxels'] == (rho.size if labels is None else int((labels != -1).sum()))


def test_long_chain_runs_batched_levels_and_the_single_workgroup_tail(ctx):
    same(run(ctx, 'ramp'), case_reference('ramp'), voxel_volume('ramp'))
    st = ctx.weight_stats()
    assert st['levels'] == case_reference('ramp')[3] >= 200
    assert st['levels_batched'] >= 1 and st['levels_tail'] >= 1, st            # both routes ran
    assert st['levels_batched'] + st['levels_tail'] == st['levels']
    assert st['batches'] < st['levels'] // 8, st                               # no host wait per level


def test_vacuum_marks_are_honoured_and_nothing_is_written(ctx):
    rho, _, labels = case('vacuum')
    got = run(ctx, 'vacuum')
    assert np.array_equal(ctx.download_density(), rho) and np.array_equal(ctx.download_labels(np.int32), labels)
    ctx.vacuum_assign(None, 1.0)                                               # the same density without the marks
    free = ctx.weight_sum(case_alpha('vacuum'), voxel_volume('vacuum'))
    same(free, restate(rho, rho, case_alpha('vacuum')), voxel_volume('vacuum'))
    assert free[0].size != got[0].size or not np.array_equal(free[1], got[1])


@pytest.mark.parametrize('name', ['tric', 'vacuum'])
def test_another_integrand_from_the_host(ctx, name):
    rho, _, labels = case(name)
    q = other_field(rho.shape)
    same(run(ctx, name, q), restate(rho, q, case_alpha(name), labels), voxel_volume(name))


@pytest.mark.skipif(torch is None, reason='torch-ROCm is not installed')
@pytest.mark.parametrize('how', ['f64', 'f32', 'f32_permuted', 'f64_sliced'])
def test_another_integrand_from_a_device_array(ctx, how):
    rho, _, _ = case('tric')
    q = other_field(rho.shape)
    if how == 'f64':
        t = torch.as_tensor(q.copy(), device='cuda')
    elif how == 'f32':
        t = torch.as_tensor(q.astype(np.float32), device='cuda')
    elif how == 'f32_permuted':
        t = torch.as_tensor(np.ascontiguousarray(q.astype(np.float32).transpose(2, 0, 1)), device='cuda').permute(1, 2, 0)
    else:
        big = torch.zeros((rho.shape[0], rho.shape[1], 2 * rho.shape[2]), dtype=torch.float64, device='cuda')
        big[:, :, ::2] = torch.as_tensor(q.copy(), device='cuda')
        t = big[:, :, ::2]
    assert tuple(t.shape) == rho.shape
    same(run(ctx, 'tric', t), restate(rho, q, case_alpha('tric')), voxel_volume('tric'))


def test_bad_arguments_are_error_codes(ctx):
    rho, _, _ = case('gauss2')
    run(ctx, 'gauss2')
    skew = case_alpha('gauss2').copy()
    skew[1, 0, 0] *= 1.5
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.weight_sum(skew, 1.0)
    assert e.value.code == _lib.XB_E_ARG
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9), (2, 9))                 # a slab: refused
    ctx.set_halo(2)
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.weight_sum(case_alpha('gauss2'), 1.0)
    assert e.value.code == _lib.XB_E_STATE
    ctx.set_grid((3, 2, 5), np.zeros(27), np.zeros(9))                         # a thin grid: no assignment
    ctx.upload_density(case('thin325')[0])
    ctx.vacuum_assign(None, 1.0)
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.assign('neargrid')
    assert e.value.code == _lib.XB_E_ARG


def test_memory_stats_count_the_buffers(ctx):
    rho, _, _ = case('tric')
    run(ctx, 'tric')
    st = ctx.weight_stats()
    assert st['bytes'] == 25 * rho.size
    total, _, scratch = ctx.memory_stats()
    assert scratch >= st['bytes'] + 8 * rho.size and total > scratch


def test_public_function_host_device_and_resident():
    rho, lat, _ = case('gauss2')
    m, A, V, _ = case_reference('gauss2')
    vv = np.abs(np.dot(lat[0], np.cross(*lat[1:]))) / np.prod(rho.shape)
    want = np.stack(np.unravel_index(m, rho.shape), axis=1)
    with utils.resident(rho):
        for _ in range(2):
            maxima, ch, vo = weight.weight_sum(rho, rho, lat)
            assert maxima.dtype == np.int64 and np.array_equal(maxima, want)
            assert np.array_equal(ch, A * vv) and np.array_equal(vo, V * vv)
    rho_v, lat_v, labels = case('vacuum')
    mv, Av, Vv, _ = case_reference('vacuum')
    vvv = np.abs(np.dot(lat_v[0], np.cross(*lat_v[1:]))) / np.prod(rho_v.shape)
    maxima, ch, vo = weight.weight_sum(rho_v, rho_v, lat_v, labels.astype(np.int16))
    assert np.array_equal(maxima, np.stack(np.unravel_index(mv, rho_v.shape), axis=1)) and np.array_equal(ch, Av * vvv)
    if torch is not None:
        t = torch.as_tensor(rho.copy(), device='cuda')
        maxima, ch, vo = weight.weight_sum(t, t, lat)
        assert np.array_equal(maxima, want) and np.array_equal(ch, A * vv) and np.array_equal(vo, V * vv)


# ---- interface.Bader ------------------------------------------------------------------------------------------------------
TODAY = {'_density', '_lattice', '_atoms', '_file_info', 'density', 'reference', 'method', 'refine_method', 'vacuum_tol',
         'refine_mode', 'threads', 'speed_flag', 'spin_flag', 'export_mode', 'fortran_format', 'vacuum_charge', 'vacuum_volume',
         'bader_volumes', '_bader_maxima', 'bader_charge', 'bader_volume', 'bader_atoms', 'bader_distance', 'atoms_volumes',
         'atoms_surface_distance', 'atoms_charge', 'atoms_volume'}
NEW = {'weight_flag', 'weight_maxima', 'weight_charge', 'weight_volume', 'weight_atoms', 'atoms_weight_charge',
       'atoms_weight_volume'}


def two_atom_cell():
    shape, lat = (20, 16, 18), np.diag([5.0, 4.0, 4.5])
    frac = np.array([[0.27, 0.5, 0.5], [0.73, 0.5, 0.5]])
    rho = gaussians(shape, lat, frac, [0.55, 0.7], [3.0, 2.0], background=0.02)
    spin = gaussians(shape, lat, frac, [0.5, 0.5], [0.4, -0.3], background=0.0)
    return rho, spin, lat, frac @ lat


def test_bader_with_weight_flag():
    rho, spin, lat, atoms = two_atom_cell()
    b = interface.Bader({'charge': rho, 'spin': spin}, lat, atoms, weight_flag=True, spin_flag=True)
    b()
    n, M = 2, b.weight_maxima.shape[0]
    assert set(vars(b)) == TODAY | NEW | {'atoms_weight_spin', 'bader_spin', 'atoms_spin'}
    assert b.weight_maxima.shape == (M, 3) and b.weight_maxima.dtype == np.int64 and M >= 2
    assert b.weight_charge.shape == b.weight_volume.shape == b.weight_atoms.shape == (M,)
    assert b.atoms_weight_charge.shape == b.atoms_weight_volume.shape == b.atoms_weight_spin.shape == (n,)
    assert set(b.weight_atoms.tolist()) == {0, 1}
    vv = b.voxel_volume
    al = weight.voronoi_weights(lat / np.array(rho.shape, dtype=np.float64)[:, None])
    m, A, V, levels = restate(rho, rho, al)
    assert np.array_equal(b.weight_maxima, np.stack(np.unravel_index(m, rho.shape), axis=1))
    assert np.array_equal(b.weight_charge, A * vv) and np.array_equal(b.weight_volume, V * vv)
    # nothing lost: both sets of atomic charges add up to the cell's charge
    for field, per_atom, grid in ((rho, b.atoms_weight_charge, b.atoms_charge), (spin, b.atoms_weight_spin, b.atoms_spin)):
        total, mag = math.fsum(field.reshape(-1)) * vv, math.fsum(np.abs(field.reshape(-1))) * vv
        print('sum of weight charges', math.fsum(per_atom), 'of grid charges', math.fsum(grid), 'cell', total)
        assert abs(math.fsum(per_atom) - total) <= bound(levels, M + n + 1, mag)
        assert abs(math.fsum(grid) - total) <= (rho.size + n + 2) * 2.0 ** -53 * mag     # the bound of tests/test_gpu_sums.py
    assert abs(math.fsum(b.atoms_weight_volume) - b.lattice_volume) <= bound(levels, M + n + 1, b.lattice_volume)
    assert (b.atoms_weight_charge > 0).all() and (b.atoms_weight_volume > 0).all()


def test_bader_without_the_flag_is_todays_run():
    rho, spin, lat, atoms = two_atom_cell()
    b = interface.Bader({'charge': rho}, lat, atoms)
    b()
    assert b.weight_flag is False and set(vars(b)) == TODAY
    v = interface.Bader({'charge': rho}, lat, atoms, vacuum_tol=0.05, weight_flag=True)
    v()
    assert set(vars(v)) == TODAY | NEW
    # (1e-9: four decades above any rounding bound of this file, five below the share of a single voxel of the 5760)
    live = rho > 0.05
    total = math.fsum(rho[live]) * v.voxel_volume
    assert abs(math.fsum(v.atoms_weight_charge) - total) <= 1e-9 * total and abs(math.fsum(v.atoms_charge) - total) <= 1e-9 * total
    assert abs(math.fsum(v.atoms_weight_volume) - live.sum() * v.voxel_volume) <= 1e-9 * v.lattice_volume


def test_without_a_map_the_resident_labels_are_left_alone_and_buffers_can_be_released():
    rho, lat, labels = case('vacuum')
    ctx = _lib.default_context()
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_labels(labels)
    maxima, ch, vo = weight.weight_sum(rho, rho, lat)                          # volumes=None: the marks are ignored ...
    vv = np.abs(np.dot(lat[0], np.cross(*lat[1:]))) / np.prod(rho.shape)
    m, A, V, _ = restate(rho, rho, case_alpha('vacuum'))
    assert np.array_equal(maxima, np.stack(np.unravel_index(m, rho.shape), axis=1)) and np.array_equal(ch, A * vv)
    assert np.array_equal(ctx.download_labels(np.int32), labels)               # ... and the map is still there
    idx, ch2, _ = ctx.weight_sum(case_alpha('vacuum'), vv)                     # the switch does not outlive the call
    assert np.array_equal(idx, case_reference('vacuum')[0])
    before = ctx.memory_stats()[0]
    ctx.weight_release()
    assert ctx.weight_stats()['bytes'] == 0 and ctx.memory_stats()[0] == before - 25 * rho.size
    with pytest.raises(_lib.BaderHipError) as e:                               # the results went with the buffers
        _lib.check(ctx.lib.xb_weight_fetch(ctx.h, None, None, None, 0))
    assert e.value.code == _lib.XB_E_STATE
    idx3, ch3, _ = ctx.weight_sum(case_alpha('vacuum'), vv)                    # allocates again
    assert np.array_equal(idx3, idx) and np.array_equal(ch3, ch2)
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.weight_sum(case_alpha('vacuum'), vv, np.zeros((3, 3, 3)))
    assert e.value.code == _lib.XB_E_ARG

"""xb_dori_field / xb_dori_sum and what stands on them (-m gpu) against the numpy restatement of tests/test_dori_cpu.py.

gamma, x = sign(lambda2) rho, the counts of the region, the domains and the surface's connectivity are compared with == : every
operation that decides them is bit-defined (include/bader_hip.h) -- gamma itself included, which has no sqrt and no cbrt in it.
XB_STENCIL_GATHER is the second implementation: everything runs through the tiles and through the gather.  THE BOUND of the
sums, per key 3 a + class, for the sum of rho and the sum of rho^2 alike (tests/test_gpu_laplacian.py's, taken from there):

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

tests/test_dori_cpu.py::test_the_bound_notices_a_voxel_in_the_wrong_class_or_on_the_wrong_side (collected here as well) shows for
every input used here that one voxel in the wrong class, or one voxel dropped from the region, breaks this bound."""
import ctypes as C

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

import history_common as H
from pybader_amd import _lib, device, dori, isosurface, synth, thread_handlers, utils
from pybader_amd.interface import Bader
from test_dori_cpu import (SUM_CUTS, SYMMETRIC_SHAPES, bits, check_sums, classes, keys, restated, sum_reference, sum_values,
                           symmetric_density, symmetric_points, ten_of, values)
from test_dori_cpu import test_the_bound_notices_a_voxel_in_the_wrong_class_or_on_the_wrong_side  # noqa: F401 -- runs here too
from test_gpu_history import Runner
from test_laplacian_cpu import sum_bound
from test_multipole_cpu import VV, label_map
from test_nci_cpu import LABELS_LDS, LATS, density, sum_inputs
from test_regions_cpu import components, per_component

pytestmark = pytest.mark.gpu
# every axis below the 8 x 8 x 32 tile; one past and across the tile on each axis
FIELD_SHAPES = [(5, 6, 7), (9, 7, 33), (20, 9, 33), (13, 17, 19), (12, 16, 40)]
RHO_MINS = [0.0, 1e-3, 0.05]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def have_torch():
    return torch is not None and torch.cuda.is_available()


def host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


def same_bits(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    diff = bits(got) != bits(want)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ from the restatement, first at {np.argwhere(diff)[0].tolist()}'


def load(ctx, rho):
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)


def check_every_route(ctx, lat, rho_min, v, what):
    """gamma and x through tiles and gather, to host and device outputs, with and without x"""
    for gather in (False, True):
        for on_device in (False, True):
            for colour in (True, False):
                g, x = ctx.dori_field(lat, rho_min, gather=gather, on_device=on_device, colour=colour)
                where = f'{what}, gather {gather}, device output {on_device}, x {colour}'
                if on_device:
                    assert isinstance(g, device.DeviceArray) and g.shape == v['gamma'].shape and g.dtype == np.float64
                same_bits(host(g), v['gamma'], where + ': gamma')
                if colour:
                    same_bits(host(x), v['x'], where + ': x')
                else:
                    assert x is None


# ---- the fields -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', FIELD_SHAPES)
def test_fields_equal_the_restatement_through_both_routes(ctx, shape, lname):
    rho, lat = density('holes', shape, lname), LATS[lname]
    load(ctx, rho)
    for rho_min in RHO_MINS:
        v = values('holes', shape, lname, rho_min)
        check_every_route(ctx, lat, rho_min, v, f'{shape} {lname} rho_min {rho_min}')
        assert (v['gamma'] > 0.5).any() and (v['gamma'] == 0).any() and (v['x'] < 0).any() and (v['x'] > 0).any()
    assert np.array_equal(ctx.download_density().view(np.uint64), rho.view(np.uint64)), 'the resident density is not written'


def test_rho_min_equal_to_a_voxels_density_pins_the_greater_than(ctx):
    shape, lname = (13, 17, 19), 'tric'
    rho, lat = density('holes', shape, lname), LATS[lname]
    base = values('holes', shape, lname, 0.0)
    at = np.unravel_index(int(np.flatnonzero((base['gamma'] > 0.25).reshape(-1))[7]), shape)
    rho_min = float(rho[at])
    on, below = restated(rho, lat, rho_min), restated(rho, lat, float(np.nextafter(rho_min, 0.0)))
    assert on['gamma'][at] == 0.0 and on['x'][at] == 0.0 and below['gamma'][at] > 0.25, 'rho > rho_min, not >='
    load(ctx, rho)
    for gather in (False, True):
        g, x = ctx.dori_field(lat, rho_min, gather=gather)
        same_bits(g, on['gamma'], f'rho_min on the voxel, gather {gather}')
        same_bits(x, on['x'], f'rho_min on the voxel, gather {gather}: x')
        g, _ = ctx.dori_field(lat, float(np.nextafter(rho_min, 0.0)), gather=gather, colour=False)
        same_bits(g, below['gamma'], f'rho_min one ulp below the voxel, gather {gather}')


@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', SYMMETRIC_SHAPES)
def test_the_symmetric_integer_density_on_the_device(ctx, shape, lname):
    """the S == 0 rule: gamma == 1.0 at exactly the 8 voxels about which the density is even, through both routes"""
    rho, lat = symmetric_density(shape), LATS[lname]
    v = restated(rho, lat, 0.0)
    load(ctx, rho)
    check_every_route(ctx, lat, 0.0, v, f'symmetric {shape} {lname}')
    g, _ = ctx.dori_field(lat, 0.0, colour=False)
    assert np.array_equal(g == 1.0, symmetric_points(shape)) and (g == 1.0).sum() == 8
    assert not ctx.dori_field(lat, 200.0, colour=False)[0].any(), 'rho_min comes before the S == 0 rule'


def test_fields_and_sums_of_a_constant_density(ctx):
    shape = (5, 6, 7)
    load(ctx, np.full(shape, 0.03125))
    ctx.upload_labels(np.zeros(shape, np.int32))
    for gather in (False, True):
        g, x = ctx.dori_field(LATS['tric'], 0.0, gather=gather)
        assert not g.any() and not x.any() and not np.signbit(g).any() and not np.signbit(x).any()
        count, charge, charge2 = ctx.dori_sum(LATS['tric'], 1, VV, 0.5, 0.0, 0.01, gather)
        assert not count.any() and not charge.any() and not charge2.any()


@pytest.mark.parametrize('k', [-40, 30])
def test_a_density_scaled_by_a_power_of_two_gives_the_same_bits(ctx, k):
    shape, lname = (13, 17, 19), 'tric'
    rho, lat = density('holes', shape, lname), LATS[lname]
    for rho_min in (0.0, 1e-3):
        base = values('holes', shape, lname, rho_min)
        load(ctx, rho * 2.0 ** k)
        for gather in (False, True):
            g, x = ctx.dori_field(lat, rho_min * 2.0 ** k, gather=gather)
            same_bits(g, base['gamma'], f'2^{k}, gather {gather}')
            same_bits(x, base['x'] * 2.0 ** k, f'2^{k}, gather {gather}: x')
    load(ctx, rho)
    for j in (-3, 10):
        same_bits(ctx.dori_field(lat * 2.0 ** j, 1e-3, colour=False)[0], base['gamma'], f'the lattice times 2^{j}')


def test_fields_of_device_tensors_and_a_host_array_through_the_python_layer():
    shape, lname, rho_min = (20, 9, 33), 'tric', 1e-3
    rho, lat = density('holes', shape, lname), LATS[lname]
    v = values('holes', shape, lname, rho_min)
    g, x = dori.dori_fields(rho, lat, rho_min)
    assert isinstance(g, np.ndarray) and isinstance(x, np.ndarray)
    same_bits(g, v['gamma'], 'host array')
    same_bits(x, v['x'], 'host array: x')
    g, x = dori.dori_fields(rho, lat, rho_min, colour=False)
    assert x is None
    same_bits(g, v['gamma'], 'host array, gamma alone')
    with utils.resident(rho):
        for gather in (True, False):
            g2, x2 = dori.dori_fields(rho, lat, rho_min, gather=gather)
            same_bits(g2, v['gamma'], f'resident, gather {gather}')
            same_bits(x2, v['x'], f'resident, gather {gather}: x')
    lin = np.flatnonzero((v['gamma'] > 0.3).reshape(-1))[::5]
    same_bits(dori.bond_dori(rho, lat, lin, rho_min), v['gamma'].reshape(-1)[lin], 'bond_dori')
    if not have_torch():
        pytest.skip('the host array passed; torch with a GPU is needed for a device tensor')
    rho32 = rho.astype(np.float32)
    v32 = restated(rho32.astype(np.float64), lat, rho_min)
    perm = torch.as_tensor(np.ascontiguousarray(rho.transpose(2, 0, 1)), device='cuda').permute(1, 2, 0)
    assert tuple(perm.shape) == shape and not perm.is_contiguous()
    for what, t, want in (('float32 tensor', torch.as_tensor(rho32.copy(), device='cuda'), v32), ('permuted float64 tensor', perm, v)):
        for gather in (False, True):
            gd, xd = dori.dori_fields(t, lat, rho_min, gather=gather)
            assert isinstance(gd, device.DeviceArray) and isinstance(xd, device.DeviceArray)
            same_bits(gd.to_host(), want['gamma'], f'{what}, gather {gather}')
            same_bits(xd.to_host(), want['x'], f'{what}, gather {gather}: x')
            back = torch.as_tensor(gd, device='cuda')        # (the result publishes the interface: no copy)
            assert back.dtype == torch.float64 and tuple(back.shape) == shape


# ---- the region's sums ------------------------------------------------------------------------------------------------------------
def test_sums_on_every_input_through_both_routes(ctx):
    assert LABELS_LDS == 85
    resident = None
    for what, kind, shape, lname, lab, n in sum_inputs():
        rho, v = density(kind, shape, lname), sum_values(kind, shape, lname)
        if resident != (kind, shape, lname):
            load(ctx, rho)
            resident = (kind, shape, lname)
        ctx.upload_labels(lab)
        for gather in (False, True):
            cnt = check_sums(ctx.dori_sum(LATS[lname], n, VV, *SUM_CUTS, gather), v, lab, n, f'{what}, gather {gather}')
        assert all(cnt[c::3].sum() >= 57 for c in range(3)), 'every class holds voxels'
    assert np.array_equal(ctx.download_labels(np.int32), lab) and np.array_equal(ctx.download_density(), rho), 'nothing resident is written'


def test_d_cut_equal_to_a_voxels_gamma_pins_the_greater_or_equal():
    shape, lname, n = (20, 9, 33), 'cubic', 3
    rho, lat, v = density('holes', shape, lname), LATS[lname], values('holes', shape, lname, 0.0)
    lab = label_map(shape, n)
    ok = (v['gamma'] > 0.3) & (v['gamma'] < 0.9) & (lab >= 0) & (lab < n)
    at = int(np.flatnonzero(ok.reshape(-1))[11])
    d_cut = float(v['gamma'].reshape(-1)[at])
    cuts = (d_cut, 0.0, 0.03)
    k = keys(v, lab, n, d_cut, 0.03)
    assert k[at] >= 0 and (v['gamma'] > d_cut).sum() == (v['gamma'] >= d_cut).sum() - 1, 'the voxel lies ON the bound, alone'
    for gather in (False, True):
        r = dori.dori_regions(rho, lab.astype(np.int8), lat, n, VV, *cuts, gather=gather)
        cnt = check_sums((r.count, r.charge, r.charge2), v, lab, n, f'd_cut on a voxel, gather {gather}', cuts)
        assert cnt.sum() == int((k >= 0).sum()) and np.array_equal(r.volume, r.count.astype(np.float64) * VV)
        assert (r.d_cut, r.rho_min, r.rho_split) == cuts
    g = dori.dori_fields(rho, lat, 0.0, colour=False)[0]
    assert int(((g >= d_cut) & (lab >= 0) & (lab < n)).sum()) == cnt.sum(), 'the stored field meets the same comparison'
    empty = dori.dori_regions(rho, lab, lat, 0, VV)
    assert empty.count.shape == empty.charge.shape == empty.volume.shape == (0, 3)


def test_the_buffer_is_counted():
    shape = (13, 17, 19)
    c = _lib.Context(0)
    try:
        load(c, density('holes', shape, 'tric'))
        c.upload_labels(label_map(shape, 2))
        before = c.memory_stats()
        c.dori_sum(LATS['tric'], 3000, VV, *SUM_CUTS)
        after = c.memory_stats()
        assert after[2] - before[2] == 72 * 3000 and after[0] - before[0] == after[2] - before[2]
        c.dori_sum(LATS['tric'], 2, VV, *SUM_CUTS)                       # (a smaller n fits the buffer)
        c.nci_sum(LATS['tric'], 3000, VV, 1.5, 1.0, 0.03)                # (the block is the NCI sums': no second one)
        c.dori_field(LATS['tric'], 0.0)                                  # (the fields go through scratch and a temporary)
        assert c.memory_stats() == after
    finally:
        c.close()


# ---- domains and surface ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(20, 9, 33), (13, 17, 19)])
def test_domains_equal_the_component_restatement_on_the_restated_gamma(shape):
    lname, level, rho_min, rho_split, n = 'tric', 0.5, 0.0, 0.03, 3
    rho, lat, v = density('holes', shape, lname), LATS[lname], values('holes', shape, lname, 0.0)
    lab = label_map(shape, n)
    reg, seeds = components(v['gamma'] >= level)
    m = seeds.size
    count, top, _ = per_component(reg, m, rho)
    assert m >= (2 if shape == (20, 9, 33) else 1) and (reg >= 0).any() and (reg < 0).any()
    ten = ten_of(rho, lat)
    d = dori.dori_domains(rho, lat, lab, n, VV, level, rho_min, rho_split)
    assert isinstance(d, dori.DoriDomains) and len(d) == d.m == m and isinstance(d.labels, np.ndarray)
    assert np.array_equal(d.labels, reg) and np.array_equal(d.seed, seeds) and np.array_equal(d.count, count) and np.array_equal(d.top, top)
    same_bits(d.value, dori.dori_value(ten[top], rho_min), 'value')
    same_bits(d.value, v['gamma'].reshape(-1)[top], 'value against the restated field')
    assert d.kind.dtype == np.int8 and np.array_equal(d.kind, dori.point_classes(ten[top], level, rho_min, rho_split))
    assert np.array_equal(d.kind, classes(v, rho_split).reshape(-1)[top]) and (d.value >= level).all()
    assert d.atoms.shape == (m, 2) and np.array_equal(d.volume, count.astype(np.float64) * VV)
    assert (d.level, d.rho_min, d.rho_split) == (level, rho_min, rho_split)
    # the same for a device density (the labels then stay there), without a label map
    c = _lib.default_context()
    e = dori.dori_domains(c.device_copy(rho), lat, level=level, rho_min=rho_min, rho_split=rho_split)
    assert isinstance(e.labels, device.DeviceArray) and np.array_equal(e.labels.to_host(), reg) and np.array_equal(e.top, top)
    assert np.array_equal(bits(e.value), bits(d.value)) and np.array_equal(e.kind, d.kind) and (e.atoms == -1).all()


def test_the_surface_is_the_isosurface_of_the_downloaded_fields():
    shape, lname, level, rho_min = (20, 9, 33), 'tric', 0.5, 1e-3
    rho, lat = density('holes', shape, lname), LATS[lname]
    a = dori.dori_isosurface(rho, lat, level, rho_min)
    g, x = dori.dori_fields(rho, lat, rho_min)
    want = isosurface.isosurface(g, lat, level, colour=x, density=rho)
    assert len(want.triangles) > 100
    b = dori.dori_isosurface(_lib.default_context().device_copy(rho), lat, level, rho_min)
    for got in (a, b):
        for name in ('vertices', 'colour', 'triangles', 'wrap', 'cells', 'positions'):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        # area and volume are float atomics in any order on both sides: two runs of at most 6 N + 2 terms bounded by the cell
        cell = abs(np.linalg.det(lat))
        lim = 2 * (6 * rho.size + 2) * 2.0 ** -53
        assert abs(got.area - want.area) <= lim * want.area and abs(got.volume - want.volume) <= lim * cell
    assert a.level == level and np.isfinite(a.vertices).all()


# ---- error codes --------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        shape = (8, 8, 8)
        rho = np.ascontiguousarray(density('rough', shape, 'cubic'))
        lat = LATS['cubic']
        n_vox = rho.size
        calls = (lambda: c.dori_field(lat, 0.0), lambda: c.dori_sum(lat, 2, VV, 0.5, 0.0, 0.01))
        for call in calls:
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        for call in calls:
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no density
        c.upload_density(rho)
        with pytest.raises(_lib.BaderHipError) as e:
            c.dori_sum(lat, 2, VV, 0.5, 0.0, 0.01)
        assert e.value.code == _lib.XB_E_STATE                      # no labels
        c.upload_labels(np.zeros(shape, np.int32))
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        lp = (C.c_double * 9)(*lat.reshape(-1))
        flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)          # a singular lattice
        out_g, out_x = np.full(n_vox, -7.0), np.full(n_vox, -7.0)
        pg, px = out_g.ctypes.data, out_x.ctypes.data
        dg, dx = device.DeviceArray(c, shape, np.float64), device.DeviceArray(c, shape, np.float64)
        vg, vx = C.c_void_p(dg.ptr), C.c_void_p(dx.ptr)
        lib, h, arg, limit = c.lib, c.h, _lib.XB_E_ARG, _lib.XB_E_LIMIT
        # the field: a null lattice, gamma on both sides or on neither, x on the other side or alone, unknown flag bits, a rho_min
        # that is negative or not finite, a singular lattice, host pointers as device outputs, a device output one element past
        # its allocation, one not aligned, the two the same, one that is the resident density
        assert lib.xb_dori_field(h, None, 0.0, 0, pg, px, None, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, pg, px, vg, vx) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, pg, None, vg, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, None, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, pg, None, None, vx) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, px, vg, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, px, None, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, None, vx) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 2, pg, px, None, None) == arg
        for bad in (-0.25, float('nan'), float('inf')):
            assert lib.xb_dori_field(h, lp, bad, 0, pg, px, None, None) == arg, bad
        assert lib.xb_dori_field(h, flat, 0.0, 0, pg, px, None, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, pg, px) == arg
        assert n_vox * 8 == dg.nbytes == 4096
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, vg, C.c_void_p(dx.ptr + 8)) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, C.c_void_p(dg.ptr + 4), vx) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, C.c_void_p(dg.ptr + 8), None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, vg, vg) == arg
        p_rho = C.c_void_p(int(lib.xb_density_ptr(h)))
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, p_rho, None) == arg
        assert lib.xb_dori_field(h, lp, 0.0, 0, None, None, vg, p_rho) == arg
        assert (out_g == -7.0).all() and (out_x == -7.0).all(), 'a refused call writes nothing'
        assert np.array_equal(c.download_density(), rho)
        # the sums: null pointers, unknown flag bits, n < 1, thresholds that are negative or not finite, d_cut outside (0, 1], a
        # singular lattice, n beyond the limit
        cnt, ch, ch2 = np.full(6, -7, np.int64), np.full(6, -7.0), np.full(6, -7.0)
        pc, pch, pch2 = cnt.ctypes.data_as(pi), ch.ctypes.data_as(pd), ch2.ctypes.data_as(pd)
        good = (0.5, 0.0, 0.01)
        assert lib.xb_dori_sum(h, None, 2, VV, *good, 0, pc, pch, pch2) == arg
        assert lib.xb_dori_sum(h, lp, 2, VV, *good, 0, None, pch, pch2) == arg
        assert lib.xb_dori_sum(h, lp, 2, VV, *good, 0, pc, None, pch2) == arg
        assert lib.xb_dori_sum(h, lp, 2, VV, *good, 0, pc, pch, None) == arg
        assert lib.xb_dori_sum(h, lp, 2, VV, *good, 4, pc, pch, pch2) == arg
        assert lib.xb_dori_sum(h, lp, 0, VV, *good, 0, pc, pch, pch2) == arg
        assert lib.xb_dori_sum(h, lp, -3, VV, *good, 0, pc, pch, pch2) == arg
        for k in (1, 2):
            for bad in (-0.25, float('nan'), float('inf')):
                cuts = list(good)
                cuts[k] = bad
                assert lib.xb_dori_sum(h, lp, 2, VV, *cuts, 0, pc, pch, pch2) == arg, (k, bad)
        for bad in (0.0, -0.0, -0.5, float(np.nextafter(1.0, 2.0)), 2.0, float('nan'), float('inf')):
            assert lib.xb_dori_sum(h, lp, 2, VV, bad, 0.0, 0.01, 0, pc, pch, pch2) == arg, bad
        assert lib.xb_dori_sum(h, flat, 2, VV, *good, 0, pc, pch, pch2) == arg
        assert lib.xb_dori_sum(h, lp, (2 ** 31 - 1) // 3 + 1, VV, *good, 0, pc, pch, pch2) == limit
        assert (cnt == -7).all() and (ch == -7.0).all() and (ch2 == -7.0).all()
        assert lib.xb_dori_sum(h, lp, 2, VV, 1.0, 0.0, 0.01, 0, pc, pch, pch2) == 0, 'd_cut = 1 is inside the range'
        assert cnt[2:].sum() == 0 and (cnt >= 0).all()
        with pytest.raises(ValueError):
            dori.dori_regions(rho, np.zeros((3, 3, 3), np.int32), lat, 2, VV)
        # a slab is refused (host outputs need the whole-grid scratch a slab context does not hold); the whole grid works again
        c.set_grid(shape, np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(rho)
        c.upload_labels(np.zeros(shape, np.int32))
        for call in calls:
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        same_bits(c.dori_field(lat, 0.0)[0], restated(rho, lat, 0.0)['gamma'], 'the whole grid again')
    finally:
        c.close()


# ---- call history -------------------------------------------------------------------------------------------------------------------
HISTORY_CUTS = (0.5, 0.0, 0.03)


def dori_call(kind, grid):
    """one of the calls through the public functions on density A and the atom map of a grid of history_common -> None, or what
    differs from the restatement (which is what a fresh context gives: the other tests of this file)"""
    rho, lab, n = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms')
    v = restated(rho, H.LAT, HISTORY_CUTS[1])
    if kind == 'fields':
        g, x = dori.dori_fields(rho, H.LAT, HISTORY_CUTS[1])
        if not np.array_equal(bits(g), bits(v['gamma'])) or not np.array_equal(bits(x), bits(v['x'])):
            return f'dori_fields on {grid}: differs'
        return None
    r = dori.dori_regions(rho, lab, H.LAT, n, VV, *HISTORY_CUTS)
    (s1, cnt, mag1), (s2, _, mag2) = sum_reference(v, lab, n, HISTORY_CUTS)
    if not np.array_equal(r.count.reshape(-1), cnt) or cnt.sum() < 100:
        return f'dori_regions on {grid}: counts differ'
    if not np.all(np.abs(r.charge.reshape(-1) - s1 * VV) <= sum_bound(cnt, mag1)):
        return f'dori_regions on {grid}: the sums of rho differ'
    if not np.all(np.abs(r.charge2.reshape(-1) - s2 * VV) <= sum_bound(cnt, mag2)):
        return f'dori_regions on {grid}: the sums of rho^2 differ'
    return None


@pytest.mark.parametrize('other', ['nci_regions', 'basin_laplacian', 'charge_sum', 'nci_histogram', 'regions', 'isosurface',
                                   'hirshfeld_charges', 'weight_own'])
@pytest.mark.parametrize('kind', ['fields', 'regions'])
def test_call_history_does_not_matter(kind, other, monkeypatch):
    """each DORI call directly before and directly after the other call, on G1 -> G2 -> G1 of history_common.GRIDS, on the default
    context: the other call's results are what they are without DORI, DORI's what a fresh context gives"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    run = Runner()
    bad = []
    try:
        for grid in ('G1', 'G2', 'G1'):
            for step in (lambda: dori_call(kind, grid), lambda: run.checked(other, grid, 'A', 'atoms'), lambda: dori_call(kind, grid),
                         lambda: run.checked(other, grid, 'A', 'atoms')):
                msg = step()
                if msg:
                    bad.append(f'{grid}: {msg}')
        with utils.resident(H.density('G1', 'A')):
            for step in (lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: dori_call(kind, 'G1'),
                         lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: dori_call(kind, 'G1')):
                msg = step()
                if msg:
                    bad.append(f'resident(A): {msg}')
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, ' | '.join(bad[:4])


# ---- Bader(dori_flag=True) ------------------------------------------------------------------------------------------------------------
DORI_ATTRIBUTES = {'dori_flag', 'dori_cut', 'dori_rho_min', 'dori_rho_split', 'atoms_dori_count', 'atoms_dori_volume', 'atoms_dori_charge',
                   'critical_dori', 'atoms_bond_dori'}
DOMAIN_ATTRIBUTES = {'dori_domains_flag', 'dori_domains', 'dori_domain_count', 'dori_domain_volume', 'dori_domain_charge',
                     'dori_domain_kind', 'dori_domain_value', 'dori_domain_atoms', 'dori_domain_position'}


def test_bader_with_the_flags(monkeypatch):
    """the 8-atom synthetic at 24^3: every new attribute equals the direct calls and the restatement, and nothing else moves"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    shape, lat = (24, 24, 24), synth.TRICLINIC
    rho = synth.synth_density(shape, lat)
    atoms = synth.atoms_cartesian(synth.ATOMS8, lat)
    cuts = dict(dori_cut=0.5, dori_rho_min=0.02, dori_rho_split=0.03)

    def make(**flags):
        b = Bader({'charge': rho.copy()}, lat, atoms, **flags)
        b()
        return b

    off = make(critical_flag=True)
    on = make(critical_flag=True, dori_flag=True, dori_domains_flag=True, **cuts)
    assert off.dori_flag is False and off.dori_domains_flag is False and not (DORI_ATTRIBUTES | DOMAIN_ATTRIBUTES) & set(vars(off))
    assert set(vars(on)) - set(vars(off)) == DORI_ATTRIBUTES | DOMAIN_ATTRIBUTES
    assert np.array_equal(host(on.atoms_volumes), host(off.atoms_volumes))
    assert np.allclose(on.atoms_charge, off.atoms_charge, rtol=2.0 ** -40, atol=0)      # (float atomics: two runs of one sum)
    assert np.array_equal(on.critical_points.lin, off.critical_points.lin)
    n, vv = atoms.shape[0], on.voxel_volume
    d_cut, rho_min, rho_split = cuts.values()
    v = restated(rho, lat, rho_min)
    lab = np.asarray(host(on.atoms_volumes))
    (s1, cnt, mag1), _ = sum_reference(v, lab, n, (d_cut, rho_min, rho_split))
    print('atoms_dori_count', on.atoms_dori_count.tolist())
    assert on.atoms_dori_count.shape == (n, 3) and np.array_equal(on.atoms_dori_count.reshape(-1), cnt) and cnt.sum() > 100
    assert np.array_equal(on.atoms_dori_volume, on.atoms_dori_count.astype(np.float64) * vv)
    lim = sum_bound(cnt, mag1, vv)
    assert np.all(np.abs(on.atoms_dori_charge.reshape(-1) - s1 * vv) <= lim)
    direct = dori.dori_regions(on.reference, on.atoms_volumes, lat, n, vv, d_cut, rho_min, rho_split)
    assert np.array_equal(direct.count, on.atoms_dori_count) and np.array_equal(direct.volume, on.atoms_dori_volume)
    assert np.all(np.abs(direct.charge - on.atoms_dori_charge).reshape(-1) <= 2 * lim)      # (two runs of float atomics)
    for got, lin in ((on.critical_dori, on.critical_points.lin), (on.atoms_bond_dori, on.atoms_bond_graph.voxel)):
        assert got.shape == (len(lin),) and len(lin) > 0
        same_bits(got, v['gamma'].reshape(-1)[lin], 'gamma at listed voxels')
        same_bits(got, dori.bond_dori(on.reference, lat, lin, rho_min), 'bond_dori')
    d = dori.dori_domains(on.reference, lat, on.atoms_volumes, n, vv, d_cut, rho_min, rho_split)
    reg, seeds = components(v['gamma'] >= d_cut)
    assert d.m == on.dori_domains.m == seeds.size >= 2 and np.array_equal(host(on.dori_domains.labels), reg)
    for name, want in (('count', d.count), ('volume', d.volume), ('kind', d.kind), ('value', d.value), ('atoms', d.atoms)):
        assert np.array_equal(getattr(on, 'dori_domain_' + name), want), name
        assert getattr(on, 'dori_domain_' + name) is getattr(on.dori_domains, name)
    count, top, _ = per_component(reg, seeds.size, rho)
    assert np.array_equal(on.dori_domain_count, count) and np.array_equal(on.dori_domains.top, top)
    w = np.array([np.sum(rho.reshape(-1)[reg.reshape(-1) == i]) for i in range(seeds.size)]) * vv
    assert np.allclose(on.dori_domain_charge, w, rtol=1e-12, atol=0) and np.allclose(d.charge, w, rtol=1e-12, atol=0)
    from pybader_amd.critical import positions
    assert np.array_equal(on.dori_domain_position, positions(top, shape, lat) + on.voxel_offset)
    # each flag alone
    lean = make(dori_flag=True, **cuts)
    assert set(vars(lean)) & (DORI_ATTRIBUTES | DOMAIN_ATTRIBUTES) == DORI_ATTRIBUTES - {'critical_dori', 'atoms_bond_dori'}
    assert np.array_equal(lean.atoms_dori_count, on.atoms_dori_count)
    alone = make(dori_domains_flag=True, **cuts)
    assert 'atoms_dori_count' not in vars(alone) and np.array_equal(alone.dori_domain_count, on.dori_domain_count)

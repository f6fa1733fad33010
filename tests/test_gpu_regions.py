"""Connected regions on the GPU against the restatement of tests/test_regions_cpu.py.  Every integer output -- the map, the number
of components, seeds, counts, tops, shares, atoms, kinds -- is compared with == through BOTH routes (tiles and
XB_DOMAINS_GLOBAL), and the routes with each other; the float sums lie under the project's bound
|got - fsum(terms) vv| <= (count + 2) 2^-53 fsum(|terms|) |vv|."""
import ctypes as C
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

import history_common as H
import test_gpu_all_flags as AF
import test_nci_cpu as tn
import test_regions_cpu as R
from pybader_amd import _lib, critical, device, nci, regions, thread_handlers, utils
from test_gpu_history import Runner
from test_multipole_cpu import VV, bound, label_map
from test_regions_cpu import check_sums
from test_regions_cpu import test_the_bound_notices_a_voxel_in_the_wrong_component  # noqa: F401 -- runs here too

pytestmark = pytest.mark.gpu
ABOVE, BELOW, NCI = _lib.XB_DOMAINS_ABOVE, _lib.XB_DOMAINS_BELOW, _lib.XB_DOMAINS_NCI


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def have_torch():
    return torch is not None and torch.cuda.is_available()


def host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


def upload(ctx, rho):
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    if ctx.shape != rho.shape:
        ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)


def both_routes(ctx, what, mode, reg, seeds, rho, level=0.5, **kw):
    """label through both routes: m, the map and the sums equal the restatement (and so each other)"""
    for route in (False, True):
        m = ctx.regions_label(mode, None, level, global_route=route, **kw)
        assert m == seeds.size, f'{what}, global {route}: {m} components, {seeds.size} restated'
        got = ctx.regions_map()
        assert got.dtype == np.int32 and np.array_equal(got, reg), f'{what}, global {route}: {int((got != reg).sum())} voxels differ'
        check_sums(f'{what}, global {route}', ctx.regions_sums(m, VV), reg, seeds, rho)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(R.hand_masks())))
def test_hand_made_masks_through_both_routes_and_inverted(ctx, i):
    name, mask, want = R.hand_masks()[i]
    reg, seeds = R.hand_reference(i)
    assert seeds.size == want
    field = mask.astype(np.float64)
    upload(ctx, field)
    both_routes(ctx, name, ABOVE, reg, seeds, field)
    if want == 0:
        assert ctx.regions_map().min() == -1 and all(a.shape[0] == 0 for a in ctx.regions_sums(0, VV))
    if want == 1 and mask.all():
        assert ctx.regions_sums(1, VV)[0].tolist() == [0]
    inverted = 1.0 - field
    upload(ctx, inverted)
    both_routes(ctx, name + ', inverted', BELOW, reg, seeds, inverted)


@pytest.mark.parametrize('density', [0.1, 0.3, 0.6])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_random_masks_through_both_routes_and_inverted(ctx, shape, density):
    mask = R.random_mask(shape, density)
    reg, seeds = R.components(mask)
    rng = np.random.default_rng(5)
    field = np.where(mask, 1.0 + rng.random(shape), rng.random(shape) * 0.25)      # (distinct values: every top is decided by a key)
    upload(ctx, field)
    both_routes(ctx, f'{shape} at {density}', ABOVE, reg, seeds, field, level=0.5)
    upload(ctx, -field)
    both_routes(ctx, f'{shape} at {density}, inverted', BELOW, reg, seeds, -field, level=-0.5)


def test_nan_is_outside_in_every_mode(ctx):
    shape = (13, 17, 19)
    rho = np.array(tn.density('rough', shape, 'cubic'))
    rho.reshape(-1)[::5] = np.nan
    upload(ctx, rho)
    level = 0.05
    with np.errstate(invalid='ignore'):
        for mode, mask in ((ABOVE, rho >= level), (BELOW, rho < level)):
            reg, seeds = R.components(mask)
            for route in (False, True):
                assert ctx.regions_label(mode, None, level, global_route=route) == seeds.size
                assert np.array_equal(ctx.regions_map(), reg)
    for route in (False, True):
        ctx.regions_label(NCI, None, 0.0, tn.LATS['cubic'], 1.5, 1.0, global_route=route)
        assert (ctx.regions_map().reshape(-1)[::5] == -1).all()


def test_a_field_that_is_not_the_density(ctx):
    """the members come from the field, top and the sums from the resident density"""
    shape = (20, 9, 33)
    rho = tn.density('rough', shape, 'cubic')
    mask = R.random_mask(shape, 0.3)
    reg, seeds = R.components(mask)
    upload(ctx, rho)
    fdev = ctx.device_copy(mask.astype(np.float64))
    for route in (False, True):
        m = ctx.regions_label(ABOVE, fdev, 0.5, global_route=route)
        assert m == seeds.size and np.array_equal(ctx.regions_map(), reg)
        check_sums(f'field, global {route}', ctx.regions_sums(m, VV), reg, seeds, rho)
        dmap = ctx.regions_map(on_device=True)
        assert isinstance(dmap, device.DeviceArray) and np.array_equal(dmap.to_host(), reg)
    assert np.array_equal(ctx.download_density(), rho)


# ---- the python layer, host arrays and device tensors -------------------------------------------------------------------------------
def check_regions(what, r, mask, rho, vv, labels=None, n=0):
    reg, seeds = R.components(mask)
    assert r.m == len(r) == seeds.size and np.array_equal(host(r.labels), reg), what
    check_sums(what, (r.seed, r.count, r.top, r.charge, r.charge2), reg, seeds, rho, vv)
    assert np.array_equal(r.voxel, np.stack(np.unravel_index(seeds, mask.shape), axis=1)) and np.array_equal(r.volume, r.count * vv)
    want = R.shares(reg, labels, n) if n else (np.zeros(0, np.int32),) * 2 + (np.zeros(0, np.int64),)
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(r.shares, want)), f'{what}: shares'
    assert np.array_equal(r.atoms, R.atoms_of(seeds.size, want)), f'{what}: atoms'
    return reg, seeds


def test_connected_regions_of_host_arrays_and_device_tensors():
    shape = (20, 9, 33)
    rho = tn.density('rough', shape, 'cubic')
    level = R.sum_level(rho)
    n = 5
    lab = label_map(shape, n)
    for route in (False, True):
        r = regions.connected_regions(rho, level, voxel_volume=VV, volumes=lab, n=n, global_route=route)
        assert isinstance(r.labels, np.ndarray)
        check_regions(f'host, global {route}', r, rho >= level, rho, VV, lab, n)
        r = regions.connected_regions(rho, level, below=True, voxel_volume=VV, global_route=route)
        check_regions(f'host below, global {route}', r, rho < level, rho, VV)
    mask = R.random_mask(shape, 0.3)
    with utils.resident(rho):
        r = regions.connected_regions(mask.astype(np.float64), 0.5, density=rho, voxel_volume=VV, volumes=lab.astype(np.int8), n=n)
        check_regions('a mask on the resident density', r, mask, rho, VV, lab, n)
    with pytest.raises(ValueError):
        regions.connected_regions(np.zeros((3, 3, 3)), 0.5, density=rho)
    regions.connected_regions(rho, level)
    held = _lib.default_context().memory_stats()
    with pytest.raises(ValueError):
        regions.connected_regions(rho, level, volumes=np.zeros((3, 3, 3), np.int32), n=2)
    with pytest.raises(ValueError):
        nci.nci_domains(rho, tn.LATS['cubic'], np.zeros((3, 3, 3), np.int32), 2)
    assert _lib.default_context().memory_stats() == held, 'a call that fails after the labelling leaves no map behind'
    if not have_torch():
        pytest.skip('the host arrays passed; torch with a GPU is needed for a device tensor')
    rho32 = rho.astype(np.float32)
    perm = torch.as_tensor(np.ascontiguousarray(rho.transpose(2, 0, 1)), device='cuda').permute(1, 2, 0)
    assert tuple(perm.shape) == shape and not perm.is_contiguous()
    for what, t, ref in (('float32 tensor', torch.as_tensor(rho32.copy(), device='cuda'), rho32.astype(np.float64)),
                         ('permuted float64 tensor', perm, rho)):
        for route in (False, True):
            r = regions.connected_regions(t, level, voxel_volume=VV, volumes=torch.as_tensor(lab.copy(), device='cuda'), n=n, global_route=route)
            assert isinstance(r.labels, device.DeviceArray)
            check_regions(f'{what}, global {route}', r, ref >= level, ref, VV, lab, n)
            back = torch.as_tensor(r.labels, device='cuda')
            assert back.dtype == torch.int32 and tuple(back.shape) == shape


# ---- cross-checks against independent kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['synth', 'rough'])
@pytest.mark.parametrize('shape', [(13, 17, 19), (20, 9, 33), (24, 16, 96)])
def test_tops_are_maxima_and_maxima_above_the_level_are_inside(shape, kind):
    rho = tn.density(kind, shape, 'cubic')
    level = R.sum_level(rho)
    cp = critical.critical_points(rho)
    maxima = cp.lin[cp.masks == _lib.XB_CRITICAL_FULL]
    assert maxima.size >= 8
    for route in (False, True):
        r = regions.connected_regions(rho, level, global_route=route)
        assert r.m >= 2 and np.isin(r.top, maxima).all(), 'every top is a listed maximum'
        inside = maxima[rho.reshape(-1)[maxima] >= level]
        assert inside.size and (r.labels.reshape(-1)[inside] >= 0).all(), 'every maximum above the level lies in a component'
        assert np.array_equal(np.unique(r.labels.reshape(-1)[inside]), np.arange(r.m)), 'every component holds a maximum'


def test_shares_sum_to_the_counts_and_both_routes_give_the_same_triplets(ctx):
    shape = (20, 9, 33)
    rho = tn.density('rough', shape, 'cubic')
    level = R.sum_level(rho)
    reg, seeds = R.components(rho >= level)
    upload(ctx, rho)
    m = ctx.regions_label(ABOVE, None, level)
    count = ctx.regions_sums(m, VV)[1]
    for n, lab in ((4, label_map(shape, 4) % 4), (3000, np.arange(rho.size, dtype=np.int32).reshape(shape) % 3000)):
        assert lab.min() >= 0 and lab.max() < n
        ctx.upload_labels(lab)
        dense, listed = ctx.regions_shares(n), ctx.regions_shares(n, force_list=True)
        want = R.shares(reg, lab, n)
        for got in (dense, listed):
            assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
        assert np.array_equal(np.bincount(dense[0], weights=dense[2], minlength=m).astype(np.int64), count)
    lab = label_map(shape, 7)          # labels -1, n, n + 7 and INT32_MAX among them: skipped
    assert lab.min() < 0 and lab.max() >= 7
    ctx.upload_labels(lab)
    dense, listed = ctx.regions_shares(7), ctx.regions_shares(7, force_list=True)
    want = R.shares(reg, lab, 7)
    for got in (dense, listed):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    labelled = (reg >= 0) & (lab >= 0) & (lab < 7)
    assert np.array_equal(np.bincount(dense[0], weights=dense[2], minlength=m).astype(np.int64), np.bincount(reg[labelled], minlength=m))
    assert dense[2].sum() < count.sum()
    assert np.array_equal(ctx.download_labels(np.int32), lab) and np.array_equal(ctx.download_density(), rho), 'nothing resident is written'


# ---- NCI domains ------------------------------------------------------------------------------------------------------------------
def nci_reference(kind, shape, lname, cuts):
    v = tn.values(kind, shape, lname)
    mask = tn.region(v, cuts[0], cuts[1])
    reg, seeds = R.components(mask)
    cls = np.where(mask, tn.classes(v, cuts[2]), -1)
    return v, mask, reg, seeds, cls


def check_classes(what, d, reg, cls, rho, m, vv):
    """count, charge and charge2 per class: counts with ==, the sums under the bound of their own class"""
    rho = np.asarray(rho, dtype=np.float64)
    for k in range(3):
        part = np.where(cls == k, reg, -1)
        cnt = np.bincount(part[part >= 0], minlength=m)
        assert np.array_equal(d.count[:, k], cnt), f'{what}: class {k} counts'
        flat, pk = rho.reshape(-1), part.reshape(-1)
        for name, g, t in (('rho', d.charge[:, k], flat), ('rho^2', d.charge2[:, k], flat * flat)):
            terms = [t[pk == i] for i in range(m)]
            w, mag = R.sums(terms)
            lim = bound(cnt, mag[:, None], vv)[:, 0]
            assert np.all(np.abs(g - w * vv) <= lim), f'{what}: class {k} sum of {name}'
            assert not g[cnt == 0].any()


def check_domains(what, d, kind, shape, lname, cuts, vv, lab=None, n=0):
    v, mask, reg, seeds, cls = nci_reference(kind, shape, lname, cuts)
    rho = tn.density(kind, shape, lname)
    m = seeds.size
    assert d.m == m and np.array_equal(host(d.labels), reg), f'{what}: the map'
    check_sums(what, (d.seed, d.size, d.top, d.total, d.total2), reg, seeds, rho, vv)
    assert d.count.shape == d.charge.shape == d.charge2.shape == (m, 3) and np.array_equal(d.count.sum(1), d.size)
    check_classes(what, d, reg, cls, rho, m, vv)
    assert np.array_equal(d.kind, cls.reshape(-1)[d.top]) and d.kind.dtype == np.int8 and (d.kind >= 0).all(), f'{what}: kind'
    want = R.shares(reg, lab, n) if n else (np.zeros(0, np.int32),) * 2 + (np.zeros(0, np.int64),)
    assert all(np.array_equal(g, w) for g, w in zip(d.shares, want)), f'{what}: shares'
    assert np.array_equal(d.atoms, R.atoms_of(m, want)), f'{what}: atoms'
    return cls


@pytest.mark.parametrize('lname', list(tn.LATS))
@pytest.mark.parametrize('shape', [(13, 17, 19), (20, 9, 33)])
def test_nci_domains_equal_the_restatement_through_every_route(shape, lname):
    n = 6
    lab = label_map(shape, n)
    rho = tn.density('holes', shape, lname)
    for gather in (False, True):
        for route in (False, True):
            d = nci.nci_domains(rho, tn.LATS[lname], lab, n, VV, *tn.SUM_CUTS, gather=gather, global_route=route, shares_list=gather)
            check_domains(f'{shape} {lname}, gather {gather}, global {route}', d, 'holes', shape, lname, tn.SUM_CUTS, VV, lab, n)
    assert d.m >= 4


def test_nci_domain_counts_sum_to_the_region_sums():
    shape, lname, n = (20, 9, 33), 'tric', 4
    rho = tn.density('holes', shape, lname)
    lab = label_map(shape, n) % n
    for gather in (False, True):
        d = nci.nci_domains(rho, tn.LATS[lname], lab, n, VV, *tn.SUM_CUTS, gather=gather)
        r = nci.nci_regions(rho, lab, tn.LATS[lname], n, VV, *tn.SUM_CUTS, gather=gather)
        assert np.array_equal(d.count.sum(0), r.count.sum(0)) and d.count.sum() > 100
        assert np.array_equal(np.bincount(d.shares[0], weights=d.shares[2], minlength=d.m).astype(np.int64), d.size)


# ---- state and errors -----------------------------------------------------------------------------------------------------------------
def test_state_errors_and_memory():
    c = _lib.Context(0)
    try:
        shape = (13, 17, 19)
        rho = tn.density('rough', shape, 'cubic')
        lat = tn.LATS['cubic']
        calls = (lambda: c.regions_label(ABOVE, None, 0.1), lambda: c.regions_label(NCI, None, 0.0, lat, 0.5, 0.05))
        for call in calls:
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        for call in calls + (lambda: c.regions_sums(0, VV), lambda: c.regions_map(), lambda: c.regions_shares(2)):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE                  # no density; no result
        c.upload_density(rho)
        before = c.memory_stats()
        level = R.sum_level(rho)
        m = c.regions_label(ABOVE, None, level)
        assert m >= 2
        after = c.memory_stats()
        assert after[2] - before[2] == 4 * rho.size + 4 * m and after[0] - before[0] == after[2] - before[2]
        with pytest.raises(_lib.BaderHipError) as e:
            c.regions_shares(2)
        assert e.value.code == _lib.XB_E_STATE                      # no labels
        with pytest.raises(_lib.BaderHipError) as e:
            c.regions_sums(m - 1, VV)
        assert e.value.code == _lib.XB_E_ARG                        # a capacity below the length
        with pytest.raises(_lib.BaderHipError) as e:
            c.regions_sums(m, VV, 0.01)
        assert e.value.code == _lib.XB_E_STATE                      # classes of components that are not the NCI region's
        c.upload_labels(np.zeros(shape, np.int32))
        lib, h, arg = c.lib, c.h, _lib.XB_E_ARG
        mm = C.c_int64(-7)
        lp = (C.c_double * 9)(*lat.reshape(-1))
        flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)          # a singular lattice
        assert lib.xb_regions_label(h, 3, None, 0.1, None, 0.0, 0.0, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, -1, None, 0.1, None, 0.0, 0.0, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, ABOVE, None, 0.1, None, 0.0, 0.0, 16, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, ABOVE, None, 0.1, None, 0.0, 0.0, _lib.XB_DOMAINS_GATHER, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, ABOVE, None, 0.1, None, 0.0, 0.0, 0, None) == arg
        assert lib.xb_regions_label(h, ABOVE, None, float('nan'), None, 0.0, 0.0, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, NCI, None, 0.0, None, 0.5, 0.05, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, NCI, None, 0.0, flat, 0.5, 0.05, 0, C.byref(mm)) == arg
        for cuts in ((-0.5, 0.05), (0.5, float('nan')), (float('inf'), 0.05)):
            assert lib.xb_regions_label(h, NCI, None, 0.0, lp, *cuts, 0, C.byref(mm)) == arg
        fdev = c.device_copy(np.ascontiguousarray(rho))
        assert lib.xb_regions_label(h, NCI, C.c_void_p(fdev.ptr), 0.0, lp, 0.5, 0.05, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, ABOVE, C.c_void_p(fdev.ptr + 8), 0.1, None, 0.0, 0.0, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, ABOVE, C.c_void_p(fdev.ptr + 4), 0.1, None, 0.0, 0.0, 0, C.byref(mm)) == arg
        assert lib.xb_regions_label(h, ABOVE, C.c_void_p(rho.ctypes.data), 0.1, None, 0.0, 0.0, 0, C.byref(mm)) == arg
        assert mm.value == -7
        # the refused calls left the result where it was
        assert np.array_equal(c.regions_map(), R.components(rho >= level)[0])
        nt = C.c_int64(-7)
        assert lib.xb_regions_shares(h, 0, 0, C.byref(nt)) == arg and lib.xb_regions_shares(h, 2, 4, C.byref(nt)) == arg
        assert lib.xb_regions_shares(h, 2, 0, None) == arg and nt.value == -7
        assert lib.xb_regions_shares_fetch(h, None, None, None, 0) == _lib.XB_E_STATE      # (no triplets yet)
        comp, lab, cnt = c.regions_shares(1)
        assert comp.tolist() == list(range(m)) and not lab.any() and np.array_equal(cnt, c.regions_sums(m, VV)[1])
        small = np.zeros(1, np.int32)
        assert lib.xb_regions_shares_fetch(h, small.ctypes.data, small.ctypes.data, np.zeros(1, np.int64).ctypes.data_as(C.POINTER(C.c_int64)),
                                           m - 1) == arg
        assert lib.xb_regions_fetch_map(h, 0, None) == arg
        assert lib.xb_regions_fetch_map(h, 1, C.c_void_p(rho.ctypes.data)) == arg
        # the density and the labels are what they were
        assert np.array_equal(c.download_density(), rho) and not c.download_labels(np.int32).any()
        # the stages' times: only of a labelling that asked for them
        with pytest.raises(_lib.BaderHipError) as e:
            c.regions_times()
        assert e.value.code == _lib.XB_E_STATE
        for route in (False, True):
            assert c.regions_label(ABOVE, None, level, global_route=route, times=True) == m
            ms = c.regions_times()
            assert ms.shape == (4,) and (ms >= 0).all() and ms.sum() > 0 and ms.sum() < 1000
            assert np.array_equal(c.regions_map(), R.components(rho >= level)[0]) and c.memory_stats() == after
        assert lib.xb_regions_times(h, None) == arg
        # release gives the memory back; a second labelling takes the same again
        c.regions_release()
        assert c.memory_stats() == before
        with pytest.raises(_lib.BaderHipError) as e:
            c.regions_map()
        assert e.value.code == _lib.XB_E_STATE
        assert c.regions_label(ABOVE, None, level, global_route=True) == m and c.memory_stats() == after
        # a writer of the density discards the result
        c.upload_density(rho)
        for call in (lambda: c.regions_map(), lambda: c.regions_sums(m, VV), lambda: c.regions_shares(1)):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE
        # a slab is refused; the whole grid works again
        c.set_grid(shape, np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(rho)
        for call in calls:
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        assert c.regions_label(ABOVE, None, level) == m
    finally:
        c.close()


# ---- call history -------------------------------------------------------------------------------------------------------------------
HISTORY_CUTS = (1.0, 1.0, 0.03)


@functools.lru_cache(maxsize=None)
def history_reference(kind, grid):
    rho = H.density(grid, 'A')
    if kind == 'regions':
        level = R.sum_level(rho)
        return (level,) + R.components(rho >= level)
    v = tn.restated(rho, H.LAT)
    mask = tn.region(v, *HISTORY_CUTS[:2])
    return (np.where(mask, tn.classes(v, HISTORY_CUTS[2]), -1),) + R.components(mask)


def regions_call(kind, grid, run=None):
    """connected_regions or nci_domains through the public functions on density A and the atom map of a grid of history_common
    (host arrays, or the Runner's device tensors) -> None, or what differs from the restatement"""
    rho, lab, n = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms')
    arg_rho, arg_lab = (rho, lab) if run is None else (run.rho(grid, 'A32'), run.lab(grid, 'atoms'))
    ref = rho if run is None else H.density(grid, 'A32')
    if kind == 'regions':
        level, reg, seeds = history_reference(kind, grid)
        if run is not None:
            reg, seeds = R.components(ref >= level)
        r = regions.connected_regions(arg_rho, level, voxel_volume=VV, volumes=arg_lab, n=n)
        got = (r.seed, r.count, r.top, r.charge, r.charge2)
    else:
        cls, reg, seeds = history_reference(kind, grid)
        if run is not None:
            v = tn.restated(ref, H.LAT)
            reg, seeds = R.components(tn.region(v, *HISTORY_CUTS[:2]))
        r = nci.nci_domains(arg_rho, H.LAT, arg_lab, n, VV, *HISTORY_CUTS)
        got = (r.seed, r.size, r.top, r.total, r.total2)
    if r.m != seeds.size or seeds.size < 2 or not np.array_equal(host(r.labels), reg):
        return f'{kind} on {grid}: the map differs'
    try:
        check_sums(f'{kind} on {grid}', got, reg, seeds, ref)
    except AssertionError as e:
        return str(e)
    want = R.shares(reg, lab, n)
    if not all(np.array_equal(g, w) for g, w in zip(r.shares, want)) or want[2].sum() < 50:
        return f'{kind} on {grid}: the shares differ'
    return None


@pytest.mark.parametrize('other', ['basin_laplacian', 'critical', 'voronoi', 'nci_regions'])
@pytest.mark.parametrize('kind', ['regions', 'domains'])
def test_call_history_does_not_matter(kind, other, monkeypatch):
    """each call directly before and directly after another analysis (voronoi rewrites the device labels), on G1 -> G2 -> G1 of
    history_common.GRIDS, on the default context, inside and outside utils.resident(): both sides' results are unchanged"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    run = Runner()

    def neighbour(grid):
        if other != 'nci_regions':
            return run.checked(other, grid, 'A', 'atoms')
        rho, lab, n = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms')
        r = nci.nci_regions(rho, lab, H.LAT, n, VV, *HISTORY_CUTS)
        cnt = tn.sum_reference(tn.restated(rho, H.LAT), lab, n, HISTORY_CUTS)[0][1]
        return None if np.array_equal(r.count.reshape(-1), cnt) else f'nci_regions on {grid}: counts differ'

    bad = []
    try:
        for grid in ('G1', 'G2', 'G1'):
            for step in (lambda: regions_call(kind, grid), lambda: neighbour(grid), lambda: regions_call(kind, grid), lambda: neighbour(grid)):
                msg = step()
                if msg:
                    bad.append(f'{grid}: {msg}')
        with utils.resident(H.density('G1', 'A')):
            for step in (lambda: neighbour('G1'), lambda: regions_call(kind, 'G1'), lambda: neighbour('G1'), lambda: regions_call(kind, 'G1')):
                msg = step()
                if msg:
                    bad.append(f'resident(A): {msg}')
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, ' | '.join(bad[:4])


@pytest.mark.parametrize('kind', ['regions', 'domains'])
def test_call_history_with_device_tensors(kind, monkeypatch):
    if not have_torch():
        pytest.skip('torch sees no device')
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    run = Runner(dev=True)
    bad = []
    try:
        for grid in ('G1', 'G2', 'G1'):
            for step in (lambda: regions_call(kind, grid, run), lambda: run.checked('critical', grid, 'A32', 'atoms'),
                         lambda: regions_call(kind, grid, run), lambda: run.checked('basin_laplacian', grid, 'A32', 'atoms'),
                         lambda: regions_call(kind, grid, run)):
                msg = step()
                if msg:
                    bad.append(f'{grid}: {msg}')
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, ' | '.join(bad[:4])


def around(kind, other, run, setting, names, pinned=None):
    """the new call, then `other` of history_common.KINDS on `names` = (density name, map name) of G1, twice in turn: the new call
    runs directly before and directly after the existing one (`other` gets the Bader map, the new call the atom map, so each also
    has to bring its own labels back).  -> the failures"""
    bad = []

    def body():
        for what, step in (('before', lambda: regions_call(kind, 'G1', run if run.dev else None)),
                           (other, lambda: run.checked(other, 'G1', *names)),
                           ('after', lambda: regions_call(kind, 'G1', run if run.dev else None)),
                           (other + ' again', lambda: run.checked(other, 'G1', *names))):
            msg = step()
            if msg:
                bad.append(f'[{setting}] {kind} around {other}, {what}: {msg}')
    if pinned is None:
        body()
    else:
        with utils.resident(pinned):
            body()
    return bad


@pytest.mark.parametrize('other', list(H.KINDS))
@pytest.mark.parametrize('kind', ['regions', 'domains'])
def test_every_existing_call_kind_before_and_after(kind, other, monkeypatch):
    """connected_regions / nci_domains directly before and directly after EVERY call kind of history_common.KINDS -- those that
    use the scratch buffer the labelling writes its ranks into (refine, bader_calc_refine, the weight method, merge, adjacency)
    and those that rewrite the device labels the shares read (volume_assign, the Voronoi kinds) among them -- in the settings of
    tests/test_gpu_history.py: 1 host arrays;  2 the same inside resident(A);  4 a float32 device tensor of A and int32 device
    tensors of the maps (expectations from A32);  4r the same inside resident(tensor).  Both sides' results are unchanged."""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    try:
        run = Runner()
        bad = around(kind, other, run, '1 plain', ('A', 'bader'))
        bad += around(kind, other, run, '2 resident(A)', ('A', 'bader'), pinned=H.density('G1', 'A'))
        if have_torch():
            dev = Runner(dev=True)
            bad += around(kind, other, dev, '4 device tensors', ('A32', 'bader'))
            bad += around(kind, other, dev, '4r resident(device tensor)', ('A32', 'bader'), pinned=dev.rho('G1', 'A32'))
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, f'{len(bad)} failures, the first: ' + ' | '.join(bad[:4])
    if not have_torch():
        pytest.skip('settings 1 and 2 passed; torch sees no device for setting 4')


# ---- Bader(nci_domains_flag=True) -----------------------------------------------------------------------------------------------------
DOMAIN_ATTRIBUTES = {'nci_domains_flag', 'nci_domains', 'nci_domain_count', 'nci_domain_volume', 'nci_domain_charge', 'nci_domain_kind',
                     'nci_domain_atoms', 'nci_domain_position'}
BADER_CUTS = {'nci_s_cut': 20.0, 'nci_rho_cut': 0.5, 'nci_rho_split': 0.002}      # (those of tests/test_gpu_nci.py)


@pytest.mark.parametrize('profile', ['default', 'reference and vacuum'])
def test_bader_with_the_flag(profile, monkeypatch):
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    off = AF.make(profile, nci_flag=True, critical_flag=True, **BADER_CUTS)
    off()
    assert off.nci_domains_flag is False and not (DOMAIN_ATTRIBUTES - {'nci_domains_flag'}) & set(dir(off))
    AF.verify(off, profile, 'nci_flag, the domains off')
    on = AF.make(profile, nci_flag=True, critical_flag=True, nci_domains_flag=True, **BADER_CUTS)
    on()
    AF.verify(on, profile, 'nci_flag and the domains')
    assert set(vars(on)) - set(vars(off)) == DOMAIN_ATTRIBUTES
    AF.same_exact_attributes(on, off, f'{profile}: the domains on against off', skip={'atoms_nci_charge'})
    assert on.atoms_nci_charge.shape == off.atoms_nci_charge.shape
    cuts = tuple(BADER_CUTS.values())
    d = nci.nci_domains(on.reference, AF.LAT, on.atoms_volumes, AF.N_ATOMS, on.voxel_volume, *cuts)
    o = on.nci_domains
    assert d.m == o.m >= 1 and np.array_equal(host(d.labels), host(o.labels))
    for name in ('seed', 'count', 'top', 'kind', 'atoms', 'size'):
        assert np.array_equal(getattr(d, name), getattr(o, name)), name
    assert all(np.array_equal(a, b) for a, b in zip(d.shares, o.shares))
    assert np.array_equal(on.nci_domain_count, d.count) and np.array_equal(on.nci_domain_volume, d.count * on.voxel_volume)
    assert np.array_equal(on.nci_domain_kind, d.kind) and np.array_equal(on.nci_domain_atoms, d.atoms)
    assert np.array_equal(on.nci_domain_position, critical.positions(d.top, d.shape, AF.LAT) + on.voxel_offset)
    # against the restatement on the reference density and the run's own atoms_volumes
    ref = AF.fields_of(profile)[0]
    v = tn.restated(ref, AF.LAT)
    mask = tn.region(v, cuts[0], cuts[1])
    reg, seeds = R.components(mask)
    lab = np.asarray(AF.host(on.atoms_volumes))
    assert np.array_equal(host(o.labels), reg) and np.array_equal(o.seed, seeds)
    cls = np.where(mask, tn.classes(v, cuts[2]), -1)
    check_classes(profile, o, reg, cls, ref, seeds.size, on.voxel_volume)
    want = R.shares(reg, lab, AF.N_ATOMS)
    assert np.array_equal(on.nci_domain_atoms, R.atoms_of(seeds.size, want))
    count, _, terms = R.per_component(reg, seeds.size, ref)
    w, mag = R.sums(terms)
    lim = bound(count, mag[:, None], on.voxel_volume)[:, 0]
    assert np.all(np.abs(o.total - w * on.voxel_volume) <= lim) and on.nci_domain_charge is o.charge

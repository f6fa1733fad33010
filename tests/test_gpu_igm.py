"""xb_igm_field / xb_igm_sum and what stands on them (-m gpu) against the numpy restatement of tests/test_igm_cpu.py.

delta-g and delta-g_inter, the counts of the region, the domains and the surface's connectivity are compared with == : every
operation that decides them is bit-defined (include/bader_hip.h; double sqrt and / are correctly rounded).  The forced full
search (XB_HIRSHFELD_FULL_SEARCH) is the second implementation: everything runs through the candidate lists and through it.  THE
BOUND of the sums, per key 3 a + class, for the sum of rho and the sum of the field alike (tests/test_laplacian_cpu.py's
sum_bound):

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|"""
import ctypes as C
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

import history_common as H
import test_hirshfeld_cpu as HS
import test_mbis_cpu as MB
from pybader_amd import _lib, device, igm, isosurface, nci, synth, thread_handlers, utils
from pybader_amd.hirshfeld import ProAtoms
from pybader_amd.interface import Bader
from pybader_amd.isa import IsaResult
from test_gpu_history import Runner
from test_igm_cpu import (MODES, P_MIN, bits, check_sums, fragments, keys_of, reference, regions_difference, restate, sum_reference,
                          sums, table_sums)
from test_laplacian_cpu import grouped, sum_bound
from test_multipole_cpu import VV, label_map
from test_regions_cpu import components, per_component

pytestmark = pytest.mark.gpu
FIELD_CASES = ['three', 'thin', 'odd_k1', 'partial', 'tric_r2', 'small_cell', 'twins', 'many_overflow', 'many_mixed']
# (F, atoms of no fragment): F = 2 and 4 are the instantiations, 1 and 3 are mapped up to them
SPLITS = [(2, False), (4, True), (4, False), (2, True)]
SUM_CASE = 'cubic_r3'


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
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.size == want.size, what
    diff = bits(got).reshape(-1) != bits(want).reshape(-1)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ from the restatement, first at {int(np.flatnonzero(diff)[0])}'


def load(ctx, c):
    """the grid, the density and the Hirshfeld setup of one input of tests/test_hirshfeld_cpu.py"""
    ctx.set_grid(c.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(c.rho)
    ctx.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)


def check_route(c, stats, full_search, what):
    if full_search:
        assert stats['candidate_tiles'] == 0 and stats['full_tiles'] > 0 and stats['max_candidates'] == 0, what
    elif c.route == 'candidate':
        assert stats['full_tiles'] == 0 and 0 < stats['max_candidates'] <= _lib.XB_HIRSHFELD_CAND_MAX, what
    elif c.route == 'overflow':
        assert stats['candidate_tiles'] == 0 and stats['max_candidates'] > _lib.XB_HIRSHFELD_CAND_MAX, what
    else:
        assert stats['candidate_tiles'] > 0 and stats['full_tiles'] > 0, what


# ---- the fields -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', FIELD_CASES)
def test_fields_equal_the_restatement_through_both_routes(ctx, name, mode):
    c = HS.case(name)
    load(ctx, c)
    n = c.atoms.shape[0]
    for F, loose in SPLITS:
        v = reference(name, F, loose, mode)
        fr = fragments(n, F, loose)
        for full_search in (False, True):
            what = f'{name}, {mode}, F = {F}, loose {loose}, full search {full_search}'
            dg, dgi, stats = ctx.igm_field(c.lattice, fr, MODES[mode], P_MIN, full_search, n_fragments=F)
            same_bits(dg, v['dg'], what + ': dg')
            same_bits(dgi, v['dgi'], what + ': dgi')
            check_route(c, stats, full_search, what)
    if name == 'tric_r2':
        assert not v['reached'].all() and v['reached'].any(), 'this input has voxels no table reaches'
        assert (dg.reshape(-1)[~v['reached']] == 0).all() and not np.signbit(dg.reshape(-1)[~v['reached']]).any()
    assert np.array_equal(ctx.download_density(), c.rho), 'nothing resident is written'


@pytest.mark.parametrize('mode', list(MODES))
def test_one_and_three_fragments_are_mapped_up_and_every_output_side_agrees(ctx, mode):
    name = 'odd_k1'
    c = HS.case(name)
    load(ctx, c)
    for F, loose in ((1, False), (3, True), (1, True), (3, False)):
        fr = fragments(8, F, loose)
        v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode], sums=sums(name))
        if F == 1:
            assert (v['dgi'] == 0).all()
        for full_search in (False, True):
            what = f'{mode}, F = {F}, loose {loose}, full search {full_search}'
            dg, dgi, _ = ctx.igm_field(c.lattice, fr, MODES[mode], P_MIN, full_search, n_fragments=F)
            same_bits(dg, v['dg'], what + ': dg')
            same_bits(dgi, v['dgi'], what + ': dgi')
        # device outputs, and each field alone on either side
        dg, dgi, _ = ctx.igm_field(c.lattice, fr, MODES[mode], P_MIN, on_device=True, n_fragments=F)
        assert isinstance(dg, device.DeviceArray) and dg.shape == c.shape and dg.dtype == np.float64
        same_bits(dg.to_host(), v['dg'], 'device dg')
        same_bits(dgi.to_host(), v['dgi'], 'device dgi')
        for on_device in (False, True):
            a, b, _ = ctx.igm_field(c.lattice, fr, MODES[mode], P_MIN, on_device=on_device, want=(True, False), n_fragments=F)
            assert b is None
            same_bits(host(a), v['dg'], f'dg alone, device {on_device}')
            a, b, _ = ctx.igm_field(c.lattice, fr, MODES[mode], P_MIN, on_device=on_device, want=(False, True), n_fragments=F)
            assert a is None
            same_bits(host(b), v['dgi'], f'dgi alone, device {on_device}')
    # one field to the host and the other to the device in one call
    fr = fragments(8, 2)
    v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode], sums=sums(name))
    out_h, out_d = np.empty(c.shape), device.DeviceArray(ctx, c.shape, np.float64)
    lat = np.ascontiguousarray(c.lattice, dtype=np.float64).reshape(9)
    st = (C.c_int64 * 3)()
    rc = ctx.lib.xb_igm_field(ctx.h, lat.ctypes.data_as(C.POINTER(C.c_double)), fr.ctypes.data_as(C.c_void_p), 2, MODES[mode], P_MIN, 0,
                              out_h.ctypes.data_as(C.c_void_p), None, None, C.c_void_p(out_d.ptr), st)
    assert rc == 0
    same_bits(out_h, v['dg'], 'dg to the host beside dgi to the device')
    same_bits(out_d.to_host(), v['dgi'], 'dgi to the device beside dg to the host')


def test_an_isa_setup(ctx):
    """the tables of an ISA setup are piecewise constant: their pairs are (A[k], +0.0), so G = 0.  Mode 'pro' gives exact zeros;
    mode 'stockholder' gives ga = w_a grad rho, all parallel, so nothing cancels and both fields are zero up to the rounding of the
    sums (a few u |grad rho|).  The kernels are held to the restatement's bits all the same"""
    c = HS.case('tric_r2')
    n, K = 8, 12
    rng = np.random.default_rng(5)
    tables = rng.random((n, K)) + 0.05
    r_cut = np.linspace(1.6, 2.4, n)
    bound = float(np.abs(c.rho).max())
    pro = ProAtoms(np.concatenate([tables, np.zeros((n, 1))], axis=1), r_cut)
    sp = np.arange(n, dtype=np.int32)
    t = table_sums(c.shape, c.lattice, c.atoms, sp, pro, flat=True)
    ctx.set_grid(c.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(c.rho)
    ctx.isa_setup(c.lattice, c.atoms, r_cut, K, bound, tables)
    for mode in MODES:
        for F, loose in ((2, False), (4, True)):
            fr = fragments(n, F, loose)
            v = restate(c.shape, c.lattice, c.atoms, sp, pro, c.rho, fr, MODES[mode], flat=True, sums=t)
            for full_search in (False, True):
                dg, dgi, _ = ctx.igm_field(c.lattice, fr, MODES[mode], P_MIN, full_search, n_fragments=F)
                same_bits(dg, v['dg'], f'ISA, {mode}, F = {F}, full search {full_search}: dg')
                same_bits(dgi, v['dgi'], f'ISA, {mode}, F = {F}, full search {full_search}: dgi')
            if mode == 'pro':
                assert (v['dg'] == 0).all() and (v['dgi'] == 0).all()
            else:
                assert max(np.abs(v['dg']).max(), np.abs(v['dgi']).max()) <= 64 * 2.0 ** -53 * np.abs(v['gr']).max()
                assert v['reached'].any() and np.abs(v['g']).max() > 0
    # through the public function, which loads the tables as isa_promolecule does
    res = IsaResult(r_cut=r_cut, shells=K, rho_bound=bound, tables=tables)
    fr = fragments(n, 2)
    v = restate(c.shape, c.lattice, c.atoms, sp, pro, c.rho, fr, MODES['stockholder'], flat=True, sums=t)
    dg, dgi, x = igm.igm_fields(c.rho, c.lattice, c.atoms, fr, isa=res, colour=False)
    assert x is None and isinstance(dg, np.ndarray)
    same_bits(dg, v['dg'], 'igm_fields on an IsaResult: dg')
    same_bits(dgi, v['dgi'], 'igm_fields on an IsaResult: dgi')


def test_p_min_equal_to_a_voxels_P_pins_the_greater_than(ctx):
    name = 'tric_r2'
    c = HS.case(name)
    P = sums(name)['P']
    inside = np.sort(P[P > 0])
    p_min = float(inside[inside.size // 3])
    at = np.flatnonzero(P == p_min)
    fr = fragments(8, 2)
    load(ctx, c)
    for mode in MODES:
        v = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, c.rho, fr, MODES[mode], p_min, sums=sums(name))
        open_ = reference(name, 2, False, mode, 0.0)
        assert at.size and not v['reached'][at].any() and open_['reached'][at].all() and (open_['dg'][at] != 0).all()
        for full_search in (False, True):
            dg, dgi, _ = ctx.igm_field(c.lattice, fr, MODES[mode], p_min, full_search, n_fragments=2)
            same_bits(dg, v['dg'], f'{mode}, p_min on a voxel: dg')
            same_bits(dgi, v['dgi'], f'{mode}, p_min on a voxel: dgi')
            assert (dg.reshape(-1)[at] == 0).all() and (dgi.reshape(-1)[at] == 0).all()
        dg, _, _ = ctx.igm_field(c.lattice, fr, MODES[mode], 0.0, n_fragments=2)
        same_bits(dg, open_['dg'], f'{mode}, p_min = 0: dg')


def test_fields_of_device_densities_and_a_host_array_through_the_python_layer():
    name = 'twins'
    c = HS.case(name)
    fr = fragments(c.atoms.shape[0], 2, True)
    args = (c.lattice, c.atoms, fr, c.species, c.pro)
    v = reference(name, 2, True, 'stockholder')
    x_want = nci.nci_fields(c.rho, c.lattice)[1]
    dg, dgi, x = igm.igm_fields(c.rho, *args)
    assert all(isinstance(a, np.ndarray) and a.shape == c.shape for a in (dg, dgi, x))
    same_bits(dg, v['dg'], 'host array: dg')
    same_bits(dgi, v['dgi'], 'host array: dgi')
    same_bits(x, x_want, 'host array: x')
    w = reference(name, 2, True, 'pro')
    with utils.resident(c.rho):
        for full_search in (False, True):
            dg, dgi, x = igm.igm_fields(c.rho, *args, mode='pro', full_search=full_search, colour=False)
            assert x is None
            same_bits(dg, w['dg'], f'resident, pro, full search {full_search}: dg')
            same_bits(dgi, w['dgi'], f'resident, pro, full search {full_search}: dgi')
    d64 = _lib.default_context().device_copy(c.rho)
    dg, dgi, x = igm.igm_fields(d64, *args)
    assert all(isinstance(a, device.DeviceArray) for a in (dg, dgi, x))
    same_bits(dg.to_host(), v['dg'], 'float64 device array: dg')
    same_bits(dgi.to_host(), v['dgi'], 'float64 device array: dgi')
    same_bits(x.to_host(), x_want, 'float64 device array: x')
    rho32 = c.rho.astype(np.float32)
    v32 = restate(c.shape, c.lattice, c.atoms, c.species, c.pro, rho32.astype(np.float64), fr, MODES['stockholder'], sums=sums(name))
    d32 = _lib.default_context().device_copy(rho32)
    dg, dgi, _ = igm.igm_fields(d32, *args, colour=False)
    same_bits(dg.to_host(), v32['dg'], 'float32 device array: dg')
    same_bits(dgi.to_host(), v32['dgi'], 'float32 device array: dgi')
    if have_torch():
        perm = torch.as_tensor(np.ascontiguousarray(c.rho.transpose(2, 0, 1)), device='cuda').permute(1, 2, 0)
        assert tuple(perm.shape) == c.shape and not perm.is_contiguous()
        dg, dgi, _ = igm.igm_fields(perm, *args, colour=False)
        same_bits(dg.to_host(), v['dg'], 'permuted float64 tensor: dg')
        same_bits(dgi.to_host(), v['dgi'], 'permuted float64 tensor: dgi')


# ---- the region's sums ------------------------------------------------------------------------------------------------------------
def sum_inputs():
    """the restated dg_inter of cubic_r3 with the fragments {0..3}, {4..7}, and a colour field with all three classes"""
    c = HS.case(SUM_CASE)
    val = reference(SUM_CASE, 2, False, 'stockholder')['dgi'].reshape(c.shape)
    turn = np.indices(c.shape).sum(axis=0) % 3
    x = np.where(turn == 0, -1.0, np.where(turn == 1, 0.25, 1.0))      # with rho_split = 0.5: a third of the voxels per class
    return c, val, x


def test_sums_counts_are_exact_and_sums_are_under_the_bound(ctx):
    c, val, x = sum_inputs()
    rho_split = 0.5
    ctx.set_grid(c.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(c.rho)
    dval, dx = ctx.device_copy(val), ctx.device_copy(x)
    generic = 0.01 * float(val.max())
    on_a_voxel = float(np.sort(val[val > generic].reshape(-1))[37])
    assert (val > on_a_voxel).sum() == (val >= on_a_voxel).sum() - 1, 'the voxel lies ON the bound, alone'
    for n in (3, 85, 86, 400):       # LDS bins up to 85 labels (3 n <= 256 keys), global atomics beyond
        lab = label_map(c.shape, n)
        ctx.upload_labels(lab)
        for cut in (generic, on_a_voxel):
            cnt = check_sums(ctx.igm_sum(dval, dx, n, VV, cut, rho_split), c, val, x, lab, n, cut, rho_split, f'n = {n}, cut = {cut}')
            assert cnt.sum() > 300 and all(cnt[j::3].sum() > 30 for j in range(3)), 'every class holds voxels'
        assert np.array_equal(ctx.download_labels(np.int32), lab)
    assert np.array_equal(ctx.download_density(), c.rho) and np.array_equal(dval.to_host(), val), 'nothing resident is written'


def test_regions_through_the_python_layer():
    c, val, _ = sum_inputs()
    n, fr = 8, fragments(8, 2)
    lab = label_map(c.shape, n)
    x = nci.nci_fields(c.rho, c.lattice)[1]
    cut, rho_split = 0.02 * float(val.max()), 0.3 * float(np.abs(x).max())
    r = igm.igm_regions(c.rho, lab.astype(np.int8), c.lattice, c.atoms, fr, n, VV, cut, rho_split, c.species, c.pro)
    cnt = check_sums((r.count, r.charge, r.integral), c, val, x, lab, n, cut, rho_split, 'igm_regions')
    assert cnt.sum() > 300 and np.array_equal(r.volume, r.count.astype(np.float64) * VV)
    assert (r.cut, r.rho_split, r.mode, r.p_min) == (cut, rho_split, 'stockholder', igm.P_MIN)
    dgi = igm.igm_fields(c.rho, c.lattice, c.atoms, fr, c.species, c.pro, colour=False)[1]
    assert int(((dgi >= cut) & (lab >= 0) & (lab < n)).sum()) == cnt.sum(), 'the stored field meets the same comparison'
    empty = igm.igm_regions(c.rho, lab, c.lattice, c.atoms, fr, 0, VV, cut, rho_split, c.species, c.pro)
    assert empty.count.shape == empty.charge.shape == empty.integral.shape == empty.volume.shape == (0, 3)
    with pytest.raises(ValueError):
        igm.igm_regions(c.rho, np.zeros((3, 3, 3), np.int32), c.lattice, c.atoms, fr, n, VV, cut, rho_split, c.species, c.pro)


# ---- domains and surface ------------------------------------------------------------------------------------------------------------
def test_domains_equal_the_component_restatement_on_the_restated_field():
    c, val, _ = sum_inputs()
    n, fr = 3, fragments(8, 2)
    lab = label_map(c.shape, n)
    x = nci.nci_fields(c.rho, c.lattice)[1]
    level, rho_split = 0.05 * float(val.max()), 0.3 * float(np.abs(x).max())
    reg, seeds = components(val >= level)
    m = seeds.size
    count, top, _ = per_component(reg, m, c.rho)
    assert m >= 2 and (reg >= 0).any() and (reg < 0).any()
    d = igm.igm_domains(c.rho, c.lattice, c.atoms, fr, lab, n, VV, level, rho_split, c.species, c.pro)
    assert isinstance(d, igm.IgmDomains) and len(d) == d.m == m and isinstance(d.labels, np.ndarray)
    assert np.array_equal(d.labels, reg) and np.array_equal(d.seed, seeds) and np.array_equal(d.count, count) and np.array_equal(d.top, top)
    same_bits(d.value, val.reshape(-1)[top], 'value against the restated field')
    xt = x.reshape(-1)[top]
    assert d.kind.dtype == np.int8 and np.array_equal(d.kind, np.where(xt < -rho_split, 0, np.where(xt > rho_split, 2, 1)))
    s, cnt, mag = grouped(val, reg, m)
    assert np.array_equal(cnt, count) and np.all(np.abs(d.integral - s * VV) <= 3 * sum_bound(cnt, mag)), 'three class sums added'
    assert d.atoms.shape == (m, 2) and np.array_equal(d.volume, count.astype(np.float64) * VV) and (d.value >= level).all()
    assert (d.level, d.rho_split, d.mode) == (level, rho_split, 'stockholder')
    # the same for a device density (the labels then stay there), without a label map
    e = igm.igm_domains(_lib.default_context().device_copy(c.rho), c.lattice, c.atoms, fr, level=level, rho_split=rho_split,
                        species=c.species, proatoms=c.pro)
    assert isinstance(e.labels, device.DeviceArray) and np.array_equal(e.labels.to_host(), reg) and np.array_equal(e.top, top)
    assert np.array_equal(bits(e.value), bits(d.value)) and np.array_equal(e.kind, d.kind) and (e.atoms == -1).all()
    none = igm.igm_domains(c.rho, c.lattice, c.atoms, fr, level=2.0 * float(val.max()), species=c.species, proatoms=c.pro)
    assert none.m == 0 and none.value.shape == none.integral.shape == none.kind.shape == (0,)


def test_the_surface_is_the_isosurface_of_the_downloaded_fields():
    c, val, _ = sum_inputs()
    fr = fragments(8, 2)
    level = 0.05 * float(val.max())
    a = igm.igm_isosurface(c.rho, c.lattice, c.atoms, fr, level, c.species, c.pro)
    _, dgi, x = igm.igm_fields(c.rho, c.lattice, c.atoms, fr, c.species, c.pro)
    same_bits(dgi, val, 'the field the surface is made of')
    want = isosurface.isosurface(dgi, c.lattice, level, colour=x, density=c.rho)
    assert len(want.triangles) > 100
    b = igm.igm_isosurface(_lib.default_context().device_copy(c.rho), c.lattice, c.atoms, fr, level, c.species, c.pro)
    for got in (a, b):
        for name in ('vertices', 'colour', 'triangles', 'wrap', 'cells', 'positions'):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        # area and volume are float atomics in any order on both sides: two runs of at most 6 N + 2 terms bounded by the cell
        cell = abs(np.linalg.det(c.lattice))
        lim = 2 * (6 * c.rho.size + 2) * 2.0 ** -53
        assert abs(got.area - want.area) <= lim * want.area and abs(got.volume - want.volume) <= lim * cell
    assert a.level == level and np.isfinite(a.vertices).all()


# ---- error codes --------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        k = HS.case('three')
        shape, lat, n_vox = k.shape, np.ascontiguousarray(k.lattice, dtype=np.float64), k.rho.size
        fr = fragments(8, 2)
        state, arg, limit = _lib.XB_E_STATE, _lib.XB_E_ARG, _lib.XB_E_LIMIT
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        lp = lat.ctypes.data_as(pd)
        pf = fr.ctypes.data_as(C.c_void_p)
        out_a, out_b = np.full(n_vox, -7.0), np.full(n_vox, -7.0)
        pa, pb = out_a.ctypes.data_as(C.c_void_p), out_b.ctypes.data_as(C.c_void_p)
        st = (C.c_int64 * 3)()
        lib, h = c.lib, c.h
        good = (2, 1, 1e-6, 0)

        def field(lattice=lp, fragment=pf, rest=good, outs=(pa, pb, None, None)):
            return lib.xb_igm_field(h, lattice, fragment, *rest, *outs, st)

        assert field() == state                                            # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        assert field() == state                                            # no setup
        c.hirshfeld_setup(k.lattice, k.atoms, k.species, k.pro.tables, k.pro.r_cut)
        assert field() == state                                            # no density
        c.upload_density(k.rho)
        assert field() == 0
        assert (out_a != -7.0).all()
        out_a[:] = -7.0
        out_b[:] = -7.0
        da, db = device.DeviceArray(c, shape, np.float64), device.DeviceArray(c, shape, np.float64)
        va, vb = C.c_void_p(da.ptr), C.c_void_p(db.ptr)
        # null pointers, fragments outside their range, n_fragments outside 1 .. 4, an unknown mode, unknown flag bits, a p_min that
        # is negative or not finite, a lattice that is singular or not the setup's, a field on both sides, no field at all
        assert field(lattice=None) == arg and field(fragment=None) == arg
        for bad in (np.array([0, 1, 2, 0, 0, 0, 0, 0], np.int32), np.array([0, 1, -2, 0, 0, 0, 0, 0], np.int32)):
            assert field(fragment=bad.ctypes.data_as(C.c_void_p)) == arg
        for nf in (0, -1, 5):
            assert field(rest=(nf, 1, 1e-6, 0)) == arg, nf
        for mode in (-1, 2):
            assert field(rest=(2, mode, 1e-6, 0)) == arg, mode
        for flags in (2, 4, 3):
            assert field(rest=(2, 1, 1e-6, flags)) == arg, flags
        for p_min in (-1e-9, float('nan'), float('inf')):
            assert field(rest=(2, 1, p_min, 0)) == arg, p_min
        flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)
        other = (C.c_double * 9)(*(lat.reshape(-1) * 1.5))
        assert field(lattice=flat) == arg and field(lattice=other) == arg
        assert field(outs=(pa, pb, va, None)) == arg and field(outs=(pa, pb, None, vb)) == arg
        assert field(outs=(None, None, None, None)) == arg
        # device outputs: host pointers, one element past the allocation, not aligned, the two the same, the resident density
        assert field(outs=(None, None, pa, pb)) == arg
        assert field(outs=(None, None, va, C.c_void_p(db.ptr + 8))) == arg
        assert field(outs=(None, None, C.c_void_p(da.ptr + 4), vb)) == arg
        assert field(outs=(None, None, va, va)) == arg
        p_rho = C.c_void_p(int(lib.xb_density_ptr(h)))
        assert field(outs=(None, None, p_rho, None)) == arg and field(outs=(None, None, va, p_rho)) == arg
        assert (out_a == -7.0).all() and (out_b == -7.0).all(), 'a refused call writes nothing'
        assert np.array_equal(c.download_density(), k.rho)
        assert field(outs=(None, None, va, vb)) == 0 and field(outs=(pa, None, None, vb)) == 0
        # an MBIS setup is no table setup
        mc = MB.case('three')
        assert mc.shape == shape
        c.mbis_setup(mc.lattice, mc.atoms, mc.r_cut, mc.shells, MB.table(), 256, mc.N0, mc.s0, mc.bound, VV)
        assert field() == state
        c.hirshfeld_setup(k.lattice, k.atoms, k.species, k.pro.tables, k.pro.r_cut)
        assert field() == 0
        # the sums
        cnt, ch, it = np.full(6, -7, np.int64), np.full(6, -7.0), np.full(6, -7.0)
        pc, pch, pit = cnt.ctypes.data_as(pi), ch.ctypes.data_as(pd), it.ctypes.data_as(pd)

        def total(val=va, x=vb, n=2, cut=0.5, rho_split=0.01, outs=(pc, pch, pit)):
            return lib.xb_igm_sum(h, val, x, n, VV, cut, rho_split, *outs)

        assert total() == state                                            # no labels
        c.upload_labels(np.zeros(shape, np.int32))
        assert total(val=None) == arg and total(x=None) == arg
        assert total(outs=(None, pch, pit)) == arg and total(outs=(pc, None, pit)) == arg and total(outs=(pc, pch, None)) == arg
        assert total(n=0) == arg and total(n=-3) == arg
        for bad in (-0.25, float('nan'), float('inf')):
            assert total(rho_split=bad) == arg, bad
        for bad in (0.0, -0.0, -0.5, float('nan'), float('inf')):
            assert total(cut=bad) == arg, bad
        assert total(n=(2 ** 31 - 1) // 3 + 1) == limit
        assert total(val=pa) == arg and total(x=pb) == arg                 # host pointers
        assert total(val=C.c_void_p(da.ptr + 8)) == arg and total(x=C.c_void_p(db.ptr + 4)) == arg
        assert (cnt == -7).all() and (ch == -7.0).all() and (it == -7.0).all()
        assert total(cut=1e-300) == 0 and cnt[3:].sum() == 0 and (cnt >= 0).all()
        # a slab is refused; the whole grid works again
        c.set_grid((8, 8, 8), np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(np.random.default_rng(3).random((8, 8, 8)))
        c.upload_labels(np.zeros((8, 8, 8), np.int32))
        assert field() == state and total() == state
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(k.rho)
        c.hirshfeld_setup(k.lattice, k.atoms, k.species, k.pro.tables, k.pro.r_cut)
        dg, _, _ = c.igm_field(k.lattice, fr, 1, P_MIN, n_fragments=2)
        same_bits(dg, reference('three', 2, False, 'stockholder')['dg'], 'the whole grid again')
        # a setup made for another shape is no setup for this one
        c.set_grid((4, 3, 3), np.zeros(27), np.zeros(9))
        c.upload_density(np.zeros((4, 3, 3)))
        with pytest.raises(_lib.BaderHipError) as e:
            c.igm_field(k.lattice, fr, 1, P_MIN, n_fragments=2)
        assert e.value.code == state
    finally:
        c.close()


# ---- call history -------------------------------------------------------------------------------------------------------------------
HISTORY_FRAGMENTS = np.array([0, 1, 0], np.int32)


@functools.lru_cache(maxsize=None)
def history_reference(grid):
    rho = H.density(grid, 'A')
    return restate(rho.shape, H.LAT, H.sites_of('A'), H.SPECIES, H.proatoms('A'), rho, HISTORY_FRAGMENTS, MODES['stockholder'])


def igm_call(kind, grid):
    """one of the calls through the public functions on density A, its three atoms and the atom map of a grid of history_common
    -> None, or what differs from the restatement (which is what a fresh context gives: the other tests of this file)"""
    rho, lab, n = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms')
    fr = HISTORY_FRAGMENTS
    atoms = (H.LAT, H.sites_of('A'), fr, H.SPECIES, H.proatoms('A'))
    v = history_reference(grid)
    if kind == 'fields':
        dg, dgi, _ = igm.igm_fields(rho, *atoms, colour=False)
        if not np.array_equal(bits(dg).reshape(-1), bits(v['dg'])) or not np.array_equal(bits(dgi).reshape(-1), bits(v['dgi'])):
            return f'igm_fields on {grid}: differs'
        return None
    cut = float(np.quantile(v['dgi'][v['dgi'] > 0], 0.5))      # (half of the voxels with a positive value: the field peaks near the cutoffs)
    r = igm.igm_regions(rho, lab, H.LAT, H.sites_of('A'), fr, n, VV, cut, 1e300, H.SPECIES, H.proatoms('A'))
    want = sum_reference(rho, v['dgi'].reshape(rho.shape), np.zeros(rho.shape), lab, n, cut, 1e300)
    return regions_difference(r.count, r.charge, r.integral, want, f'igm_regions on {grid}')


@pytest.mark.parametrize('other', ['hirshfeld_charges', 'isa_charges', 'nci_regions', 'basin_laplacian',
                                   'regions', 'isosurface', 'charge_sum', 'weight_own'])
@pytest.mark.parametrize('kind', ['fields', 'regions'])
def test_call_history_does_not_matter(kind, other, monkeypatch):
    """each IGM call directly before and directly after the other call, on G1 -> G2 -> G1 of history_common.GRIDS, on the default
    context: the other call's results are what they are without IGM, IGM's what a fresh context gives"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    run = Runner()
    bad = []
    try:
        for grid in ('G1', 'G2', 'G1'):
            for step in (lambda: igm_call(kind, grid), lambda: run.checked(other, grid, 'A', 'atoms'), lambda: igm_call(kind, grid),
                         lambda: run.checked(other, grid, 'A', 'atoms')):
                msg = step()
                if msg:
                    bad.append(f'{grid}: {msg}')
        with utils.resident(H.density('G1', 'A')):
            for step in (lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: igm_call(kind, 'G1'),
                         lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: igm_call(kind, 'G1')):
                msg = step()
                if msg:
                    bad.append(f'resident(A): {msg}')
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, ' | '.join(bad[:4])


# ---- Bader(igm_flag=True) -------------------------------------------------------------------------------------------------------------
IGM_ATTRIBUTES = {'igm_flag', 'igm_fragments', 'igm_cut', 'igm_rho_split', 'atoms_igm_count', 'atoms_igm_volume', 'atoms_igm_charge',
                  'atoms_igm_integral'}
DOMAIN_ATTRIBUTES = {'igm_domains_flag', 'igm_domains', 'igm_domain_count', 'igm_domain_volume', 'igm_domain_charge', 'igm_domain_integral',
                     'igm_domain_kind', 'igm_domain_value', 'igm_domain_atoms', 'igm_domain_position'}


def test_bader_with_the_flags(monkeypatch):
    """the 8-atom synthetic at 24^3: every new attribute equals the direct calls and the restatement, and nothing else moves"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    shape, lat = (24, 24, 24), synth.TRICLINIC
    rho = synth.synth_density(shape, lat)
    atoms = synth.atoms_cartesian(synth.ATOMS8, lat)
    pro, species = HS.synth_proatoms(synth.ATOMS8, 3.0, 4096), np.arange(8, dtype=np.int32)
    fr = fragments(8, 2)

    def make(**flags):
        b = Bader({'charge': rho.copy()}, lat, atoms, **flags)
        b()
        return b

    with pytest.raises(ValueError, match='neither ran'):
        make(igm_flag=True, igm_fragments=fr)
    base = dict(hirshfeld_flag=True, proatoms=pro, species=species)
    off = make(**base)
    assert off.igm_flag is False and off.igm_domains_flag is False and not (IGM_ATTRIBUTES | DOMAIN_ATTRIBUTES) & set(vars(off))
    v = restate(shape, lat, atoms - off.voxel_offset, species, pro, rho, fr, MODES['stockholder'])
    cuts = dict(igm_cut=0.05 * float(v['dgi'].max()), igm_rho_split=0.03)
    on = make(igm_flag=True, igm_domains_flag=True, igm_fragments=fr, **cuts, **base)
    assert set(vars(on)) - set(vars(off)) == IGM_ATTRIBUTES | DOMAIN_ATTRIBUTES
    assert np.array_equal(host(on.atoms_volumes), host(off.atoms_volumes))
    assert np.allclose(on.atoms_charge, off.atoms_charge, rtol=2.0 ** -40, atol=0)      # (float atomics: two runs of one sum)
    assert np.allclose(on.hirshfeld_charge, off.hirshfeld_charge, rtol=2.0 ** -40, atol=0)
    n, vv = 8, on.voxel_volume
    lab = np.asarray(host(on.atoms_volumes))
    x = nci.nci_fields(rho, lat)[1]
    val = v['dgi'].reshape(shape)
    k = keys_of(val, x, lab, n, cuts['igm_cut'], cuts['igm_rho_split'])
    s1, cnt, mag1 = grouped(rho, k, 3 * n)
    s2, _, mag2 = grouped(val, k, 3 * n)
    print('atoms_igm_count', on.atoms_igm_count.tolist())
    assert on.atoms_igm_count.shape == (n, 3) and np.array_equal(on.atoms_igm_count.reshape(-1), cnt) and cnt.sum() > 100
    assert np.array_equal(on.atoms_igm_volume, on.atoms_igm_count.astype(np.float64) * vv)
    assert np.all(np.abs(on.atoms_igm_charge.reshape(-1) - s1 * vv) <= sum_bound(cnt, mag1, vv))
    assert np.all(np.abs(on.atoms_igm_integral.reshape(-1) - s2 * vv) <= sum_bound(cnt, mag2, vv))
    reg, seeds = components(val >= cuts['igm_cut'])
    assert on.igm_domains.m == seeds.size >= 1 and np.array_equal(host(on.igm_domains.labels), reg)
    count, top, _ = per_component(reg, seeds.size, rho)
    assert np.array_equal(on.igm_domain_count, count) and np.array_equal(on.igm_domains.top, top)
    same_bits(on.igm_domain_value, val.reshape(-1)[top], 'igm_domain_value')
    for name in ('count', 'volume', 'charge', 'integral', 'kind', 'value', 'atoms'):
        assert getattr(on, 'igm_domain_' + name) is getattr(on.igm_domains, name), name
    from pybader_amd.critical import positions
    assert np.array_equal(on.igm_domain_position, positions(top, shape, lat) + on.voxel_offset)
    # each flag alone, and ISA in the place of Hirshfeld
    lean = make(igm_flag=True, igm_fragments=fr, **cuts, **base)
    assert set(vars(lean)) & (IGM_ATTRIBUTES | DOMAIN_ATTRIBUTES) == IGM_ATTRIBUTES
    assert np.array_equal(lean.atoms_igm_count, on.atoms_igm_count)
    alone = make(igm_domains_flag=True, igm_fragments=fr, **cuts, **base)
    assert set(vars(alone)) & (IGM_ATTRIBUTES | DOMAIN_ATTRIBUTES) == DOMAIN_ATTRIBUTES | {'igm_fragments', 'igm_cut', 'igm_rho_split'}
    assert np.array_equal(alone.igm_domain_count, on.igm_domain_count)
    isa = make(igm_flag=True, igm_fragments=fr, isa_flag=True, isa_r_cut=2.0, isa_shells=16, isa_tol=1e-4, **cuts)
    assert isa.atoms_igm_count.shape == (n, 3) and isa.isa_charge.shape == (n,)

"""xb_isa_setup / xb_isa_iterate / xb_isa_tables and what stands on them (-m gpu) against the numpy restatement of
tests/test_isa_cpu.py.

The counts, every iteration's qsum row, the tables and the field of the iterated tables are compared with ==: the shell sums are
64-bit integers, so every iterate is bit-defined whatever the order of the atomics.  Each case runs through the three routes --
the waves' LDS windows (default), one global atomic per pair (XB_ISA_DIRECT) and the full search (XB_HIRSHFELD_FULL_SEARCH).  The
final charges and volumes are xb_hirshfeld_sum's float atomics and go against math.fsum under the float64 sum bound of section 19."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, device, hirshfeld, isa, laplacian, synth, utils
from pybader_amd.interface import Bader
from test_hirshfeld_cpu import VV, n_tiles, sum_bound
from test_hirshfeld_cpu import case as hs_case
from test_hirshfeld_cpu import reference_sums as hs_sums
from test_isa_cpu import CASES, case, exponent, geo, geometry, reference, restated_charges, run, total

pytestmark = pytest.mark.gpu
PRO, DEF = _lib.XB_HIRSHFELD_PROMOLECULE, _lib.XB_HIRSHFELD_DEFORMATION
ROUTES = {'windows': {}, 'direct': {'direct': True}, 'full_search': {'full_search': True}}
GPU_CASES = [n for n in CASES if n != 'tric_r3_k64']


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    diff = got.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ from the restatement, first at {np.flatnonzero(diff)[0]}'


def setup(ctx, c, initial=None, bound=None, density=True):
    ctx.set_grid(c.shape, np.zeros(27), np.zeros(9))
    if density:
        ctx.upload_density(c.rho)
    return ctx.isa_setup(c.lattice, c.atoms, c.r_cut, c.K, c.bound if bound is None else bound, initial)


def restated_sums(g, rho, A):
    """the restated charge and volume sums (fsum, before voxel_volume) on the tables A, with their term counts and magnitudes"""
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    charge, volume, w = restated_charges(g, rho, A, 1.0)
    none = ~(total(g, A) > 0)
    return dict(charge=charge, volume=volume, count=(w != 0).sum(axis=1), charge_mag=np.abs(rho * w).sum(axis=1), volume_mag=w.sum(axis=1),
                rest=(math.fsum(rho[none]), int(none.sum())), rest_mag=float(np.abs(rho[none]).sum()))


@functools.lru_cache(maxsize=None)
def final_sums(name):
    """... of one input on the tables after 7 iterations"""
    return restated_sums(geo(name), case(name).rho, reference(name)[2][6])


def check_sums(name, got, s, vv=VV):
    charge, volume, rest, _ = got
    lim_c, lim_v = sum_bound(s['count'], s['charge_mag'], vv), sum_bound(s['count'], s['volume_mag'], vv)
    assert charge.shape == s['charge'].shape and np.all(np.abs(charge - s['charge'] * vv) <= lim_c), name
    assert np.all(np.abs(volume - s['volume'] * vv) <= lim_v), name
    assert abs(rest[0] - s['rest'][0] * vv) <= sum_bound(s['rest'][1], s['rest_mag'], vv) and rest[1] == s['rest'][1] * vv, name


# ---- counts, iterates, the field, the sums: every case through every route ----------------------------------------------------
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('name', GPU_CASES)
def test_iterates_equal_the_restatement(ctx, name, route):
    c, g = case(name), geo(name)
    e, rows, tabs = reference(name)
    kw = ROUTES[route]
    info = setup(ctx, c)
    assert info == {'e': e, 'cmax': int(g.count.max()), 'pairs': int(g.count.sum()), 'empty_shells': int((g.count == 0).sum())}, name
    A0, count = ctx.isa_tables()
    assert count.dtype == np.int64 and np.array_equal(count, g.count), name
    same_bits(A0, np.ones((g.n, g.K)), f'{name}: the start')
    got_rows, done = [], 0
    for iters in (1, 1, 5):      # after 1, 2 and 7 iterations
        q, stats = ctx.isa_iterate(iters, **kw)
        got_rows.append(q)
        done += iters
        assert q.dtype == np.int64 and np.array_equal(np.concatenate(got_rows), rows[:done]), (name, route, done)
        same_bits(ctx.isa_tables()[0], tabs[done - 1], f'{name} ({route}): the tables after {done} iterations')
        tiles = n_tiles(c.shape)
        assert stats['candidate_tiles'] + stats['full_tiles'] == tiles and stats['beyond_bound'] == 0
        if route == 'full_search':
            assert stats['full_tiles'] == tiles and stats['max_candidates'] == 0
        elif CASES[name][-1] == 'overflow':
            assert stats['candidate_tiles'] == 0 and stats['max_candidates'] > _lib.XB_HIRSHFELD_CAND_MAX
        else:
            assert stats['full_tiles'] == 0 and stats['max_candidates'] <= _lib.XB_HIRSHFELD_CAND_MAX
    assert np.array_equal(ctx.isa_tables()[1], g.count), 'the counts stay'
    full = route == 'full_search'
    P = total(g, tabs[6])
    same_bits(ctx.hirshfeld_field(PRO, full), P, f'{name} ({route}): the field of the iterated tables')
    same_bits(ctx.hirshfeld_field(DEF, full), c.rho.reshape(-1) - P, f'{name} ({route}): the residual')
    got = ctx.hirshfeld_sum(VV, full)
    if g.N == 1:
        # a one-voxel grid: every sum has one term per atom at most -- compared with ==
        s = final_sums(name)
        assert np.array_equal(got[0], s['charge'] * VV) and np.array_equal(got[1], s['volume'] * VV)
    check_sums(f'{name} ({route})', got, final_sums(name))
    assert np.array_equal(ctx.download_density(), c.rho), 'the resident density is not written'
    if name == 'negative':
        # shells whose sum is not positive clamp to zero and stay zero
        zero = [(t == 0) & (g.count > 0) for t in tabs]
        assert zero[0].any() and all((zero[i + 1] | ~zero[i]).all() for i in range(6))
    if name.startswith('cubic_r2'):
        assert got[2][1] > 0, 'voxels that belong to nobody'


def test_five_iterations_in_one_call_are_five_calls_of_one(ctx):
    c = case('tric_r2_k64')
    setup(ctx, c)
    q5, _ = ctx.isa_iterate(5)
    A5 = ctx.isa_tables()[0]
    setup(ctx, c)
    q1 = np.concatenate([ctx.isa_iterate(1)[0] for _ in range(5)])
    assert np.array_equal(q5, q1)
    same_bits(ctx.isa_tables()[0], A5, 'five calls of one')
    before = ctx.host_waits()
    ctx.isa_iterate(7)
    assert ctx.host_waits() - before == 1, 'one host wait per call'


def test_a_callers_initial_tables(ctx):
    name = 'cubic_r2_k16'
    c, g = case(name), geo(name)
    initial = 0.5 + synth.hash_noise((g.n, g.K), 5)
    initial[3, :4] = 0.0
    info = setup(ctx, c, initial=initial)
    same_bits(ctx.isa_tables()[0], initial, 'the start')
    rows, tabs = run(g, c.rho, info['e'], 3, initial)
    for route, kw in ROUTES.items():
        setup(ctx, c, initial=initial)
        q, _ = ctx.isa_iterate(3, **kw)
        assert np.array_equal(q, rows), route
        same_bits(ctx.isa_tables()[0], tabs[-1], f'{route}: from the initial tables')
    assert (tabs[-1][3, :4] == 0).all(), 'a zero shell stays zero'
    # the same tables loaded into a setup that has iterated already: the counts and e stay, the iterates are the same
    setup(ctx, c)
    ctx.isa_iterate(2)
    ctx.isa_load(initial)
    same_bits(ctx.isa_tables()[0], initial, 'the loaded tables')
    q, _ = ctx.isa_iterate(3)
    assert np.array_equal(q, rows) and np.array_equal(ctx.isa_tables()[1], g.count)
    same_bits(ctx.isa_tables()[0], tabs[-1], 'from the loaded tables')
    for bad in (-initial, np.where(initial > 1, np.nan, initial)):
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.isa_load(bad)
        assert e.value.code == _lib.XB_E_ARG
    same_bits(ctx.isa_tables()[0], tabs[-1], 'a refused load leaves the tables')


@pytest.mark.parametrize('f32', [False, True], ids=['float64', 'float32'])
def test_a_device_density(ctx, f32):
    name = 'tric_r3_k16'
    c, g = case(name), geo(name)
    rho = c.rho.astype(np.float32) if f32 else c.rho
    rho64 = rho.astype(np.float64)
    bound = float(np.abs(rho64).max())
    e = exponent(bound, g.count.max())
    rows, tabs = run(g, rho64, e, 7)
    x = _lib.default_context()
    x.set_grid(c.shape, np.zeros(27), np.zeros(9))
    dev = x.device_copy(rho)
    vv = 0.0371
    r = isa.isa_charges(dev, c.lattice, c.atoms, vv, r_cut=c.r_cut, shells=c.K, tol=0.0, max_iter=7, check_every=3)
    assert x.density_absmax() == bound and r.rho_bound == bound and r.stats['e'] == e
    assert r.iterations == 7 and not r.converged and r.history.shape == (7, g.n)
    assert np.array_equal(r.history, rows.astype(np.float64) * (2.0 ** -e * vv))
    same_bits(r.tables, tabs[6], 'the tables of isa_charges on a device density')
    assert np.array_equal(r.counts, g.count)
    check_sums('isa_charges on a device density', (r.charge, r.volume, r.rest, None), restated_sums(g, rho64, tabs[6]), vv)
    res = isa.isa_residual(dev, c.lattice, c.atoms, r)
    pro = isa.isa_promolecule(dev, c.lattice, c.atoms, r)
    assert isinstance(res, device.DeviceArray) and isinstance(pro, device.DeviceArray)
    same_bits(pro.to_host(), total(g, tabs[6]), 'isa_promolecule')
    same_bits(res.to_host(), rho64.reshape(-1) - total(g, tabs[6]), 'isa_residual')


def test_isa_charges_stops_at_the_first_iteration_below_tol():
    """the history's last row is the first whose change lies below tol, and the tables are that iteration's, although the library
    ran check_every iterations per call"""
    name = 'cubic_r3_k64'
    c, g = case(name), geo(name)
    vv = 0.0156
    tol = 2e-3
    r = isa.isa_charges(c.rho, c.lattice, c.atoms, vv, r_cut=c.r_cut, shells=c.K, tol=tol, check_every=16)
    r7 = isa.isa_charges(c.rho, c.lattice, c.atoms, vv, r_cut=c.r_cut, shells=c.K, tol=tol, check_every=7)
    # (one of the two stops inside a call, unless the iteration count is a multiple of 112)
    assert r7.iterations == r.iterations and r.iterations % 112 != 0 and np.array_equal(r7.history, r.history)
    same_bits(r7.tables, r.tables, 'check_every changes nothing')
    e = r.stats['e']
    rows, tabs = run(g, c.rho, e, r.iterations)
    hist = rows.astype(np.float64) * (2.0 ** -e * vv)
    change = np.abs(np.diff(hist, axis=0)).max(axis=1)
    assert r.converged and 2 < r.iterations < 2000
    assert change[-1] < tol and (change[:-1] >= tol).all()
    assert np.array_equal(r.history, hist)
    same_bits(r.tables, tabs[-1], 'the tables of the iteration that converged')
    host_pro = isa.isa_promolecule(c.rho, c.lattice, c.atoms, r)
    assert isinstance(host_pro, np.ndarray) and host_pro.shape == c.shape
    same_bits(host_pro, total(g, tabs[-1]), 'isa_promolecule on a host density')


# ---- errors -------------------------------------------------------------------------------------------------------------------
def code(call):
    with pytest.raises(_lib.BaderHipError) as e:
        call()
    return e.value.code


def test_a_density_beyond_rho_bound_is_refused_and_the_tables_stay(ctx):
    c = case('cubic_r2_k16')
    for kw in ROUTES.values():
        setup(ctx, c)
        ctx.isa_iterate(2)
        before = ctx.isa_tables()[0].copy()
        # the same setup with a bound below max |rho|: the tables of two iterations as the start
        setup(ctx, c, initial=before, bound=0.5 * c.bound)
        for iters in (1, 2, 5):
            assert code(lambda: ctx.isa_iterate(iters, **kw)) == _lib.XB_E_ARG
            same_bits(ctx.isa_tables()[0], before, f'the tables after a refused call of {iters}')
        assert 'rho_bound' in _lib.load().xb_last_error().decode()
        # a bound that holds: the call after the refused ones gives what it gives alone
        ctx.upload_density(c.rho * 0.25)
        q, st = ctx.isa_iterate(1, **kw)
        assert st['beyond_bound'] == 0
        g = geo('cubic_r2_k16')
        rows, tabs = run(g, c.rho * 0.25, exponent(0.5 * c.bound, g.count.max()), 1, before)
        assert np.array_equal(q, rows)
        same_bits(ctx.isa_tables()[0], tabs[0], 'the iteration after a refused call')


def test_error_codes(ctx):
    c = case('three')
    A, S, L = _lib.XB_E_ARG, _lib.XB_E_STATE, _lib.XB_E_LIMIT
    x = _lib.Context(0)
    try:
        assert code(lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, 1.0)) == S         # no grid
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        assert code(lambda: x.isa_iterate(1)) == S and code(lambda: x.isa_tables()) == S   # no setup
        assert code(lambda: x.density_absmax()) == S                                       # no density
        x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, c.bound)
        assert code(lambda: x.isa_iterate(1)) == S                                         # no density
        x.upload_density(c.rho)
        good = x.isa_iterate(1)[0]
        tables = x.isa_tables()[0]
        for call in (lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 0, 1.0),
                     lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, 0.0),
                     lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, np.inf),
                     lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, np.nan),
                     lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut * 0, 4, 1.0),
                     lambda: x.isa_setup(c.lattice, c.atoms * np.nan, c.r_cut, 4, 1.0),
                     lambda: x.isa_setup(c.lattice * 0, c.atoms, c.r_cut, 4, 1.0),
                     lambda: x.isa_setup(c.lattice, c.atoms[:0], c.r_cut[:0], 4, 1.0),
                     lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, 1.0, -np.ones((8, 4))),
                     lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, 1.0, np.full((8, 4), np.inf)),
                     lambda: x.isa_iterate(0), lambda: x.isa_iterate(-3)):
            assert code(call) == A
        assert code(lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, (1 << 26) // 8 + 1, 1.0)) == L
        assert code(lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut * 1e4, 4, 1.0)) == L
        assert code(lambda: x.isa_iterate(_lib.XB_ISA_ITERS_MAX + 1)) == L
        lib = x.lib
        q = np.zeros(8, np.int64)
        assert lib.xb_isa_iterate(x.h, 1, 4, q.ctypes.data_as(_lib._pi64), None) == A                      # an unknown flag bit
        assert lib.xb_isa_iterate(x.h, 1, 0, None, None) == A
        assert lib.xb_isa_tables(x.h, None, None) == A
        assert lib.xb_isa_load(x.h, None) == A
        # more atoms than any table holds: refused before anything is sized by n or read
        lat9, at3, rc8 = np.ascontiguousarray(c.lattice), np.ascontiguousarray(c.atoms), np.ascontiguousarray(c.r_cut)
        info = (C.c_int64 * 4)()
        for n in (1 << 40, (1 << 26) // 4 + 1):
            assert lib.xb_isa_setup(x.h, lat9.ctypes.data_as(_lib._pdbl), at3.ctypes.data_as(_lib._pdbl), n, rc8.ctypes.data_as(_lib._pdbl),
                                    4, None, 1.0, info) == L
        assert lib.xb_isa_rho_bound(x.h, None) == A
        # every refused call left the setup alone
        same_bits(x.isa_tables()[0], tables, 'the tables after the refused calls')
        x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, c.bound)
        assert np.array_equal(x.isa_iterate(1)[0], good)
        # a new shape clears it
        x.set_grid((4, 3, 3), np.zeros(27), np.zeros(9))
        assert code(lambda: x.isa_iterate(1)) == S and code(lambda: x.hirshfeld_field(PRO)) == S
        # a Hirshfeld setup is no ISA setup
        h = hs_case('three')
        x.set_grid(h.shape, np.zeros(27), np.zeros(9))
        x.upload_density(h.rho)
        x.hirshfeld_setup(h.lattice, h.atoms, h.species, h.pro.tables, h.pro.r_cut)
        assert code(lambda: x.isa_iterate(1)) == S and code(lambda: x.isa_tables()) == S and code(lambda: x.isa_load(np.ones((8, 4)))) == S
        # a slab of the same shape: refused, and fine again on the whole grid; the block is hs_buf, with the size the header gives
        x.hirshfeld_release()
        c = case('cubic_r2_k16')
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        x.upload_density(c.rho)
        before = x.memory_stats()
        x.isa_setup(c.lattice, c.atoms, c.r_cut, c.K, c.bound)
        after = x.memory_stats()
        n, K = c.atoms.shape[0], c.K
        n_img = _lib.hirshfeld_images(c.lattice, c.atoms, np.arange(n), c.r_cut).shape[0]
        words = 16 + 3 * sum(c.shape) + 3 * n
        words += words & 1
        words += 2 * n * K + 4 * n_img + 2 * n + 3
        words += words & 1
        words += 4 * n * K + _lib.XB_ISA_ITERS_MAX * n + 1
        assert after[2] - before[2] == 8 * words
        good = x.isa_iterate(2)[0]
        x.set_grid(c.shape, np.zeros(27), np.zeros(9), (2, 9))
        for call in (lambda: x.isa_iterate(1), lambda: x.isa_tables(), lambda: x.isa_setup(c.lattice, c.atoms, c.r_cut, c.K, c.bound)):
            assert code(call) == S
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        x.upload_density(c.rho)
        assert np.array_equal(np.concatenate([good, x.isa_iterate(1)[0]]), reference('cubic_r2_k16')[1][:3])
        x.hirshfeld_release()
        assert x.memory_stats()[2] == before[2] and code(lambda: x.isa_iterate(1)) == S
    finally:
        x.close()


# ---- history: ISA between the other analyses ------------------------------------------------------------------------------------
def test_isa_then_hirshfeld_then_isa(ctx):
    """each gives what it gives alone: the one setup of the context is replaced, not mixed"""
    name = 'three'
    c, h = case(name), hs_case('three')
    e, rows, tabs = reference(name)
    x = _lib.default_context()
    alone = hirshfeld.hirshfeld_charges(h.rho, h.lattice, h.atoms, h.species, h.pro, VV)
    r1 = isa.isa_charges(c.rho, c.lattice, c.atoms, VV, r_cut=c.r_cut, shells=c.K, tol=0.0, max_iter=7)
    assert x.hirshfeld_key is None, 'an ISA setup clears what hirshfeld._setup remembered'
    between = hirshfeld.hirshfeld_charges(h.rho, h.lattice, h.atoms, h.species, h.pro, VV)
    with pytest.raises(_lib.BaderHipError):
        x.isa_iterate(1)
    r2 = isa.isa_charges(c.rho, c.lattice, c.atoms, VV, r_cut=c.r_cut, shells=c.K, tol=0.0, max_iter=7)
    for r in (r1, r2):
        same_bits(r.tables, tabs[6], 'the tables')
        assert np.array_equal(r.history, rows.astype(np.float64) * (2.0 ** -e * VV))
    # the Hirshfeld sums of the two calls are float atomics in an order of their own each: either lies within section 19's bound of
    # the one restated sum, so the two within twice that bound of each other
    s = hs_sums('three')
    for got in (alone, between):
        assert np.all(np.abs(got[0] - s['charge'] * VV) <= sum_bound(s['count'], s['charge_mag']))
        assert np.all(np.abs(got[1] - s['volume'] * VV) <= sum_bound(s['count'], s['volume_mag']))
    assert np.all(np.abs(alone[0] - between[0]) <= 2 * sum_bound(s['count'], s['charge_mag']))
    assert np.array_equal(alone[2], between[2]) and alone[3] == between[3]


def test_the_neighbours_give_the_same_before_and_after(ctx):
    """xb_charge_sum on a label map and the Laplacian of the density: the same bits before and after an ISA run on the context"""
    name = 'cubic_r2_k16'
    c = case(name)
    x = _lib.default_context()
    labels = (np.arange(c.rho.size, dtype=np.int64).reshape(c.shape) // 7 % 5).astype(np.int32)
    rho = np.round(c.rho * 2.0 ** 20) / 2.0 ** 20           # (multiples of 2^-20: the charge sums are exact in any order)

    def neighbours():
        charge, volume = np.zeros(5), np.zeros(5)
        utils.charge_sum(charge, volume, VV, rho, labels)
        return charge, volume, laplacian.laplacian(rho, c.lattice)

    before = neighbours()
    isa.isa_charges(rho, c.lattice, c.atoms, VV, r_cut=c.r_cut, shells=c.K, tol=0.0, max_iter=3)
    after = neighbours()
    for b, a in zip(before, after):
        assert np.array_equal(np.asarray(b), np.asarray(a))
    assert np.array_equal(x.download_density(), rho)


# ---- Bader(isa_flag=True) -------------------------------------------------------------------------------------------------------
def _host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


@pytest.mark.parametrize('spin', [False, True], ids=['charge', 'charge and spin'])
@pytest.mark.parametrize('on_device', [False, True], ids=['host density', 'device density'])
def test_bader_with_the_flag(on_device, spin):
    """two unequal atoms at 24^3.  The densities are rounded to multiples of 2^-20, which makes every charge sum of the run without
    the flag exact in any order: its attributes can be compared bit for bit between the two runs"""
    shape, lat = (24, 24, 24), synth.TRICLINIC
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5, 0.0) * 2.0 ** 20) / 2.0 ** 20
    sp_rho = np.round(rho * (synth.hash_noise(shape, 11) - 0.5) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(atoms5, lat)
    ctx = _lib.default_context()

    def dev(a):
        if not on_device:
            return a.copy()
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        ctx.upload_density(a)
        ctx.upload_labels(np.zeros(shape, np.int8))
        return ctx.export_volume(0)          # a library-owned device array holding the density

    def density():
        return {'charge': dev(rho), 'spin': dev(sp_rho)} if spin else {'charge': dev(rho)}

    off = Bader(density(), lat, atoms, spin_flag=spin, voronoi_flag=True)
    off()
    on = Bader(density(), lat, atoms, spin_flag=spin, voronoi_flag=True, isa_flag=True, isa_r_cut=2.5, isa_shells=20, isa_tol=1e-7)
    on()
    new = {'isa_flag', 'isa_r_cut', 'isa_shells', 'isa_tol', 'isa_charge', 'isa_volume', 'isa_rest', 'isa_iterations',
           'isa_converged'} | ({'isa_spin'} if spin else set())
    assert set(vars(on)) - set(vars(off)) == new, (set(vars(on)) - set(vars(off))) ^ new
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference'):
            continue
        got, want = _host(getattr(on, key)), _host(want)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert got == want, key
    # against the restatement run to the same tolerance
    vv = on.voxel_volume
    g = geometry(shape, lat, atoms - on.voxel_offset, 2.5, 20)
    e = exponent(np.abs(rho).max(), g.count.max())
    rows, tabs = run(g, rho, e, on.isa_iterations)
    hist = rows.astype(np.float64) * (2.0 ** -e * vv)
    change = np.abs(np.diff(hist, axis=0)).max(axis=1)
    assert on.isa_converged and on.isa_iterations > 3 and change[-1] < 1e-7 and (change[:-1] >= 1e-7).all()
    charge, volume, w = restated_charges(g, rho.reshape(-1), tabs[-1], vv)
    count = (w != 0).sum(axis=1)
    assert np.all(np.abs(on.isa_charge - charge) <= sum_bound(count, np.abs(rho.reshape(-1) * w).sum(axis=1), vv))
    assert np.all(np.abs(on.isa_volume - volume) <= sum_bound(count, w.sum(axis=1), vv))
    if spin:
        s_charge, _, _ = restated_charges(g, sp_rho.reshape(-1), tabs[-1], vv)
        assert np.all(np.abs(on.isa_spin - s_charge) <= sum_bound(count, np.abs(sp_rho.reshape(-1) * w).sum(axis=1), vv))
    print('Bader', on.atoms_charge.tolist(), 'Voronoi', on.voronoi_charge.tolist(), 'ISA', on.isa_charge.tolist(), on.isa_iterations)

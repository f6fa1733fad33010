"""xb_mbis_setup / xb_mbis_iterate / xb_mbis_params / xb_mbis_load / xb_mbis_field and what stands on them (-m gpu) against the
numpy restatement of tests/test_mbis_cpu.py.

The info, the counts, every iteration's row (qsum, vsum, rest), the parameters and both fields are compared with ==: the sums are
64-bit integers, so every iterate is bit-defined whatever the order of the atomics, and the charges are exact scalings of them.
Each case runs through the three routes -- sums in registers, over the wave and in LDS (default), one global atomic per pair and
shell (XB_MBIS_DIRECT) and the full search (XB_HIRSHFELD_FULL_SEARCH)."""
import ctypes as C
import warnings

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, device, isa, mbis, synth
from pybader_amd.interface import Bader
from test_hirshfeld_cpu import n_tiles
from test_hirshfeld_cpu import case as hs_case
from test_mbis_cpu import CASES, VV, Table, case, exponents, geo, geometry, reference, results, run, same_rows, table, total

pytestmark = pytest.mark.gpu
PRO, DEF = _lib.XB_HIRSHFELD_PROMOLECULE, _lib.XB_HIRSHFELD_DEFORMATION
ROUTES = {'reduced': {}, 'direct': {'direct': True}, 'full_search': {'full_search': True}}
J = 256


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


def setup(ctx, c, N=None, sigma=None, bound=None, density=True, vv=VV):
    ctx.set_grid(c.shape, np.zeros(27), np.zeros(9))
    if density:
        ctx.upload_density(c.rho)
    return ctx.mbis_setup(c.lattice, c.atoms, c.r_cut, c.shells, table(), J, c.N0 if N is None else N, c.s0 if sigma is None else sigma,
                          c.bound if bound is None else bound, vv)


# ---- info, counts, rows, parameters, fields: every case through every route ------------------------------------------------------
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('name', list(CASES))
def test_iterates_equal_the_restatement(ctx, name, route):
    c, g = case(name), geo(name)
    e, rows, pars = reference(name)
    kw = ROUTES[route]
    info = setup(ctx, c)
    assert info == {'eN': e[0], 'eS': e[1], 'eV': e[2], 'eR': e[3], 'cmax': int(g.count.max()), 'pairs': int(g.count.sum())}, name
    N0, s0, count = ctx.mbis_params()
    assert count.dtype == np.int64 and np.array_equal(count, g.count), name
    same_bits(N0, c.N0, f'{name}: the start')
    same_bits(s0, c.s0, f'{name}: the start')
    tiles, done = n_tiles(c.shape), 0
    for iters in (1, 1, 5):      # after 1, 2 and 7 iterations
        q, v, r, stats = ctx.mbis_iterate(iters, **kw)
        same_rows((q, v, r), rows[done:done + iters], f'{name} ({route}): iterations {done} .. {done + iters}')
        done += iters
        N, sg, _ = ctx.mbis_params()
        same_bits(N, pars[done - 1][0], f'{name} ({route}): the populations after {done} iterations')
        same_bits(sg, pars[done - 1][1], f'{name} ({route}): the widths after {done} iterations')
        assert stats['candidate_tiles'] + stats['full_tiles'] == tiles and stats['beyond_bound'] == 0
        if route == 'full_search':
            assert stats['full_tiles'] == tiles and stats['max_candidates'] == 0
        elif CASES[name][-1] == 'overflow':
            assert stats['candidate_tiles'] == 0 and stats['max_candidates'] > _lib.XB_HIRSHFELD_CAND_MAX
        else:
            assert stats['full_tiles'] == 0 and stats['max_candidates'] <= _lib.XB_HIRSHFELD_CAND_MAX
    assert np.array_equal(ctx.mbis_params()[2], g.count), 'the counts stay'
    full = route == 'full_search'
    P = total(g, Table(table(), J), c.shells, *pars[6])
    same_bits(ctx.mbis_field(PRO, full), P, f'{name} ({route}): the field of the iterated atoms')
    same_bits(ctx.mbis_field(DEF, full), c.rho.reshape(-1) - P, f'{name} ({route}): the residual')
    assert np.array_equal(ctx.download_density(), c.rho), 'the resident density is not written'
    # the results are exact scalings of the last row
    charge, volume, rest = results(e, rows[6])
    got = mbis._results(info, VV, q[-1], v[-1], r[-1])
    same_bits(got[0], charge, 'charge')
    same_bits(got[1], volume, 'volume')
    same_bits(got[2], rest, 'rest')


def test_five_iterations_in_one_call_are_five_calls_of_one(ctx):
    c = case('tric_mixed')
    setup(ctx, c)
    q5, v5, r5, _ = ctx.mbis_iterate(5)
    p5 = ctx.mbis_params()
    setup(ctx, c)
    one = [ctx.mbis_iterate(1)[:3] for _ in range(5)]
    for k, got in enumerate((q5, v5, r5)):
        assert np.array_equal(got, np.concatenate([o[k] for o in one]))
    same_bits(ctx.mbis_params()[0], p5[0], 'five calls of one')
    same_bits(ctx.mbis_params()[1], p5[1], 'five calls of one')
    before = ctx.host_waits()
    ctx.mbis_iterate(7)
    assert ctx.host_waits() - before == 1, 'one host wait per call'


def test_keep_leaves_the_parameters_and_load_round_trips(ctx):
    name = 'tric_mixed'
    c, g = case(name), geo(name)
    e, rows, pars = reference(name)
    for route, kw in ROUTES.items():
        setup(ctx, c)
        ctx.mbis_iterate(2, **kw)
        N, sg, _ = ctx.mbis_params()
        q, v, r, _ = ctx.mbis_iterate(1, keep=True, **kw)
        same_rows((q, v, r), rows[2:3], f'{route}: the kept pass is the third iteration')
        N2, sg2, _ = ctx.mbis_params()
        same_bits(N2, N, f'{route}: XB_MBIS_KEEP leaves the populations')
        same_bits(sg2, sg, f'{route}: XB_MBIS_KEEP leaves the widths')
        # another density on the same weights: the spin pass
        other = c.rho * (synth.hash_noise(c.shape, 11) - 0.5)
        ctx.upload_density(other)
        qs = ctx.mbis_iterate(1, keep=True, **kw)[0]
        want = run(g, Table(table(), J), c.shells, other, *pars[1], c.bound, e, 1)[0][0]
        assert np.array_equal(qs[0], want[0]), route
        ctx.upload_density(c.rho)
        same_rows(ctx.mbis_iterate(1, **kw)[:3], rows[2:3], f'{route}: and the iteration after it')
    # load after params round-trips, into a setup that has iterated on: the counts and exponents stay, the iterates are the same
    setup(ctx, c)
    ctx.mbis_iterate(2)
    N, sg, _ = ctx.mbis_params()
    ctx.mbis_iterate(3)
    ctx.mbis_load(N, sg)
    N2, sg2, count = ctx.mbis_params()
    same_bits(N2, N, 'the loaded populations')
    same_bits(sg2, sg, 'the loaded widths')
    same_rows(ctx.mbis_iterate(5)[:3], rows[2:7], 'from the loaded parameters')
    same_bits(ctx.mbis_params()[0], pars[6][0], 'from the loaded parameters')
    assert np.array_equal(count, g.count)
    for bad_N, bad_s in ((-N, sg), (np.where(N > 0.3, np.nan, N), sg), (N, sg * 0), (N, -sg), (N, np.where(sg > 0.3, np.inf, sg))):
        with pytest.raises(_lib.BaderHipError) as err:
            ctx.mbis_load(bad_N, bad_s)
        assert err.value.code == _lib.XB_E_ARG
    same_bits(ctx.mbis_params()[0], pars[6][0], 'a refused load leaves the parameters')


@pytest.mark.parametrize('f32', [False, True], ids=['float64', 'float32'])
def test_a_device_density_equals_the_host_one(f32):
    name = 'tric_mixed'
    c, g = case(name), geo(name)
    rho = c.rho.astype(np.float32) if f32 else c.rho
    rho64 = rho.astype(np.float64)
    bound = float(np.abs(rho64).max())
    e = exponents(bound, g.count.max(), c.r_cut.max(), g.N)
    rows, pars = run(g, Table(table(), J), c.shells, rho64, c.N0, c.s0, bound, e, 7)
    x = _lib.default_context()
    x.set_grid(c.shape, np.zeros(27), np.zeros(9))
    dev = x.device_copy(rho)
    kw = dict(shells=c.shells, r_cut=c.r_cut, tol=0.0, max_iter=7, check_every=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r = mbis.mbis_charges(dev, c.lattice, c.atoms, VV, **kw)
        h = mbis.mbis_charges(rho64, c.lattice, c.atoms, VV, **kw)
    assert r.rho_bound == bound and (r.stats['eN'], r.stats['eS'], r.stats['eV'], r.stats['eR']) == e
    assert r.iterations == 7 and not r.converged and r.history.shape == (7, g.n)
    want = results(e, rows[6])
    for got in (r, h):
        same_bits(got.charge, want[0], 'charge')
        same_bits(got.volume, want[1], 'volume')
        same_bits(got.rest, want[2], 'rest')
        same_bits(got.populations, pars[6][0], 'populations')
        same_bits(got.widths, pars[6][1], 'widths')
        same_bits(got.history, np.array([results(e, row)[0] for row in rows]), 'history')
        same_bits(got.tail, mbis.tail(pars[6][0], pars[6][1], c.r_cut), 'tail')
    res = mbis.mbis_residual(dev, c.lattice, c.atoms, r)
    pro = mbis.mbis_promolecule(dev, c.lattice, c.atoms, r)
    assert isinstance(res, device.DeviceArray) and isinstance(pro, device.DeviceArray)
    P = total(g, Table(table(), J), c.shells, *pars[6])
    same_bits(pro.to_host(), P, 'mbis_promolecule')
    same_bits(res.to_host(), rho64.reshape(-1) - P, 'mbis_residual')
    host_pro = mbis.mbis_promolecule(rho64, c.lattice, c.atoms, h)
    assert isinstance(host_pro, np.ndarray) and host_pro.shape == c.shape
    same_bits(host_pro, P, 'mbis_promolecule on a host density')


def test_mbis_charges_stops_at_the_first_iteration_below_tol():
    """the history's last row is the first whose change lies below tol, and the parameters are that iteration's, although the
    library ran check_every iterations per call"""
    name = 'cubic_m1'
    c, g = case(name), geo(name)
    tol = 1e-6
    with pytest.warns(RuntimeWarning, match='truncates'):      # (r_cut = 3 A cuts 1e-3 of an atom off)
        r = mbis.mbis_charges(c.rho, c.lattice, c.atoms, VV, shells=c.shells, r_cut=c.r_cut, tol=tol, check_every=8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r5 = mbis.mbis_charges(c.rho, c.lattice, c.atoms, VV, shells=c.shells, r_cut=c.r_cut, tol=tol, check_every=5)
    # (one of the two stops inside a call, unless the iteration count is a multiple of 40)
    assert r5.iterations == r.iterations and r.iterations % 40 != 0 and np.array_equal(r5.history, r.history)
    same_bits(r5.populations, r.populations, 'check_every changes nothing')
    e = exponents(c.bound, g.count.max(), c.r_cut.max(), g.N)
    rows, pars = run(g, Table(table(), J), c.shells, c.rho, c.N0, c.s0, c.bound, e, r.iterations)
    hist = np.array([results(e, row)[0] for row in rows])
    change = np.abs(np.diff(hist, axis=0)).max(axis=1)
    assert r.converged and 2 < r.iterations < 60
    assert change[-1] < tol and (change[:-1] >= tol).all()
    same_bits(r.history, hist, 'history')
    same_bits(r.populations, pars[-1][0], 'the populations of the iteration that converged')
    same_bits(r.widths, pars[-1][1], 'the widths of the iteration that converged')
    same_bits(r.charge, hist[-1], 'the charge is the last row')
    assert (r.tail > 1e-3).any() and r.tail.max() < 0.1


# ---- errors -------------------------------------------------------------------------------------------------------------------
def code(call):
    with pytest.raises(_lib.BaderHipError) as e:
        call()
    return e.value.code


def test_a_density_beyond_rho_bound_is_refused_and_the_parameters_stay(ctx):
    name = 'cubic_m1'
    c, g = case(name), geo(name)
    for kw in ROUTES.values():
        setup(ctx, c)
        ctx.mbis_iterate(2)
        N, sg, _ = ctx.mbis_params()
        # the same setup with a bound below max |rho|: the parameters of two iterations as the start
        setup(ctx, c, N=N, sigma=sg, bound=0.5 * c.bound)
        for iters in (1, 2, 5):
            assert code(lambda: ctx.mbis_iterate(iters, **kw)) == _lib.XB_E_ARG
            same_bits(ctx.mbis_params()[0], N, f'the populations after a refused call of {iters}')
            same_bits(ctx.mbis_params()[1], sg, f'the widths after a refused call of {iters}')
        assert 'rho_bound' in _lib.load().xb_last_error().decode()
        assert code(lambda: ctx.mbis_iterate(1, keep=True, **kw)) == _lib.XB_E_ARG
        # a bound that holds: the call after the refused ones gives what it gives alone
        ctx.upload_density(c.rho * 0.25)
        q, v, r, st = ctx.mbis_iterate(1, **kw)
        assert st['beyond_bound'] == 0
        e = exponents(0.5 * c.bound, g.count.max(), c.r_cut.max(), g.N)
        rows, pars = run(g, Table(table(), J), c.shells, c.rho * 0.25, N, sg, 0.5 * c.bound, e, 1)
        same_rows((q, v, r), rows, 'the iteration after a refused call')
        same_bits(ctx.mbis_params()[0], pars[0][0], 'the iteration after a refused call')


def test_error_codes(ctx):
    c = case('three')
    A, S, L = _lib.XB_E_ARG, _lib.XB_E_STATE, _lib.XB_E_LIMIT
    E = table()
    x = _lib.Context(0)

    def make(lattice=c.lattice, atoms=c.atoms, r_cut=c.r_cut, shells=c.shells, E=E, J=J, N=c.N0, sigma=c.s0, bound=c.bound, vv=VV):
        return x.mbis_setup(lattice, atoms, r_cut, shells, E, J, N, sigma, bound, vv)

    try:
        assert code(make) == S                                                                  # no grid
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        assert code(lambda: x.mbis_iterate(1)) == S and code(lambda: x.mbis_params()) == S      # no setup
        assert code(lambda: x.mbis_field(PRO)) == S
        assert x.lib.xb_mbis_load(x.h, c.N0.ctypes.data_as(_lib._pdbl), c.s0.ctypes.data_as(_lib._pdbl)) == S
        make()
        assert code(lambda: x.mbis_iterate(1)) == S and code(lambda: x.mbis_field(DEF)) == S    # no density
        assert x.mbis_field(PRO).shape == c.shape                                               # (the promolecule reads none)
        x.upload_density(c.rho)
        good = x.mbis_iterate(1)[0]
        N, sg, _ = x.mbis_params()
        bad_E = [E[:-1], np.where(np.arange(E.size) == 5, -1.0, E), np.where(np.arange(E.size) == 5, np.nan, E), np.append(E[:-1], 1e-300)]
        wide = lambda a, fill: np.concatenate([a, np.full((8, 9 - a.shape[1]), fill)], axis=1)      # (nine columns for nine shells)
        for call in ([lambda s=s: make(shells=np.where(np.arange(8) == 3, s, c.shells)) for s in (0, -1)]
                     + [lambda: make(shells=np.where(np.arange(8) == 3, 9, c.shells), N=wide(c.N0, 0.1), sigma=wide(c.s0, 1.0))]
                     + [lambda b=b: make(E=b) for b in bad_E]
                     + [lambda: make(J=0), lambda: make(E=E[:1]),
                        lambda: make(sigma=c.s0 * 0), lambda: make(sigma=-c.s0), lambda: make(sigma=np.where(c.s0 > 0.3, np.nan, c.s0)),
                        lambda: make(N=-c.N0 - 1), lambda: make(N=np.where(c.N0 > 0, np.inf, c.N0)),
                        lambda: make(vv=0.0), lambda: make(vv=-1.0), lambda: make(vv=np.inf), lambda: make(vv=np.nan),
                        lambda: make(bound=0.0), lambda: make(bound=np.inf), lambda: make(bound=np.nan),
                        lambda: make(r_cut=c.r_cut * 0), lambda: make(atoms=c.atoms * np.nan), lambda: make(lattice=c.lattice * 0),
                        lambda: x.mbis_iterate(0), lambda: x.mbis_iterate(-3),
                        lambda: x.mbis_iterate(2, keep=True), lambda: x.mbis_iterate(_lib.XB_MBIS_ITERS_MAX, keep=True)]):
            assert code(call) == A
        assert code(lambda: make(r_cut=c.r_cut * 1e4)) == L
        assert code(lambda: x.mbis_iterate(_lib.XB_MBIS_ITERS_MAX + 1)) == L
        lib = x.lib
        q, v, r = np.zeros(8, np.int64), np.zeros(8, np.int64), np.zeros(2, np.int64)
        pq, pv, pr = (a.ctypes.data_as(_lib._pi64) for a in (q, v, r))
        assert lib.xb_mbis_iterate(x.h, 1, 8, pq, pv, pr, None) == A                               # an unknown flag bit
        assert lib.xb_mbis_iterate(x.h, 1, 0, None, pv, pr, None) == A and lib.xb_mbis_iterate(x.h, 1, 0, pq, pv, None, None) == A
        assert lib.xb_mbis_params(x.h, None, None, None) == A
        assert lib.xb_mbis_load(x.h, None, None) == A
        assert lib.xb_mbis_field(x.h, 2, 0, None, None) == A and lib.xb_mbis_field(x.h, PRO, 0, None, None) == A
        assert lib.xb_mbis_field(x.h, PRO, 2, np.zeros(27).ctypes.data_as(_lib._pdbl), None) == A
        # a table beyond 2^26 knots and more atoms than any setup holds: refused before anything is sized by them or read
        lat9, at3, rc8 = np.ascontiguousarray(c.lattice), np.ascontiguousarray(c.atoms), np.ascontiguousarray(c.r_cut)
        sh8, info = np.ascontiguousarray(c.shells), (C.c_int64 * 6)()
        pd = lambda a: a.ctypes.data_as(_lib._pdbl)
        M = int(sh8.max())
        N0, s0 = np.ascontiguousarray(c.N0), np.ascontiguousarray(c.s0)
        assert N0.shape == (8, M)
        for n, KE in ((8, (1 << 26) + 1), (1 << 40, E.size - 1), ((1 << 23) + 1, E.size - 1)):
            assert lib.xb_mbis_setup(x.h, pd(lat9), pd(at3), n, pd(rc8), sh8.ctypes.data_as(C.c_void_p), pd(E), J, KE, pd(N0), pd(s0),
                                     1.0, 1.0, info) == L
        assert lib.xb_mbis_setup(x.h, pd(lat9), pd(at3), 0, pd(rc8), sh8.ctypes.data_as(C.c_void_p), pd(E), J, E.size - 1, pd(N0), pd(s0),
                                 1.0, 1.0, info) == A
        # every refused call left the setup alone
        same_bits(x.mbis_params()[0], N, 'the populations after the refused calls')
        same_bits(x.mbis_params()[1], sg, 'the widths after the refused calls')
        make()
        assert np.array_equal(x.mbis_iterate(1)[0], good)
        # a new shape clears it
        x.set_grid((4, 3, 3), np.zeros(27), np.zeros(9))
        assert code(lambda: x.mbis_iterate(1)) == S and code(lambda: x.mbis_field(PRO)) == S
        # a slab of the same shape: refused, and fine again on the whole grid; the block is the Hirshfeld setup's and goes with it
        c2 = case('cubic_m1')
        x.hirshfeld_release()
        x.set_grid(c2.shape, np.zeros(27), np.zeros(9))
        x.upload_density(c2.rho)
        before = x.memory_stats()
        x.mbis_setup(c2.lattice, c2.atoms, c2.r_cut, c2.shells, E, J, c2.N0, c2.s0, c2.bound, VV)
        after = x.memory_stats()
        n, M, nb = 8, 1, 3
        n_img = _lib.hirshfeld_images(c2.lattice, c2.atoms, np.arange(n), c2.r_cut).shape[0]
        words = 16 + 3 * sum(c2.shape) + 3 * n
        words += words & 1
        words += 2 * n + 4 * n_img + 2 * n + 3
        words += words & 1
        words += 2 * (E.size - 1) + 8 * n * M + n + (n * nb + 2) + _lib.XB_MBIS_ITERS_MAX * (2 * n + 2) + 1 + (n + 1) // 2
        assert after[2] - before[2] == 8 * words
        good2 = x.mbis_iterate(2)[0]
        x.set_grid(c2.shape, np.zeros(27), np.zeros(9), (2, 9))
        for call in (lambda: x.mbis_iterate(1), lambda: x.mbis_params(), lambda: x.mbis_field(PRO),
                     lambda: x.mbis_setup(c2.lattice, c2.atoms, c2.r_cut, c2.shells, E, J, c2.N0, c2.s0, c2.bound, VV)):
            assert code(call) == S
        x.set_grid(c2.shape, np.zeros(27), np.zeros(9))
        x.upload_density(c2.rho)
        rows = reference('cubic_m1')[1]
        assert np.array_equal(np.concatenate([good2, x.mbis_iterate(1)[0]]), np.array([row[0] for row in rows[:3]]))
        x.hirshfeld_release()
        assert x.memory_stats()[2] == before[2] and code(lambda: x.mbis_iterate(1)) == S
    finally:
        x.close()


def test_setups_of_the_three_kinds_replace_and_refuse_one_another(ctx):
    c, h = case('three'), hs_case('three')
    S = _lib.XB_E_STATE
    rows = reference('three')[1]
    x = ctx
    x.set_grid(c.shape, np.zeros(27), np.zeros(9))
    x.upload_density(c.rho)

    def mbis_calls():
        return (lambda: x.mbis_iterate(1), lambda: x.mbis_params(), lambda: x.mbis_load(c.N0, c.s0), lambda: x.mbis_field(PRO))

    def isa_load():      # (the library's own answer: the binding would check the shape against its last ISA setup first)
        ones = np.ones((8, 4))
        _lib.check(x.lib.xb_isa_load(x.h, ones.ctypes.data_as(_lib._pdbl)))

    def isa_calls():
        return (lambda: x.isa_iterate(1), lambda: x.isa_tables(), isa_load)

    # MBIS: the Hirshfeld and the ISA calls refuse it
    setup(x, c)
    for call in isa_calls() + (lambda: x.hirshfeld_sum(VV), lambda: x.hirshfeld_field(PRO), lambda: x.hirshfeld_field(DEF)):
        assert code(call) == S
    same_rows(x.mbis_iterate(1)[:3], rows[:1], 'after the refused calls')
    # Hirshfeld replaces it: the MBIS calls refuse it
    x.hirshfeld_setup(h.lattice, h.atoms, h.species, h.pro.tables, h.pro.r_cut)
    for call in mbis_calls():
        assert code(call) == S
    alone = x.hirshfeld_field(PRO)
    # ISA replaces that: the MBIS calls refuse it, the Hirshfeld calls serve it as before
    x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, c.bound)
    for call in mbis_calls():
        assert code(call) == S
    q_isa = x.isa_iterate(1)[0]
    x.hirshfeld_sum(VV)
    # MBIS replaces ISA, and gives what it gives alone; then each of the others again
    setup(x, c)
    same_rows(x.mbis_iterate(2)[:3], rows[:2], 'MBIS after ISA')
    x.isa_setup(c.lattice, c.atoms, c.r_cut, 4, c.bound)
    assert np.array_equal(x.isa_iterate(1)[0], q_isa)
    setup(x, c)
    x.hirshfeld_setup(h.lattice, h.atoms, h.species, h.pro.tables, h.pro.r_cut)
    assert np.array_equal(x.hirshfeld_field(PRO), alone)
    x.hirshfeld_release()
    for call in mbis_calls():
        assert code(call) == S


# ---- Bader(mbis_flag=True) ------------------------------------------------------------------------------------------------------
def _host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


@pytest.mark.parametrize('spin', [False, True], ids=['charge', 'charge and spin'])
@pytest.mark.parametrize('on_device', [False, True], ids=['host density', 'device density'])
def test_bader_with_the_flag_equals_mbis_charges(on_device, spin):
    """two unequal atoms at 24^3.  The densities are rounded to multiples of 2^-20, which makes every charge sum of the run without
    the flag exact in any order: its attributes can be compared bit for bit between the two runs"""
    shape, lat = (24, 24, 24), synth.TRICLINIC
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5, 0.0) * 2.0 ** 20) / 2.0 ** 20
    sp_rho = np.round(rho * 3.0 * (synth.hash_noise(shape, 11) - 0.5) * 2.0 ** 20) / 2.0 ** 20     # (|spin| exceeds the charge somewhere)
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
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        on = Bader(density(), lat, atoms, spin_flag=spin, voronoi_flag=True, mbis_flag=True, mbis_shells=2, mbis_r_cut=2.5, mbis_tol=1e-7)
        on()
    new = {'mbis_flag', 'mbis_shells', 'mbis_r_cut', 'mbis_tol', 'mbis_charge', 'mbis_volume', 'mbis_rest', 'mbis_populations',
           'mbis_widths', 'mbis_iterations', 'mbis_converged'} | ({'mbis_spin'} if spin else set())
    assert set(vars(on)) - set(vars(off)) == new, (set(vars(on)) - set(vars(off))) ^ new
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference'):
            continue
        got, want = _host(getattr(on, key)), _host(want)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert got == want, key
    # against mbis_charges alone, and against the restatement run to the same tolerance
    vv = on.voxel_volume
    bound = max(np.abs(rho).max(), np.abs(sp_rho).max()) if spin else np.abs(rho).max()
    assert not spin or bound > np.abs(rho).max()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r = mbis.mbis_charges(rho, lat, atoms - on.voxel_offset, vv, shells=2, r_cut=2.5, tol=1e-7, rho_bound=float(bound) if spin else None)
    same_bits(on.mbis_charge, r.charge, 'mbis_charge')
    same_bits(on.mbis_volume, r.volume, 'mbis_volume')
    same_bits(on.mbis_rest, r.rest, 'mbis_rest')
    same_bits(on.mbis_populations, r.populations, 'mbis_populations')
    same_bits(on.mbis_widths, r.widths, 'mbis_widths')
    assert on.mbis_iterations == r.iterations and on.mbis_converged and r.converged
    g = geometry(shape, lat, atoms - on.voxel_offset, 2.5)
    e = exponents(bound, g.count.max(), 2.5, g.N)
    shells = np.full(2, 2, np.int32)
    N0, s0 = mbis.default_initial(shells)
    rows, pars = run(g, Table(table(), J), shells, rho, N0, s0, bound, e, on.mbis_iterations, vv)
    hist = np.array([results(e, row, vv)[0] for row in rows])
    change = np.abs(np.diff(hist, axis=0)).max(axis=1)
    assert on.mbis_iterations > 3 and change[-1] < 1e-7 and (change[:-1] >= 1e-7).all()
    same_bits(on.mbis_charge, hist[-1], 'mbis_charge against the restatement')
    same_bits(on.mbis_populations, pars[-1][0], 'mbis_populations against the restatement')
    if spin:
        srow = run(g, Table(table(), J), shells, sp_rho, *pars[-1], bound, e, 1, vv)[0][0]
        same_bits(on.mbis_spin, results(e, srow, vv)[0], 'mbis_spin: one kept pass on the converged weights')
    print('Bader', on.atoms_charge.tolist(), 'Voronoi', on.voronoi_charge.tolist(), 'MBIS', on.mbis_charge.tolist(), on.mbis_iterations)

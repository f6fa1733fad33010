"""xb_stockholder_moments and what stands on it (-m gpu) against the numpy restatement of tests/test_stockmom_cpu.py.

The bins and the info are compared with ==: the sums are 64-bit integers, so they are bit-defined whatever the order of the atomics,
and the moments are exact scalings of them.  Each input runs through the three routes -- sums in registers, over the wave and in LDS
(default), one global atomic per pair and bin (XB_STOCKMOM_DIRECT) and the full search (XB_HIRSHFELD_FULL_SEARCH) -- and the inputs
cover the three kinds of setup: Hirshfeld, ISA and MBIS."""
import ctypes as C
import warnings

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

import test_hirshfeld_cpu as hs
import test_mbis_cpu as mb
from pybader_amd import _lib, device, isa, mbis, stockholder, synth
from pybader_amd.interface import Bader
from test_hirshfeld_cpu import candidate_counts, n_tiles
from test_stockmom_cpu import (J, ROWS, SETUPS, VV, bins, exponents, geo, geometry, mbis_term, moments, reference, setup,
                               table_term, want_info)

pytestmark = pytest.mark.gpu
PRO = _lib.XB_HIRSHFELD_PROMOLECULE
ROUTES = {'reduced': {}, 'direct': {'direct': True}, 'full_search': {'full_search': True}}
U = 2.0 ** -53


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


def install(ctx, s, density=True, grid=True):
    """the setup of one input on the context (and its grid and density)"""
    if grid:
        ctx.set_grid(s.shape, np.zeros(27), np.zeros(9))
    if density:
        ctx.upload_density(s.rho)
    c = s.c
    if s.kind == 'hirshfeld':
        ctx.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)
    elif s.kind == 'isa':
        ctx.isa_setup(c.lattice, c.atoms, c.r_cut, c.K, s.bound, s.tables)
    else:
        ctx.mbis_setup(c.lattice, c.atoms, c.r_cut, c.shells, mb.table(), J, c.N0, c.s0, s.bound, VV)


# ---- bins, info and counts: every input through every route ----------------------------------------------------------------------
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('name', list(SETUPS))
def test_bins_equal_the_restatement(ctx, name, route):
    s, g = setup(name), geo(name)
    E, want, beyond, P, _ = reference(name)
    install(ctx, s)
    got, info, stats = ctx.stockholder_moments(s.bound, **ROUTES[route])
    assert info == want_info(name, E), name
    assert got.dtype == np.int64 and got.shape == (g.n, 12)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{name} ({route}): {bad.shape[0]} of {want.size} bins differ, first (atom, bin) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}'
    tiles = n_tiles(s.shape)
    assert stats['candidate_tiles'] + stats['full_tiles'] == tiles
    if route == 'full_search':
        assert stats['full_tiles'] == tiles and stats['max_candidates'] == 0
    elif 'overflow' in name:
        assert stats['candidate_tiles'] == 0 and stats['max_candidates'] > _lib.XB_HIRSHFELD_CAND_MAX
    else:
        assert stats['full_tiles'] == 0 and stats['max_candidates'] <= _lib.XB_HIRSHFELD_CAND_MAX
    if name == 'hs_rows' and route != 'full_search':
        pro = s.c.pro
        assert stats['max_candidates'] == candidate_counts(s.shape, s.lattice, s.atoms, s.species, pro).max() > ROWS
    assert np.array_equal(ctx.download_density(), s.rho), 'the resident density is not written'
    # the results are exact scalings
    m = stockholder.StockholderMoments(got, info, stats, VV)
    same_bits(m.moments, moments(E, want), 'moments')


def test_the_counting_pass_of_a_hirshfeld_setup_runs_once_and_a_call_waits_once(ctx):
    name = 'hs_tric'
    s = setup(name)
    E, want, _, _, _ = reference(name)
    install(ctx, s)
    before = ctx.host_waits()
    first = ctx.stockholder_moments(s.bound)
    assert 1 <= ctx.host_waits() - before <= 3, 'the counts, the bins (and the buffer, when it grows)'
    mem = ctx.memory_stats()
    for kw in ROUTES.values():
        before = ctx.host_waits()
        again = ctx.stockholder_moments(s.bound, **kw)
        assert ctx.host_waits() - before == 1, 'one host wait per call'
        assert np.array_equal(again[0], want) and again[1] == first[1] == want_info(name, E)
    assert ctx.memory_stats() == mem
    # a larger bound: other exponents, the same counts
    E2 = exponents(8 * s.bound, geo(name).count.max(), s.r_cut.max())
    got, info, _ = ctx.stockholder_moments(8 * s.bound)
    assert info == want_info(name, E2) and E2[0] == E[0] - 3
    assert np.array_equal(got, bins(geo(name), s.term, s.rho, 8 * s.bound, E2)[0])
    # on ISA and MBIS setups the counts are the setup's: one wait from the first call on
    for other in ('isa_three', 'mbis_thin'):
        o = setup(other)
        install(ctx, o)
        ctx.stockholder_moments(o.bound)          # (the buffer may grow here)
        install(ctx, o)
        before = ctx.host_waits()
        got, info, _ = ctx.stockholder_moments(o.bound)
        assert ctx.host_waits() - before == 1 and np.array_equal(got, reference(other)[1]) and info == want_info(other, reference(other)[0])


# ---- against the independent kernels ----------------------------------------------------------------------------------------------
def restated_sums(name):
    """xb_hirshfeld_sum's terms rho p_a / P of a table setup, from this restatement's own pairs"""
    s, g = setup(name), geo(name)
    P = reference(name)[3]
    p = np.zeros((g.n, g.N))
    for a, vox, e, d2 in g.images:
        p[a][vox] = p[a][vox] + s.term(a, d2)
    return hs.restated_sums(s.rho, P, p)


@pytest.mark.parametrize('name', ['hs_cubic', 'hs_tric', 'hs_thin', 'hs_twins', 'isa_k16', 'isa_three'])
def test_the_charges_against_xb_hirshfeld_sum(ctx, name):
    """moments[:, 0] against the charge of xb_hirshfeld_sum, another kernel with float atomics.  BOUND: that of
    tests/test_gpu_hirshfeld.py for the float sum against math.fsum of the restated terms, (count + 2) u |terms| vv, plus half a
    quantum of bin 0 per pair of the atom: count[a] 2^-(E0 + 1) vv."""
    s, g = setup(name), geo(name)
    E = reference(name)[0]
    sums = restated_sums(name)
    install(ctx, s)
    got, info, _ = ctx.stockholder_moments(s.bound)
    charge = ctx.hirshfeld_sum(VV)[0]
    m0 = moments(info['E'], got)[:, 0]
    lim = hs.sum_bound(sums['count'], sums['charge_mag'], VV) + g.count * 2.0 ** -(E[0] + 1) * VV
    worst = np.max(np.abs(m0 - charge) / np.maximum(lim, 1e-300))
    print(f'{name}: |moments[:, 0] - charge| uses {worst:.3g} of its bound; charges {charge.round(6).tolist()}')
    assert info['E'] == E and np.all(np.abs(m0 - charge) <= lim)
    assert np.all(np.abs(m0 - sums['charge'] * VV) <= lim), 'and against the fsum of the restated terms'


@pytest.mark.parametrize('name', ['mbis_mixed', 'mbis_negative', 'mbis_thin'])
def test_the_charges_against_a_kept_mbis_pass(ctx, name):
    """moments[:, 0] against the charge of xb_mbis_iterate(1, keep), whose qsum[a] = sum over pairs and shells of
    rint(2^eN rho (t_i / P)) where bin 0 here is the sum over pairs of rint(2^E0 rho (T / P)); eN == E0 for one rho_bound.
    BOUND, written out.  Per pair of an atom with m <= M shells: T = ((0 + t_0) + t_1) + ... carries m - 1 roundings, every
    quotient one, every product with rho one: sum_i rho fl(t_i / P) and rho fl(T / P) differ by at most (M + 3) u |rho T / P| to
    first order (taken with a factor 1 + 2^-40); the m + 1 rints move the two by at most (M + 1) / 2 quanta.  The shares' magnitudes
    sum to mag[a][0] quanta (the restatement's, each within half a quantum of |rho T / P| 2^E0).  Both sides are then scaled: the
    conversion to double and the product with vv carry one u each, 4 u |charge| for the two.  So
      |moments[a][0] - charge[a]| <= vv 2^-E0 [(M + 1) / 2 count[a] + (M + 3) u (1 + 2^-40) (mag[a][0] + count[a] / 2)] + 4 u |charge[a]|."""
    s, g = setup(name), geo(name)
    E, want, _, _, mag = reference(name)
    install(ctx, s)
    got, info, _ = ctx.stockholder_moments(s.bound)
    q, v, r, _ = ctx.mbis_iterate(1, keep=True)
    minfo = {'eN': mb.case_exponents(SETUPS[name][1])[0], 'eV': mb.case_exponents(SETUPS[name][1])[2], 'eR': mb.case_exponents(SETUPS[name][1])[3]}
    assert minfo['eN'] == E[0]
    charge = mbis._results(minfo, VV, q[0], v[0], r[0])[0]
    m0 = moments(info['E'], got)[:, 0]
    M = int(s.c.shells.max())
    mag0 = np.array([float(x) for x in mag[:, 0]])
    lim = VV * 2.0 ** -E[0] * ((M + 1) / 2 * g.count + (M + 3) * U * (1 + 2.0 ** -40) * (mag0 + g.count / 2)) + 4 * U * np.abs(charge)
    worst = np.max(np.abs(m0 - charge) / np.maximum(lim, 1e-300))
    print(f'{name}: |moments[:, 0] - charge| uses {worst:.3g} of its bound; charges {charge.round(6).tolist()}')
    assert np.array_equal(got, want) and np.all(np.abs(m0 - charge) <= lim)


# ---- state and inputs -----------------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing(ctx):
    """parameters, tables and the resident density are bit-identical before and after; the calls that follow give what they gave"""
    # MBIS: the parameters, a kept pass, the field, then the iteration
    s = setup('mbis_mixed')
    install(ctx, s)
    kept = ctx.mbis_iterate(1, keep=True)[:3]
    field = ctx.mbis_field(PRO)
    for kw in ROUTES.values():
        ctx.stockholder_moments(s.bound, **kw)
    N, sg, count = ctx.mbis_params()
    same_bits(N, s.c.N0, 'the populations')
    same_bits(sg, s.c.s0, 'the widths')
    assert np.array_equal(count, geo('mbis_mixed').count) and np.array_equal(ctx.download_density(), s.rho)
    after = ctx.mbis_iterate(1, keep=True)[:3]
    assert all(np.array_equal(x, y) for x, y in zip(kept, after))
    same_bits(ctx.mbis_field(PRO), field, 'the field')
    rows = mb.reference('tric_mixed')[1]
    q, v, r, _ = ctx.mbis_iterate(2)
    assert np.array_equal(q, np.array([w[0] for w in rows[:2]])) and np.array_equal(v, np.array([w[1] for w in rows[:2]]))
    # ISA: the tables, the counts, the field, then the iteration against one from a fresh setup
    s = setup('isa_k16')
    install(ctx, s)
    fresh = ctx.isa_iterate(2)[0]
    install(ctx, s)
    tables, counts = ctx.isa_tables()
    field = ctx.hirshfeld_field(PRO)
    stats = ctx.hirshfeld_sum(VV)[3]
    for kw in ROUTES.values():
        ctx.stockholder_moments(s.bound, **kw)
    t2, c2 = ctx.isa_tables()
    same_bits(t2, tables, 'the tables')
    same_bits(t2, s.tables, 'the tables')
    assert np.array_equal(c2, counts) and np.array_equal(ctx.download_density(), s.rho)
    same_bits(ctx.hirshfeld_field(PRO), field, 'the field')
    assert ctx.hirshfeld_sum(VV)[3] == stats
    assert np.array_equal(ctx.isa_iterate(2)[0], fresh)
    # Hirshfeld: the fields (bit-defined) and the routes of the sum
    s = setup('hs_tric')
    install(ctx, s)
    field = ctx.hirshfeld_field(PRO)
    deform = ctx.hirshfeld_field(_lib.XB_HIRSHFELD_DEFORMATION)
    stats = ctx.hirshfeld_sum(VV)[3]
    for kw in ROUTES.values():
        ctx.stockholder_moments(s.bound, **kw)
    same_bits(ctx.hirshfeld_field(PRO), field, 'P')
    same_bits(ctx.hirshfeld_field(_lib.XB_HIRSHFELD_DEFORMATION), deform, 'rho - P')
    same_bits(field, hs.reference('tric_r3')[0], 'P')
    assert ctx.hirshfeld_sum(VV)[3] == stats and np.array_equal(ctx.download_density(), s.rho)


def test_setups_of_another_kind_between_calls(ctx):
    names = ['hs_three', 'mbis_one', 'isa_three', 'hs_thin', 'mbis_thin', 'isa_one', 'hs_three']
    for name in names:
        s = setup(name)
        install(ctx, s)
        got, info, _ = ctx.stockholder_moments(s.bound)
        assert np.array_equal(got, reference(name)[1]) and info == want_info(name, reference(name)[0]), name
    # on one grid and one density: only the setup changes
    a, b, c = setup('hs_three'), setup('isa_three'), mb.case('three')
    assert a.shape == b.shape == c.shape and np.array_equal(a.rho, b.rho) and np.array_equal(a.rho, c.rho)
    install(ctx, a)
    for _ in range(2):
        install(ctx, b, density=False, grid=False)
        assert np.array_equal(ctx.stockholder_moments(b.bound)[0], reference('isa_three')[1])
        ctx.mbis_setup(c.lattice, c.atoms, c.r_cut, c.shells, mb.table(), J, c.N0, c.s0, c.bound, VV)
        g = geometry(c.shape, c.lattice, c.atoms, np.arange(8), c.r_cut)
        E = exponents(c.bound, g.count.max(), c.r_cut.max())
        want = bins(g, mbis_term(mb.Table(mb.table(), J), c.shells, c.N0, c.s0), c.rho, c.bound, E)[0]
        assert np.array_equal(ctx.stockholder_moments(c.bound)[0], want)
        install(ctx, a, density=False, grid=False)
        assert np.array_equal(ctx.stockholder_moments(a.bound)[0], reference('hs_three')[1])


@pytest.mark.parametrize('f32', [False, True], ids=['float64', 'float32'])
def test_a_device_density_equals_the_host_one(f32):
    name = 'hs_tric'
    s = setup(name)
    E, want, _, _, _ = reference(name, f32)
    rho = s.rho.astype(np.float32) if f32 else s.rho
    rho64 = rho.astype(np.float64)
    x = _lib.default_context()
    x.set_grid(s.shape, np.zeros(27), np.zeros(9))
    dev = x.device_copy(rho)
    args = (s.lattice, s.atoms, s.species, s.c.pro, VV)
    for density in (dev, rho64):
        for kw in ROUTES.values():
            m = stockholder.hirshfeld_moments(density, *args, **kw)
            assert m.info == want_info(name, E) and np.array_equal(m.bins, want)
            same_bits(m.moments, moments(E, want), 'moments')
    assert (E != reference(name)[0] or not np.array_equal(want, reference(name)[1])) == f32
    # ... and for the two other kinds, on the Python layer's own results
    c = mb.case('tric_mixed')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r = mbis.mbis_charges(rho64, c.lattice, c.atoms, VV, shells=c.shells, r_cut=c.r_cut, tol=0.0, max_iter=3)
    host = stockholder.mbis_moments(rho64, c.lattice, c.atoms, r)
    on_dev = stockholder.mbis_moments(dev, c.lattice, c.atoms, r, direct=True)
    assert np.array_equal(host.bins, on_dev.bins) and host.info == on_dev.info and (host.bins[:, 0] != 0).all()
    g = geo('mbis_mixed')
    bound = float(np.abs(rho64).max())
    Em = exponents(bound, g.count.max(), c.r_cut.max())
    assert np.array_equal(host.bins, bins(g, mbis_term(mb.Table(mb.table(), J), c.shells, r.populations, r.widths), rho64, bound, Em)[0])
    ri = isa.isa_charges(rho64, c.lattice, c.atoms, VV, r_cut=2.0, shells=16, tol=0.0, max_iter=3)
    host = stockholder.isa_moments(rho64, c.lattice, c.atoms, ri, VV)
    on_dev = stockholder.isa_moments(dev, c.lattice, c.atoms, ri, VV, full_search=True)
    assert np.array_equal(host.bins, on_dev.bins) and host.info == on_dev.info and (host.bins[:, 0] != 0).all()


def code(call):
    with pytest.raises(_lib.BaderHipError) as e:
        call()
    return e.value.code


def test_a_density_beyond_rho_bound_is_refused_and_the_output_stays(ctx):
    for name in ('hs_tric', 'mbis_mixed', 'isa_k16'):
        s = setup(name)
        install(ctx, s)
        low = 0.5 * s.bound
        beyond = int((np.abs(s.rho) > low).sum())
        assert beyond > 0
        for flags in (0, _lib.XB_STOCKMOM_DIRECT, _lib.XB_HIRSHFELD_FULL_SEARCH):
            out = np.full((s.atoms.shape[0], 12), -77, np.int64)
            info, st = (C.c_int64 * 8)(), (C.c_int64 * 3)()
            assert ctx.lib.xb_stockholder_moments(ctx.h, low, flags, out.ctypes.data_as(_lib._pi64), info, st) == _lib.XB_E_ARG
            assert (out == -77).all(), 'bins_out is untouched'
            assert info[7] == beyond and 'rho_bound' in ctx.lib.xb_last_error().decode()
        assert code(lambda: ctx.stockholder_moments(low)) == _lib.XB_E_ARG
        # the call after the refused ones gives what it gives alone
        got, info, _ = ctx.stockholder_moments(s.bound)
        assert np.array_equal(got, reference(name)[1]) and info['beyond_bound'] == 0
        # a NaN in the density is beyond every bound
        bad = np.array(s.rho)
        bad.reshape(-1)[5] = np.nan
        ctx.upload_density(bad)
        assert code(lambda: ctx.stockholder_moments(s.bound)) == _lib.XB_E_ARG
        ctx.upload_density(s.rho)


def test_error_codes():
    s = setup('hs_three')
    A, S = _lib.XB_E_ARG, _lib.XB_E_STATE
    x = _lib.Context(0)
    try:
        lib = x.lib
        out = np.zeros((8, 12), np.int64)
        po, info, st = out.ctypes.data_as(_lib._pi64), (C.c_int64 * 8)(), (C.c_int64 * 3)()
        assert lib.xb_stockholder_moments(None, 1.0, 0, po, info, st) == A                  # a null context
        assert code(lambda: x.stockholder_moments(1.0)) == S                                # no grid
        x.set_grid(s.shape, np.zeros(27), np.zeros(9))
        assert code(lambda: x.stockholder_moments(1.0)) == S                                # no setup
        install(x, s, density=False)
        assert code(lambda: x.stockholder_moments(1.0)) == S                                # no density
        x.upload_density(s.rho)
        good = x.stockholder_moments(s.bound)[0]
        assert np.array_equal(good, reference('hs_three')[1])
        waits = x.host_waits()
        for bound in (0.0, -1.0, np.inf, -np.inf, np.nan):
            assert code(lambda: x.stockholder_moments(bound)) == A
        assert lib.xb_stockholder_moments(x.h, s.bound, 4, po, info, st) == A               # unknown flag bits
        assert lib.xb_stockholder_moments(x.h, s.bound, 8 | 1, po, info, st) == A
        assert lib.xb_stockholder_moments(x.h, s.bound, 0, None, info, st) == A             # null pointers
        assert lib.xb_stockholder_moments(x.h, s.bound, 0, po, None, st) == A
        assert x.host_waits() == waits, 'every one of these is found before any launch'
        assert lib.xb_stockholder_moments(x.h, s.bound, 0, po, info, None) == 0            # (the statistics may be left out)
        assert np.array_equal(out, good)
        # a slab of the same shape: refused, and fine again on the whole grid
        x.set_grid(s.shape, np.zeros(27), np.zeros(9), (1, 2))
        assert code(lambda: x.stockholder_moments(s.bound)) == S
        x.set_grid(s.shape, np.zeros(27), np.zeros(9))
        x.upload_density(s.rho)
        assert np.array_equal(x.stockholder_moments(s.bound)[0], good)
        # a new shape clears the setup, a release too; what the calls allocated goes with the grid
        x.set_grid((4, 3, 3), np.zeros(27), np.zeros(9))
        x.upload_density(np.ones((4, 3, 3)))
        assert code(lambda: x.stockholder_moments(1.0)) == S
        install(x, s)
        x.hirshfeld_release()
        assert code(lambda: x.stockholder_moments(s.bound)) == S
    finally:
        x.close()


# ---- Bader(stockholder_moments_flag=True) -------------------------------------------------------------------------------------------
def _host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


NEW = ('moments', 'dipole', 'quadrupole', 'r3', 'r4')


@pytest.mark.parametrize('on_device', [False, True], ids=['host density', 'device density'])
def test_bader_with_the_flag_equals_the_module(on_device):
    """two unequal atoms at 24^3, as tests/test_gpu_mbis.py's: Bader(mbis_flag, stockholder_moments_flag) against
    stockholder.mbis_moments on the result of mbis_charges, and the same for the two other kinds"""
    shape, lat = (24, 24, 24), synth.TRICLINIC
    atoms5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
    rho = np.round(synth.synth_density(shape, lat, atoms5, 0.0) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(atoms5, lat)
    ctx = _lib.default_context()

    def dev(a):
        if not on_device:
            return a.copy()
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        ctx.upload_density(a)
        ctx.upload_labels(np.zeros(shape, np.int8))
        return ctx.export_volume(0)          # a library-owned device array holding the density

    pro = hs.synth_proatoms(atoms5, 2.5, 256)
    species = np.arange(2, dtype=np.int32)
    kw = dict(mbis_flag=True, mbis_shells=2, mbis_r_cut=2.5, mbis_tol=1e-7, isa_flag=True, isa_r_cut=2.0, isa_shells=16, isa_tol=1e-4,
              hirshfeld_flag=True, proatoms=pro, species=species)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        off = Bader({'charge': dev(rho)}, lat, atoms, **kw)
        off()
        on = Bader({'charge': dev(rho)}, lat, atoms, stockholder_moments_flag=True, **kw)
        on()
    new = {'stockholder_moments_flag', 'hirshfeld_volume_ratio'} | {f'{k}_{w}' for k in ('hirshfeld', 'isa', 'mbis') for w in NEW}
    assert set(vars(on)) - set(vars(off)) == new, (set(vars(on)) - set(vars(off))) ^ new
    for k in ('hirshfeld', 'isa', 'mbis'):
        for w in NEW + ('volume_ratio',):
            assert not hasattr(off, f'{k}_{w}')
    same_bits(on.mbis_charge, off.mbis_charge, 'the flag changes no charge')
    same_bits(on.mbis_populations, off.mbis_populations, 'the flag changes no parameter')
    vv, at = on.voxel_volume, atoms - on.voxel_offset
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r = mbis.mbis_charges(rho, lat, at, vv, shells=2, r_cut=2.5, tol=1e-7)
    same_bits(on.mbis_populations, r.populations, 'mbis_populations')
    ri = isa.isa_charges(rho, lat, at, vv, r_cut=2.0, shells=16, tol=1e-4)
    for kind, m in (('mbis', stockholder.mbis_moments(dev(rho) if on_device else rho, lat, at, r)),
                    ('isa', stockholder.isa_moments(rho, lat, at, ri, vv)),
                    ('hirshfeld', stockholder.hirshfeld_moments(rho, lat, at, species, pro, vv))):
        assert m.moments.shape == (2, 12) and (m.bins[:, 0] > 0).all(), kind
        same_bits(getattr(on, f'{kind}_moments'), m.moments, f'{kind}_moments')
        same_bits(getattr(on, f'{kind}_dipole'), m.dipole, f'{kind}_dipole')
        same_bits(getattr(on, f'{kind}_quadrupole'), m.quadrupole, f'{kind}_quadrupole')
        same_bits(getattr(on, f'{kind}_r3'), m.r3, f'{kind}_r3')
        same_bits(getattr(on, f'{kind}_r4'), m.r4, f'{kind}_r4')
    free = pro.radial_moment(3)
    same_bits(on.hirshfeld_volume_ratio, stockholder.hirshfeld_moments(rho, lat, at, species, pro, vv).volume_ratio(free), 'hirshfeld_volume_ratio')
    # against the restatement, for the kind whose setup is the caller's own
    g = geometry(shape, lat, at, species, pro.r_cut)
    bound = float(np.abs(rho).max())
    E = exponents(bound, g.count.max(), pro.r_cut.max())
    want = bins(g, table_term(pro, species), rho, bound, E)[0]
    same_bits(on.hirshfeld_moments, moments(E, want, vv), 'hirshfeld_moments against the restatement')
    print('volume ratios', on.hirshfeld_volume_ratio.tolist(), 'MBIS |dipole|', np.linalg.norm(on.mbis_dipole, axis=1).tolist())

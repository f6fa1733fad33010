"""xb_hirshfeld_setup / xb_hirshfeld_sum / xb_hirshfeld_field and what stands on them (-m gpu) against the numpy restatement of
tests/test_hirshfeld_cpu.py.

The fields -- the promolecular density P and the deformation density rho - P -- are compared with == (bit patterns): every value
at a voxel is bit-defined (include/bader_hip.h).  The sums per atom are float atomics in any order and are compared with math.fsum
under the float64 sum bound of sections 13 and 18; test_hirshfeld_cpu.py shows what that bound is worth.  The forced full search
(XB_HIRSHFELD_FULL_SEARCH) is the second implementation: every case runs through both.  Which route the tiles took is asserted
from the call's statistics; test_hirshfeld_cpu.py::test_the_inputs_of_the_gpu_tests_reach_their_routes says why."""
import ctypes as C
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, device, hirshfeld, synth, utils
from pybader_amd.interface import Bader
from test_hirshfeld_cpu import (CAP, CASES, FIELD_CASES, SUM_CASES, VV, candidate_counts, case, n_tiles, reference,
                                reference_sums, restate, restated_sums, sum_bound, synth_proatoms)

pytestmark = pytest.mark.gpu
PRO, DEF = _lib.XB_HIRSHFELD_PROMOLECULE, _lib.XB_HIRSHFELD_DEFORMATION


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


def setup(ctx, c, density=True):
    ctx.set_grid(c.shape, np.zeros(27), np.zeros(9))
    if density:
        ctx.upload_density(c.rho)
    ctx.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)


@functools.lru_cache(maxsize=None)
def kept(name):
    c = case(name)
    return candidate_counts(c.shape, c.lattice, c.atoms, c.species, c.pro)


def check_route(name, stats, forced=False):
    tiles, route = n_tiles(case(name).shape), CASES[name][-1]
    assert stats['candidate_tiles'] + stats['full_tiles'] == tiles, name
    if not forced:
        # exactly the restatement of phase 1: how many tiles overflow, and the longest list
        print(f'{name}: {stats}; the restatement keeps {kept(name).min()} to {kept(name).max()}')
        assert stats['full_tiles'] == int((kept(name) > CAP).sum()) and stats['max_candidates'] == int(kept(name).max()), name
    if forced:
        assert stats == {'candidate_tiles': 0, 'full_tiles': tiles, 'max_candidates': 0}, name
    elif route == 'candidate':
        assert stats['full_tiles'] == 0 and 0 < stats['max_candidates'] <= CAP, name
    elif route == 'overflow':
        assert stats['candidate_tiles'] == 0 and stats['max_candidates'] > CAP, name
    else:
        assert stats['candidate_tiles'] > 0 and stats['full_tiles'] > 0 and stats['max_candidates'] > CAP, name


def check_sums(name, got, s, vv=VV):
    """charge, volume and rest of one call against the restatement's fsum, each under its bound"""
    charge, volume, rest, _ = got
    lim_c, lim_v = sum_bound(s['count'], s['charge_mag'], vv), sum_bound(s['count'], s['volume_mag'], vv)
    worst_c = np.max(np.abs(charge - s['charge'] * vv) / np.maximum(lim_c, 1e-300))
    worst_v = np.max(np.abs(volume - s['volume'] * vv) / np.maximum(lim_v, 1e-300))
    print(f'{name}: the charges use {worst_c:.3f} of their bound, the volumes {worst_v:.3f}; rest {rest.tolist()}')
    assert charge.shape == s['charge'].shape and np.all(np.abs(charge - s['charge'] * vv) <= lim_c), name
    assert np.all(np.abs(volume - s['volume'] * vv) <= lim_v), name
    assert abs(rest[0] - s['rest'][0] * vv) <= sum_bound(s['rest'][1], s['rest_mag'], vv) and rest[1] == s['rest'][1] * vv, name


# ---- the fields -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIELD_CASES)
def test_fields_equal_the_restatement_through_both_routes(ctx, name):
    c = case(name)
    P, _ = reference(name)
    setup(ctx, c)
    rho = c.rho.reshape(-1)
    for full in (False, True):
        same_bits(ctx.hirshfeld_field(PRO, full), P, f'{name} P (full {full}, host output)')
        same_bits(ctx.hirshfeld_field(DEF, full), rho - P, f'{name} rho - P (full {full}, host output)')
        for mode, want in ((PRO, P), (DEF, rho - P)):
            dev = ctx.hirshfeld_field(mode, full, on_device=True)
            assert isinstance(dev, device.DeviceArray) and dev.shape == c.shape and dev.dtype == np.float64
            same_bits(dev.to_host(), want, f'{name} mode {mode} (full {full}, device output)')
    assert np.array_equal(ctx.download_density(), c.rho), 'the resident density is not written'


def test_the_promolecule_needs_no_density(ctx):
    c = case('tric_r2')
    ctx.set_grid((3, 3, 3), np.zeros(27), np.zeros(9))       # (another shape first: the context holds no density of this grid)
    setup(ctx, c, density=False)
    same_bits(ctx.hirshfeld_field(PRO), reference('tric_r2')[0], 'P without a density')
    for call in (lambda: ctx.hirshfeld_field(DEF), lambda: ctx.hirshfeld_sum(VV)):
        with pytest.raises(_lib.BaderHipError) as e:
            call()
        assert e.value.code == _lib.XB_E_STATE


# ---- the sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SUM_CASES)
def test_sums_are_under_the_bound_through_both_routes(ctx, name):
    c = case(name)
    s = reference_sums(name)
    setup(ctx, c)
    got = ctx.hirshfeld_sum(VV)
    check_route(name, got[3])
    check_sums(name, got, s)
    full = ctx.hirshfeld_sum(VV, full_search=True)
    check_route(name, full[3], forced=True)
    check_sums(name + ' (full search)', full, s)
    assert np.array_equal(ctx.download_density(), c.rho), 'the resident density is not written'
    if name.endswith('_r2'):
        assert got[2][1] > 0 and got[2][0] != 0
    if name == 'twins':
        # atoms 3 and 8 are one atom twice: the same terms (test_hirshfeld_cpu.py compares them with ==), summed by float atomics
        # in an order of their own each, so each lies within the bound of the one restated sum
        lim = 2 * sum_bound(s['count'][3], s['charge_mag'][3])
        assert abs(got[0][3] - got[0][8]) <= lim and s['charge'][3] == s['charge'][8]


def test_a_second_density_reuses_the_setup(ctx):
    """the spin after the charge: another density, signed, on the same setup -- and the first one's sums again afterwards"""
    name = 'partial'
    c = case(name)
    setup(ctx, c)
    first = ctx.hirshfeld_sum(VV)
    spin = np.ascontiguousarray(c.rho * (synth.hash_noise(c.shape, 3) - 0.5))
    before = ctx.memory_stats()
    ctx.upload_density(spin)
    s = restated_sums(spin, *reference(name))
    check_sums('spin on ' + name, ctx.hirshfeld_sum(VV), s)
    same_bits(ctx.hirshfeld_field(DEF), spin.reshape(-1) - reference(name)[0], 'the deformation of the second density')
    ctx.upload_labels(np.zeros(c.shape, np.int32))            # (a label upload does not touch the setup either)
    ctx.upload_density(c.rho)
    check_sums(name + ' again', ctx.hirshfeld_sum(VV), reference_sums(name))
    assert ctx.memory_stats() == before
    assert first[3] == ctx.hirshfeld_sum(VV)[3]


def test_a_float32_device_density():
    if torch is None or not torch.cuda.is_available():
        pytest.skip('torch with a GPU is needed for a device tensor')
    name = 'cubic_r3'
    c = case(name)
    rho32 = c.rho.astype(np.float32)
    t = torch.as_tensor(rho32.copy(), device='cuda')
    P, _ = reference(name)
    args = (c.lattice, c.atoms, c.species, c.pro)
    for full in (False, True):
        got = hirshfeld.deformation_density(t, *args, full_search=full)
        assert isinstance(got, device.DeviceArray)
        same_bits(got.to_host(), rho32.astype(np.float64).reshape(-1) - P, f'float32 tensor, full {full}')
        pro = hirshfeld.promolecule(t, *args, full_search=full)
        assert isinstance(pro, device.DeviceArray)
        same_bits(pro.to_host(), P, 'P for a device density')
        check_sums('float32 tensor', hirshfeld.hirshfeld_charges(t, *args, VV, full_search=full), reference_sums(name, True))


def test_the_python_layer_on_a_host_density():
    name = 'tric_r3'
    c = case(name)
    P, _ = reference(name)
    args = (c.lattice, c.atoms, c.species, c.pro)
    ctx = _lib.default_context()
    got = hirshfeld.hirshfeld_charges(c.rho, *args, VV)
    check_sums(name, got, reference_sums(name))
    key = ctx.hirshfeld_key
    assert key is not None
    same_bits(hirshfeld.promolecule(c.rho, *args), P, 'promolecule')
    same_bits(hirshfeld.deformation_density(c.rho, *args), c.rho.reshape(-1) - P, 'deformation_density')
    assert ctx.hirshfeld_key is key, 'the same arguments make no second setup'
    assert hirshfeld.promolecule(c.rho, *args).shape == c.shape
    # another grid and back: the library dropped the setup with the shape, and the layer knows
    other = case('three')
    hirshfeld.promolecule(other.rho, other.lattice, other.atoms, other.species, other.pro)
    same_bits(hirshfeld.promolecule(c.rho, *args), P, 'promolecule after another grid')


def test_a_setup_made_through_the_context_is_not_mistaken_for_the_layers_own():
    """hirshfeld_charges(A), Context.hirshfeld_setup(B), hirshfeld_charges(A): the layer remembers what the library's setup was
    made from, and the context's own method replaces the setup -- so it must forget; the third call answers for A again"""
    a, b = case('tric_r3'), case('twins')
    ctx = _lib.default_context()
    args = (a.lattice, a.atoms, a.species, a.pro)
    check_sums('A', hirshfeld.hirshfeld_charges(a.rho, *args, VV), reference_sums('tric_r3'))
    assert ctx.hirshfeld_key is not None
    ctx.hirshfeld_setup(b.lattice, b.atoms, b.species, b.pro.tables, b.pro.r_cut)
    assert ctx.hirshfeld_key is None
    assert ctx.hirshfeld_sum(VV)[0].shape == (9,)
    got = hirshfeld.hirshfeld_charges(a.rho, *args, VV)
    assert got[0].shape == (8,) and ctx.hirshfeld_key is not None
    check_sums('A after B', got, reference_sums('tric_r3'))
    same_bits(hirshfeld.promolecule(a.rho, *args), reference('tric_r3')[0], 'P of A after B')
    ctx.hirshfeld_release()
    assert ctx.hirshfeld_key is None
    check_sums('A after a release', hirshfeld.hirshfeld_charges(a.rho, *args, VV), reference_sums('tric_r3'))


@pytest.mark.parametrize('name', ['twins', 'more_overflow'])      # (the atoms and pro-atoms of these cases, on another grid)
def test_one_voxel_grids_pin_every_weight_with_equality(ctx, name):
    """On a grid of ONE voxel every sum has one term, so no order is left free: charge[a] == (rho * w_a) * voxel_volume and
    volume[a] == w_a * voxel_volume bit for bit (zeros are added to it exactly on the way: the other lanes, the empty bin, the
    cleared accumulator).  The voxel sits at the origin; moving the atoms moves it through the cell.  This is the card's own
    p_a / P per voxel compared with == -- through both routes, with bins per atom (9 atoms) and per slot (343) -- and the
    duplicated atom of 'twins' gets exactly the bits of its twin."""
    c = case(name)
    rho = np.full((1, 1, 1), 0.7321)
    ctx.set_grid((1, 1, 1), np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    seen = 0
    # (the twins are narrow: most places are taken near them)
    places = {'twins': ([0.739, 0.771, 0.263], [0.74, 0.77, 0.27], [0.70, 0.80, 0.30], [0.78, 0.72, 0.22], [0.65, 0.70, 0.35], [0.5, 0.5, 0.5]),
              'more_overflow': ([0.0, 0.0, 0.0], [0.24, 0.26, 0.25], [0.5, 0.5, 0.5], [0.1, 0.9, 0.6])}[name]
    for frac in places:
        atoms = np.ascontiguousarray(c.atoms - np.array(frac) @ c.lattice)
        P, p = restate((1, 1, 1), c.lattice, atoms, c.species, c.pro)
        assert P[0] > 0
        w = p[:, 0] / P[0]
        ctx.hirshfeld_setup(c.lattice, atoms, c.species, c.pro.tables, c.pro.r_cut)
        for full in (False, True):
            charge, volume, rest, stats = ctx.hirshfeld_sum(VV, full)
            same_bits(charge, (rho[0, 0, 0] * w) * VV, f'{name} at {frac}: charge (full {full})')
            same_bits(volume, w * VV, f'{name} at {frac}: volume (full {full})')
            assert rest.tolist() == [0.0, 0.0]
            if name == 'twins':
                assert charge[3] == charge[8] and volume[3] == volume[8]
                seen += int(charge[3] > 0)
            else:
                assert (w > 0).sum() > 150 and (full or stats['max_candidates'] >= (w > 0).sum())
    assert name != 'twins' or seen >= 4, 'the twins hold a share of the voxel in most places'


# ---- state, memory, errors ------------------------------------------------------------------------------------------------------
def test_the_setup_is_counted_survives_uploads_and_falls_with_the_shape():
    c = case('cubic_r2')
    x = _lib.Context(0)
    try:
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        x.upload_density(c.rho)
        before = x.memory_stats()
        x.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)
        after = x.memory_stats()
        n_img = _lib.hirshfeld_images(c.lattice, c.atoms, c.species, c.pro.r_cut).shape[0]
        S, K, n = c.pro.n_species, c.pro.knots, c.atoms.shape[0]
        words = 16 + 3 * sum(c.shape) + 3 * S
        words += words & 1
        words += 2 * S * K + 4 * n_img + 2 * n + 3
        assert after[2] - before[2] == 8 * words and after[0] - before[0] == after[2] - before[2]
        x.hirshfeld_sum(VV)
        x.hirshfeld_field(PRO)
        x.hirshfeld_setup(c.lattice, c.atoms[:4], c.species[:4], c.pro.tables, c.pro.r_cut)      # (a smaller one fits the buffer)
        assert x.hirshfeld_sum(VV)[0].shape == (4,)
        assert x.memory_stats() == after
        # the same shape again, and a dist_mat: the setup stays
        x.set_grid(c.shape, np.ones(27), np.ones(9))
        x.upload_density(c.rho)
        x.hirshfeld_sum(VV)
        # a slab of the same shape: refused, and fine again on the whole grid
        x.set_grid(c.shape, np.zeros(27), np.zeros(9), (2, 9))
        for call in (lambda: x.hirshfeld_sum(VV), lambda: x.hirshfeld_field(PRO),
                     lambda: x.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        x.upload_density(c.rho)
        x.hirshfeld_sum(VV)
        # another shape with the same number of voxels, then the first again: refused both times until a new setup
        for shape in ((24, 12, 48), c.shape, (5, 6, 7), c.shape):
            x.set_grid(shape, np.zeros(27), np.zeros(9))
            x.upload_density(np.ones(shape))
            for call in (lambda: x.hirshfeld_sum(VV), lambda: x.hirshfeld_field(PRO), lambda: x.hirshfeld_field(DEF)):
                with pytest.raises(_lib.BaderHipError) as e:
                    call()
                assert e.value.code == _lib.XB_E_STATE, shape
        x.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)
        same_bits(x.hirshfeld_field(PRO), reference('cubic_r2')[0], 'a new setup')
        x.hirshfeld_release()
        assert x.memory_stats()[2] == before[2]
        with pytest.raises(_lib.BaderHipError) as e:
            x.hirshfeld_sum(VV)
        assert e.value.code == _lib.XB_E_STATE
        x.hirshfeld_release()                                         # (nothing to free: fine)
    finally:
        x.close()


def test_error_codes():
    c = case('three')
    x = _lib.Context(0)
    try:
        lib, h, arg, state = x.lib, x.h, _lib.XB_E_ARG, _lib.XB_E_STATE
        pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        lat, at, sp = np.ascontiguousarray(c.lattice).reshape(9), c.atoms.copy(), c.species.copy()
        tab, rc = c.pro.tables.copy(), c.pro.r_cut.copy()
        n, S, K = at.shape[0], rc.shape[0], tab.shape[1] - 1

        def do_setup(lat=lat, at=at, sp=sp, n=n, tab=tab, rc=rc, S=S, K=K):
            ptr = lambda a, f: None if a is None else f(a)
            return lib.xb_hirshfeld_setup(h, ptr(lat, pd), ptr(at, pd), ptr(sp, lambda a: a.ctypes.data), n, ptr(tab, pd), ptr(rc, pd), S, K)

        charge, volume, rest = np.full(n, -7.0), np.full(n, -7.0), np.full(2, -7.0)
        out = np.full(c.rho.size, -7.0)
        do_sum = lambda flags=0, a=charge, b=volume, r=rest: lib.xb_hirshfeld_sum(
            h, VV, flags, None if a is None else pd(a), None if b is None else pd(b), None if r is None else pd(r), None)
        # no grid
        assert do_setup() == state and do_sum() == state and lib.xb_hirshfeld_field(h, PRO, 0, out.ctypes.data, None) == state
        # a null context is a null pointer: XB_E_ARG in all of the calls that take one
        assert lib.xb_hirshfeld_setup(None, pd(lat), pd(at), sp.ctypes.data, n, pd(tab), pd(rc), S, K) == arg
        assert lib.xb_hirshfeld_sum(None, VV, 0, pd(charge), pd(volume), pd(rest), None) == arg
        assert lib.xb_hirshfeld_field(None, PRO, 0, out.ctypes.data, None) == arg
        assert lib.xb_hirshfeld_release(None) == arg
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        # no setup
        assert do_sum() == state and lib.xb_hirshfeld_field(h, PRO, 0, out.ctypes.data, None) == state
        # the setup's arguments
        for kw in (dict(lat=None), dict(at=None), dict(sp=None), dict(tab=None), dict(rc=None), dict(n=0), dict(S=0), dict(K=0)):
            assert do_setup(**kw) == arg, kw
        bad = sp.copy(); bad[2] = S
        assert do_setup(sp=bad) == arg
        bad[2] = -1
        assert do_setup(sp=bad) == arg
        for v in (np.nan, np.inf):
            b = lat.copy(); b[4] = v
            assert do_setup(lat=b) == arg
            b = at.copy(); b[1, 2] = v
            assert do_setup(at=b) == arg
            b = rc.copy(); b[0] = v
            assert do_setup(rc=b) == arg
            b = tab.copy(); b[1, 3] = v
            assert do_setup(tab=b) == arg
        assert do_setup(lat=np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1])) == arg           # determinant exactly 0
        for v in (0.0, -1.0):
            b = rc.copy(); b[S - 1] = v
            assert do_setup(rc=b) == arg
        b = tab.copy(); b[0, 5] = -1e-300
        assert do_setup(tab=b) == arg
        b = tab.copy(); b[S - 1, K] = 1e-300
        assert do_setup(tab=b) == arg                                                   # f[s][K] != 0
        b = rc.copy(); b[0] = 1e5
        assert do_setup(rc=b) == _lib.XB_E_LIMIT                                        # more than 2^31 - 1 images
        assert do_sum() == state, 'no setup has been accepted yet'
        assert do_setup() == 0
        # the sum: no density, null pointers, unknown flag bits
        assert do_sum() == state
        assert lib.xb_hirshfeld_field(h, DEF, 0, out.ctypes.data, None) == state
        assert lib.xb_hirshfeld_field(h, PRO, 0, out.ctypes.data, None) == 0 and (out != -7.0).all()
        out[:] = -7.0
        x.upload_density(c.rho)
        assert do_sum(a=None) == arg and do_sum(b=None) == arg and do_sum(r=None) == arg and do_sum(flags=2) == arg
        assert (charge == -7.0).all() and (volume == -7.0).all() and (rest == -7.0).all()
        # the field: an unknown mode, both outputs, neither, unknown flag bits, a host pointer as the device output, a device
        # output that reaches one element past its allocation, one that is not aligned
        dev = device.DeviceArray(x, c.shape, np.float64)
        assert lib.xb_hirshfeld_field(h, 2, 0, out.ctypes.data, None) == arg
        assert lib.xb_hirshfeld_field(h, -1, 0, out.ctypes.data, None) == arg
        assert lib.xb_hirshfeld_field(h, PRO, 0, out.ctypes.data, C.c_void_p(dev.ptr)) == arg
        assert lib.xb_hirshfeld_field(h, PRO, 0, None, None) == arg
        assert lib.xb_hirshfeld_field(h, DEF, 4, out.ctypes.data, None) == arg
        assert lib.xb_hirshfeld_field(h, PRO, 0, None, out.ctypes.data) == arg
        assert lib.xb_hirshfeld_field(h, PRO, 0, None, C.c_void_p(dev.ptr + 8)) == arg
        assert lib.xb_hirshfeld_field(h, PRO, 0, None, C.c_void_p(dev.ptr + 4)) == arg
        assert (out == -7.0).all(), 'a refused call writes nothing'
        assert lib.xb_hirshfeld_release(None) == arg
        # and the calls still work
        assert do_sum() == 0
        check_sums('three', (charge, volume, rest, None), reference_sums('three'))
    finally:
        x.close()


def test_hygiene_the_label_readers_see_what_they_saw_before():
    """xb_charge_sum and xb_laplacian_sum give identical bits before and after the Hirshfeld calls: the density is rounded to
    multiples of 2^-20 so that the charge sums are exact in any order, and the Laplacian's field is bit-defined"""
    c = case('partial')
    x = _lib.Context(0)
    try:
        rho = np.round(c.rho * 2.0 ** 20) / 2.0 ** 20
        labels = (np.arange(rho.size, dtype=np.int32).reshape(c.shape) // 97) % 5
        x.set_grid(c.shape, np.zeros(27), np.zeros(9))
        x.upload_density(rho)
        x.upload_labels(labels)
        before = (x.charge_sum(0.5, 5), x.laplacian_field(c.lattice), x.laplacian_sum(c.lattice, 5, 0.5)[2])
        x.hirshfeld_setup(c.lattice, c.atoms, c.species, c.pro.tables, c.pro.r_cut)
        for full in (False, True):
            x.hirshfeld_sum(VV, full)
            x.hirshfeld_field(PRO, full)
            x.hirshfeld_field(DEF, full, on_device=True)
        after = (x.charge_sum(0.5, 5), x.laplacian_field(c.lattice), x.laplacian_sum(c.lattice, 5, 0.5)[2])
        for b, a in zip(before[0], after[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        assert np.array_equal(x.download_labels(np.int32), labels) and np.array_equal(x.download_density(), rho)
    finally:
        x.close()


# ---- Bader(hirshfeld_flag=True) -------------------------------------------------------------------------------------------------
def _host(a):
    return a.to_host() if isinstance(a, device.DeviceArray) else a


def _same_attributes(on, off, new):
    assert set(vars(on)) - set(vars(off)) == new, (set(vars(on)) - set(vars(off))) ^ new
    for key, want in vars(off).items():
        if key in ('_density', '_file_info', 'density', 'reference'):
            continue
        got, want = _host(getattr(on, key)), _host(want)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        elif isinstance(want, dict):
            assert got == want, key
        else:
            assert got == want, key


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
    pro = synth_proatoms(atoms5, 3.0, 256)
    species = np.array([0, 1])
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
    on = Bader(density(), lat, atoms, spin_flag=spin, voronoi_flag=True, hirshfeld_flag=True, hirshfeld_field=True, proatoms=pro,
               species=species)
    on()
    new = {'hirshfeld_flag', 'hirshfeld_field', 'proatoms', 'species', 'hirshfeld_charge', 'hirshfeld_volume', 'hirshfeld_rest',
           'hirshfeld_stats', 'hirshfeld_deformation'} | ({'hirshfeld_spin'} if spin else set())
    _same_attributes(on, off, new)
    vv = on.voxel_volume
    P, p = restate(shape, lat, atoms, species, pro)
    check_sums('Bader', (on.hirshfeld_charge, on.hirshfeld_volume, on.hirshfeld_rest, None), restated_sums(rho, P, p), vv)
    if spin:
        s = restated_sums(sp_rho, P, p)
        assert np.all(np.abs(on.hirshfeld_spin - s['charge'] * vv) <= sum_bound(s['count'], s['charge_mag'], vv))
    assert isinstance(on.hirshfeld_deformation, device.DeviceArray if on_device else np.ndarray)
    same_bits(_host(on.hirshfeld_deformation), rho.reshape(-1) - P, 'hirshfeld_deformation')
    assert on.hirshfeld_stats['full_tiles'] == 0
    print('Bader', on.atoms_charge.tolist(), 'Voronoi', on.voronoi_charge.tolist(), 'Hirshfeld', on.hirshfeld_charge.tolist())
    # without hirshfeld_field no field is kept; without pro-atoms the step says what it needs
    lean = Bader(density(), lat, atoms, hirshfeld_flag=True, proatoms=pro, species=species)
    lean()
    assert not hasattr(lean, 'hirshfeld_deformation') and not hasattr(lean, 'hirshfeld_spin')
    assert np.all(np.abs(lean.hirshfeld_charge - on.hirshfeld_charge) <= 2 * sum_bound(*[restated_sums(rho, P, p)[k] for k in ('count', 'charge_mag')], vv))
    with pytest.raises(ValueError):
        Bader(density(), lat, atoms, hirshfeld_flag=True)()

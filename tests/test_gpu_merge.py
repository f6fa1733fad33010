"""xb_merge_basins and what stands on it (-m gpu) against the numpy restatement of tests/test_merge_cpu.py, on the shapes,
densities, label maps and lattices of tests/test_gpu_adjacency.py.  Roots, rounds and targets are integers, saddles are maxima
of existing doubles and the persistence is one float64 subtraction: every comparison is `==` (bitwise for the persistence),
nothing has a tolerance -- except the total of the charge sums, which is held to the rounding bound of a float64 sum."""
import ctypes as C
import math

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, adjacency, device, merge, synth, utils
from pybader_amd.interface import Bader
from test_gpu_adjacency import INTS, LATTICES, SHAPES, densities, directions, label_maps
from test_merge_cpu import TOLS, cases, expected, maxima_of, reference_merge

pytestmark = pytest.mark.gpu
INF = np.inf


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same(got, want, what=''):
    """got: Context.merge_basins' tuple; want: reference_merge's dict"""
    root, rnd, pers, rounds, left, converged = got
    assert root.dtype == np.int32 and rnd.dtype == np.int32 and pers.dtype == np.float64, what
    assert np.array_equal(root, want['root']), what
    assert np.array_equal(rnd, want['merge_round']), what
    assert np.array_equal(pers.view(np.uint64), want['merge_persistence'].view(np.uint64)), what
    assert (rounds, left, converged) == (want['rounds'], want['n_survivors'], want['converged']), what


# ---- against reference_merge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_merge(ctx, shape):
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    up_d = up_m = None
    for dname, mname, lname in cases(shape):
        rho, lab, n, dirs, max_idx, per_tol = expected(shape, dname, mname, lname)
        if dname != up_d:
            ctx.upload_density(rho)
            up_d, up_m = dname, None
        if mname != up_m:
            ctx.upload_labels(lab)
            up_m = mname
        for tname in TOLS:
            tol, want = per_tol[tname]
            got = ctx.merge_basins(dirs, max_idx, tol)
            what = f'{shape} {dname} / {mname} / {lname} / {tname} n {n}'
            print(what, ':', got[4], 'survivors after', got[3], 'rounds')
            same(got, want, what)
            if tname == 'zero':
                assert got[4] == n and got[3] == 1
        if mname == 'two halves':
            assert per_tol['inf'][1]['n_survivors'] == 1, 'two labels that touch: one is above the other'
    # nothing resident was written
    assert np.array_equal(ctx.download_labels(np.int32), lab)
    assert np.array_equal(ctx.download_density().view(np.uint64), rho.view(np.uint64))


def test_max_rounds_stops_the_loop(ctx):
    shape, dname, mname, lname = (12, 10, 14), 'smooth', 'every voxel its own label', 'tric'
    rho, lab, n, dirs, max_idx, per_tol = expected(shape, dname, mname, lname)
    assert per_tol['inf'][1]['rounds'] >= 3
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    ctx.upload_labels(lab)
    for max_rounds in (1, 2):
        want = reference_merge(rho, lab, n, dirs, max_idx, INF, max_rounds)
        assert not want['converged'] and want['rounds'] == max_rounds
        same(ctx.merge_basins(dirs, max_idx, INF, max_rounds), want)


# ---- the buffer: reuse, bookkeeping ---------------------------------------------------------------------------------------------------
def test_another_n_reuses_the_buffer_and_release_frees_it():
    c = _lib.Context(0)
    try:
        shape, dname, lname = (12, 10, 14), 'signed', 'tric'
        big = expected(shape, dname, 'every voxel its own label', lname)
        small = expected(shape, dname, 'random, 3 labels', lname)
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(big[0])
        c.upload_labels(small[1])
        before = c.memory_stats()
        c.enable_timing(only=[_lib.XB_TIMER_MERGE])
        c.kernel_time_reset()
        for rho, lab, n, dirs, max_idx, per_tol in (small, big, small, big):
            c.upload_labels(lab)
            for tname in ('mid', 'inf'):
                same(c.merge_basins(dirs, max_idx, per_tol[tname][0]), per_tol[tname][1], f'n {n} {tname}')
        ms, launches = c.kernel_time(_lib.XB_TIMER_MERGE)
        assert launches >= 8 and ms > 0.0 and c.kernel_time(_lib.XB_TIMER_ADJACENCY) == (0.0, 0)
        c.enable_timing(False)
        held = c.memory_stats()
        assert held[2] - before[2] == 44 * big[2] and held[0] - before[0] == held[2] - before[2], '44 bytes per label, counted'
        c.merge_release()
        assert c.memory_stats() == before
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        a, b, p = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3)
        assert c.lib.xb_merge_fetch(c.h, ptr(a), ptr(b), ptr(p), 3) == _lib.XB_E_STATE, 'the release drops the result'
        rho, lab, n, dirs, max_idx, per_tol = small
        c.upload_labels(lab)
        same(c.merge_basins(dirs, max_idx, per_tol['mid'][0]), per_tol['mid'][1])        # the context works on
        c.set_grid((6, 5, 4), np.zeros(27), np.zeros(9))
        assert c.lib.xb_merge_fetch(c.h, ptr(a), ptr(b), ptr(p), 3) == _lib.XB_E_STATE, 'another shape drops buffer and result'
    finally:
        c.close()


# ---- error codes: each found on the host ------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        shape, n = (5, 7, 11), 3
        rho = densities(shape)['smooth']
        lab, _ = label_maps(shape)['random, 3 labels']
        dirs = np.array([(0, 0, 1), (0, 1, 0), (1, 0, 0)], np.int32)
        idx = maxima_of(rho, lab, n)
        nvox = int(np.prod(shape))

        def code(fn, *a):
            with pytest.raises(_lib.BaderHipError) as e:
                fn(*a)
            return e.value.code

        assert code(c.merge_basins, dirs, idx, 1.0) == _lib.XB_E_STATE                     # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        assert code(c.merge_basins, dirs, idx, 1.0) == _lib.XB_E_STATE                     # no density
        c.upload_density(rho)
        assert code(c.merge_basins, dirs, idx, 1.0) == _lib.XB_E_STATE                     # no labels
        c.upload_labels(lab)
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        rounds, left, conv = C.c_int64(-5), C.c_int64(-5), C.c_int(-5)

        def raw(d=dirs, k=3, m=n, mx=idx, tol=1.0, mr=64, out=(rounds, left, conv)):
            return c.lib.xb_merge_basins(c.h, ptr(d), k, m, ptr(mx), tol, mr, *[None if o is None else C.byref(o) for o in out])

        waits = C.c_int64()
        c.lib.xb_host_waits(C.byref(waits))
        w0 = waits.value
        i32 = lambda rows: np.array(rows, np.int32)
        assert raw(m=0) == _lib.XB_E_ARG and raw(m=-2) == _lib.XB_E_ARG                          # n < 1
        assert raw(k=0) == _lib.XB_E_ARG and raw(d=np.zeros((14, 3), np.int32), k=14) == _lib.XB_E_ARG
        assert raw(d=i32([(0, 0, 1), (0, 0, 0)]), k=2) == _lib.XB_E_ARG                          # the null direction
        assert raw(d=i32([(0, 0, 1), (0, 2, 0)]), k=2) == _lib.XB_E_ARG                          # a step of two
        assert raw(d=i32([(0, 1, 1), (1, 0, 0), (0, 1, 1)])) == _lib.XB_E_ARG                    # given twice
        assert raw(d=i32([(0, 1, 1), (1, 0, 0), (0, -1, -1)])) == _lib.XB_E_ARG                  # together with its negative
        assert raw(d=None) == _lib.XB_E_ARG and raw(mx=None) == _lib.XB_E_ARG                    # null pointers
        for k in range(3):
            out = [rounds, left, conv]
            out[k] = None
            assert raw(out=out) == _lib.XB_E_ARG
        assert raw(mr=0) == _lib.XB_E_ARG and raw(mr=-1) == _lib.XB_E_ARG                        # max_rounds < 1
        assert raw(tol=float('nan')) == _lib.XB_E_ARG and raw(tol=-1e-300) == _lib.XB_E_ARG and raw(tol=-INF) == _lib.XB_E_ARG
        for bad in (-1, nvox, 2 ** 40):                                                          # a max_idx outside [0, N)
            mx = idx.copy()
            mx[1] = bad
            assert raw(mx=mx) == _lib.XB_E_ARG
        assert raw(m=2 ** 31) == _lib.XB_E_LIMIT
        assert (rounds.value, left.value, conv.value) == (-5, -5, -5)
        a, b, p = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
        assert c.lib.xb_merge_fetch(c.h, ptr(a), ptr(b), ptr(p), n) == _lib.XB_E_STATE           # no result yet
        c.lib.xb_host_waits(C.byref(waits))
        assert waits.value == w0, 'every bad argument is found before anything is launched or waited for'
        # +inf and the 13 directions of the ABI are fine
        all13 = i32([d for d in np.ndindex(3, 3, 3)]) - 1
        all13 = all13[[tuple(d) > tuple(-d) for d in all13]]
        same(c.merge_basins(all13, idx, INF), reference_merge(rho, lab, n, all13, idx, INF, 64))
        want = reference_merge(rho, lab, n, dirs, idx, INF, 64)
        same(c.merge_basins(dirs, idx, INF), want)
        # fetch: a short capacity, a null pointer, then enough
        assert c.lib.xb_merge_fetch(c.h, ptr(a), ptr(b), ptr(p), n - 1) == _lib.XB_E_ARG
        assert c.lib.xb_merge_fetch(c.h, ptr(a), None, ptr(p), n) == _lib.XB_E_ARG
        assert not a.any() and not p.any()
        big = [np.zeros(n + 4, np.int32), np.zeros(n + 4, np.int32), np.zeros(n + 4)]
        assert c.lib.xb_merge_fetch(c.h, ptr(big[0]), ptr(big[1]), ptr(big[2]), n + 4) == 0
        assert np.array_equal(big[0][:n], want['root']) and np.array_equal(big[1][:n], want['merge_round'])
        # a slab context
        c.set_grid(shape, np.zeros(27), np.zeros(9), (1, 4))
        c.upload_density(rho)
        c.upload_labels(lab)
        assert code(c.merge_basins, dirs, idx, 1.0) == _lib.XB_E_STATE
        # another grid forgets the old density and labels
        c.set_grid((6, 5, 4), np.zeros(27), np.zeros(9))
        assert code(c.merge_basins, dirs, idx, 1.0) == _lib.XB_E_STATE
    finally:
        c.close()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def test_merge_basins_and_apply_on_every_label_dtype():
    shape, dname, mname, lname = (12, 10, 14), 'smooth', 'vacuum, labels beyond n and an absent label', 'tric'
    rho, base, n, dirs, max_idx, per_tol = expected(shape, dname, mname, lname)
    tol, want = per_tol['mid']
    assert 1 < want['n_survivors'] < n
    vox = np.stack(np.unravel_index(max_idx, shape), axis=1)
    for dt in INTS:
        lab = base.astype(np.int64)
        # the largest label that both the dtype and the device's int32 map hold, far above n: it must come back unchanged
        lab[lab == np.iinfo(np.int32).max] = min(np.iinfo(dt).max, np.iinfo(np.int32).max)
        lab = lab.astype(dt)
        m = merge.merge_basins(rho, lab, LATTICES[lname], vox, tol)
        assert np.array_equal(m.root, want['root']) and np.array_equal(m.merge_round, want['merge_round'])
        assert np.array_equal(m.merge_persistence.view(np.uint64), want['merge_persistence'].view(np.uint64))
        assert (m.rounds, m.converged, len(m)) == (want['rounds'], want['converged'], want['n_survivors'])
        assert np.array_equal(m.survivors, np.flatnonzero(want['merge_round'] < 0))
        assert np.array_equal(m.survivors[m.swap], want['root'])
        inside = (lab >= 0) & (lab < n)
        relabelled = np.where(inside, m.swap[np.where(inside, lab, 0)], lab).astype(dt)
        out = lab.copy()
        assert m.apply(out) is out and out.dtype == dt and np.array_equal(out, relabelled), dt
        assert (out[lab < 0] == lab[lab < 0]).all() and (lab < 0).any(), 'labels < 0 stay'
    empty = merge.merge_basins(rho, lab, LATTICES[lname], np.zeros((0, 3), np.int64), tol)
    assert len(empty) == 0 and empty.converged and empty.rounds == 0
    with pytest.raises(ValueError):
        merge.merge_basins(rho, lab, LATTICES[lname], [[0, 0, shape[2]]], tol)


def test_device_arrays():
    if torch is None or not torch.cuda.is_available():
        pytest.skip('torch does not see the GPU')
    shape, dname, mname, lname = (12, 10, 14), 'smooth', 'random, 3 labels', 'tric'
    rho, lab, n, dirs, max_idx, per_tol = expected(shape, dname, mname, lname)
    tol, want = per_tol['inf']
    vox = np.stack(np.unravel_index(max_idx, shape), axis=1)
    drho = torch.as_tensor(rho.copy(), device='cuda')
    dlab = torch.as_tensor(lab.copy(), device='cuda')
    assert device.is_device_array(drho) and device.is_device_array(dlab)
    m = merge.merge_basins(drho, dlab, LATTICES[lname], vox, tol)
    assert np.array_equal(m.root, want['root']) and np.array_equal(m.merge_round, want['merge_round'])
    assert np.array_equal(dlab.cpu().numpy(), lab), 'the map is not written by the merge'
    assert m.apply(dlab) is dlab
    assert np.array_equal(dlab.cpu().numpy(), m.swap[lab].astype(np.int32))
    # a float32 device density: the run of its widened copy (the maxima are those of the widened field)
    rho32 = rho.astype(np.float32)
    wide = rho32.astype(np.float64)
    idx32 = maxima_of(wide, lab, n)
    vox32 = np.stack(np.unravel_index(idx32, shape), axis=1)
    mid = float(np.median(reference_merge(wide, lab, n, dirs, idx32, 0.0, 1)['merge_persistence'][1:]))
    for t in (mid, INF):
        f32 = merge.merge_basins(torch.as_tensor(rho32, device='cuda'), torch.as_tensor(lab.copy(), device='cuda'), LATTICES[lname], vox32, t)
        f64 = merge.merge_basins(wide, lab, LATTICES[lname], vox32, t)
        ref = reference_merge(wide, lab, n, dirs, idx32, t, 64)
        for got in (f32, f64):
            assert np.array_equal(got.root, ref['root']) and np.array_equal(got.merge_round, ref['merge_round'])
            assert np.array_equal(got.merge_persistence.view(np.uint64), ref['merge_persistence'].view(np.uint64))


def test_inside_resident_a_second_call_uploads_nothing(monkeypatch):
    shape, dname, mname, lname = (12, 10, 14), 'smooth', 'slabs of two planes', 'cubic'
    rho, lab, n, dirs, max_idx, per_tol = expected(shape, dname, mname, lname)
    rho, lab = np.ascontiguousarray(rho.copy()), lab.copy()
    vox = np.stack(np.unravel_index(max_idx, shape), axis=1)
    ctx = _lib.default_context()
    calls = []
    for name in ('upload_density', 'upload_labels', 'import_density', 'import_labels'):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    with utils.resident(rho):
        first = merge.merge_basins(rho, lab, LATTICES[lname], vox, per_tol['mid'][0])
        assert sorted(calls) == ['upload_density', 'upload_labels']
        mem = ctx.memory_stats()
        second = merge.merge_basins(rho, lab, LATTICES[lname], vox, per_tol['mid'][0])
        assert sorted(calls) == ['upload_density', 'upload_labels'], 'the second call uploads nothing'
        assert ctx.memory_stats() == mem, 'and allocates nothing'
    for got in (first, second):
        assert np.array_equal(got.root, per_tol['mid'][1]['root'])
    assert lab.flags.writeable and rho.flags.writeable


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
NOISY_TOL = 4e-3      # twice the noise's amplitude: below it lie the ripples of the vacuum, far above it the atoms' maxima


def noisy_cell():
    """the 8-atom synthetic cell at 24^3 with seeded uniform noise of 2e-3 in its vacuum, rounded to multiples of 2^-20 so
    that every charge sum is exact in any order (as tests/test_gpu_adjacency.py does)"""
    shape, lat = (24, 24, 24), synth.CUBIC6
    rho = synth.synth_density(shape, lat)
    rho = rho + np.where(rho < 0.2, 2e-3 * np.random.default_rng(11).random(shape), 0.0)
    return np.round(rho * 2.0 ** 20) / 2.0 ** 20, lat, synth.atoms_cartesian(synth.ATOMS8, lat)


def same_attributes(a, b):
    assert set(vars(a)) == set(vars(b))
    for name, want in vars(b).items():
        if name in ('_density', '_file_info', 'density', 'reference'):
            continue
        got = getattr(a, name)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), name
        else:
            assert got == want, name


@pytest.mark.parametrize('kwargs', [{}, {'fused': False}, {'speed_flag': True}], ids=['fused', 'two calls', 'speed_flag'])
def test_bader_with_the_threshold(kwargs):
    rho, lat, atoms = noisy_cell()
    shape = rho.shape
    plain = Bader({'charge': rho.copy()}, lat, atoms, **kwargs)               # never sets the attribute
    plain()
    off = Bader({'charge': rho.copy()}, lat, atoms, persistence_tol=None, **kwargs)
    off()
    assert set(vars(off)) - set(vars(plain)) == {'persistence_tol'}
    del off.persistence_tol
    same_attributes(off, plain)
    # the unmerged Bader map and the voxels of its maxima, by the steps _run takes before the merge
    keep = Bader({'charge': rho.copy()}, lat, atoms, adjacency_flag=True, **kwargs)
    keep.volumes_init()
    if 'speed_flag' in kwargs:
        keep.bader_calc()
    else:
        keep.bader_calc_refine()
        assert np.array_equal(keep.bader_volumes, plain.bader_volumes)
    vox, unmerged = keep._bader_maxima_voxels, keep.bader_volumes
    n = vox.shape[0]
    on = Bader({'charge': rho.copy()}, lat, atoms, persistence_tol=NOISY_TOL, **kwargs)
    on()
    m = on.bader_merge
    dirs, _ = adjacency.active_directions(lat / 24.0)
    want = reference_merge(rho, unmerged, n, dirs, np.ravel_multi_index(tuple(vox.T), shape), NOISY_TOL, 64)
    print(kwargs, ':', n, 'maxima,', len(m), 'after', m.rounds, 'rounds')
    assert np.array_equal(m.root, want['root']) and np.array_equal(m.merge_round, want['merge_round'])
    assert np.array_equal(m.merge_persistence.view(np.uint64), want['merge_persistence'].view(np.uint64))
    assert 1 < on.bader_maxima.shape[0] == len(m) == want['n_survivors'] < n, 'the maxima drop'
    assert np.array_equal(on._bader_maxima_voxels, vox[m.survivors])
    assert np.array_equal(on.bader_maxima_fractional, keep.bader_maxima_fractional[m.survivors])
    assert on.atoms_charge.shape == (atoms.shape[0],) and np.all(on.atoms_charge > 0)
    assert on.bader_atoms.shape == (len(m),)
    # The merged volumes hold the charge of the unmerged ones.  Each of the L per-label sums adds its count_m doubles within
    # (count_m + 2) u mag_m (the bound of tests/test_gpu_sums.py), over all labels at most (N + 2 L) u mag; the total is taken
    # with math.fsum, which rounds once more: u mag.
    u, nvox, mag = 2.0 ** -53, rho.size, math.fsum(np.abs(rho).reshape(-1)) * on.voxel_volume
    bound = lambda labels: (nvox + 2 * labels + 1) * u * mag
    if 'speed_flag' in kwargs:
        assert not hasattr(on, 'bader_volumes') and not hasattr(on, 'bader_charge')
    else:
        assert np.array_equal(on.bader_volumes, m.apply(unmerged.copy())) and on.bader_volumes.dtype == unmerged.dtype
        assert on.bader_charge.shape == (len(m),)
        assert abs(math.fsum(on.bader_charge) - math.fsum(plain.bader_charge)) <= bound(len(m)) + bound(n)
    assert abs(math.fsum(on.atoms_charge) - math.fsum(plain.atoms_charge)) <= 2 * bound(atoms.shape[0])

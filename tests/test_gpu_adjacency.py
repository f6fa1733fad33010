"""xb_adjacency and what stands on it (-m gpu) against the numpy restatement of tests/test_adjacency_cpu.py.  Facet counts are
integers, the saddle is a maximum of existing doubles and ties go to an index: every comparison is `==`, nothing has a
tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

from pybader_amd import _lib, adjacency, device, synth, utils
from pybader_amd.interface import Bader
from test_adjacency_cpu import AJ_DENSE, CUBIC, TRIC, reference_adjacency, same

pytestmark = pytest.mark.gpu
INTS = (np.int8, np.int16, np.int32, np.int64)
SHAPES = [(5, 7, 11), (12, 10, 14), (16, 8, 8), (1, 9, 6), (2, 3, 64)]
LATTICES = {'cubic': CUBIC, 'tric': TRIC}


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def cell(shape, lname):
    """the cell of a case.  Three of the shapes cut the triclinic test cell into voxels too flat for a 26-neighbour stencil
    (voronoi_areas raises on them, as documented); there the cell is the one whose voxels are those of the (5, 7, 11) grid:
    the same angles, the same seven active directions."""
    lat = LATTICES[lname]
    if lname == 'tric' and shape in ((16, 8, 8), (1, 9, 6), (2, 3, 64)):
        lat = lat / np.array([5.0, 7.0, 11.0])[:, None] * np.array(shape, float)[:, None]
    return lat


@functools.lru_cache(maxsize=None)
def directions(shape, lname):
    dirs, areas = adjacency.active_directions(cell(shape, lname) / np.array(shape, float)[:, None])
    assert len(dirs) == (7 if lname == 'tric' else 3)
    return dirs, areas


@functools.lru_cache(maxsize=None)
def densities(shape):
    smooth = synth.synth_density(shape, CUBIC)
    three = np.ascontiguousarray(np.round(smooth / smooth.max() * 2.0))          # 0, 1, 2: ties everywhere
    assert len(np.unique(three)) <= 3
    rng = np.random.default_rng(5)
    signed = np.ascontiguousarray(smooth - np.median(smooth)) * rng.choice([1.0, -1.0], shape)
    signed.reshape(-1)[::7] = -0.0
    signed.reshape(-1)[3::11] = 0.0
    out = {'smooth': smooth, 'three values': three, 'signed': signed}
    for a in out.values():
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def label_maps(shape):
    """name -> (map, [n, ...])"""
    nvox = int(np.prod(shape))
    p0, p1, p2 = np.indices(shape)
    rng = np.random.default_rng(17)
    big = rng.integers(0, AJ_DENSE + 1, shape)
    holes = rng.integers(0, 6, shape)
    holes[holes == 4] = 5                                              # a label nobody carries
    r = rng.random(shape)
    holes[r < 0.15] = -1
    holes[(r >= 0.15) & (r < 0.25)] = 6                                # labels >= n
    holes[(r >= 0.25) & (r < 0.30)] = np.iinfo(np.int32).max
    maps = {
        'two halves': (np.where(2 * p2 >= shape[2], 1, 0) if shape[0] < 4 else np.where(2 * p0 >= shape[0], 1, 0), [2]),
        'slabs of two planes': (p0 // 2 if shape[0] >= 4 else p1 // 2, [max(shape) // 2 + 1]),
        'runs of five along z': (p2 // 5, [shape[2] // 5 + 1]),
        'random, 3 labels': (rng.integers(0, 3, shape), [3]),
        'random, both sides of the dense limit': (big, [AJ_DENSE, AJ_DENSE + 1]),
        'every voxel its own label': (np.arange(nvox).reshape(shape), [nvox]),
        'vacuum, labels beyond n and an absent label': (holes, [6]),
    }
    out = {}
    for name, (lab, ns) in maps.items():
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        lab.flags.writeable = False
        out[name] = (lab, ns)
    return out


def setup(ctx, shape, rho, lab=None, x_range=None):
    ctx.set_grid(shape, np.zeros(27), np.zeros(9), x_range)
    ctx.upload_density(rho)
    if lab is not None:
        ctx.upload_labels(lab)


# ---- against reference_adjacency ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_adjacency(ctx, shape):
    assert AJ_DENSE >= 3
    for dname, rho in densities(shape).items():
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        ctx.upload_density(rho)
        for mname, (lab, ns) in label_maps(shape).items():
            ctx.upload_labels(lab)
            for lname in LATTICES:
                dirs, areas = directions(shape, lname)
                per_n = {}
                for n in ns:
                    want = reference_adjacency(rho, lab, n, dirs)
                    got = ctx.adjacency(dirs, n)
                    what = f'{shape} {dname} / {mname} / {lname} n {n}'
                    print(what, ':', len(got[0]), 'pairs')
                    same(got, want)
                    per_n[n] = got
                if AJ_DENSE in per_n:
                    # the same map through the dense and the hashed route: the pairs below the limit agree entry by entry
                    d, h = per_n[AJ_DENSE], per_n[AJ_DENSE + 1]
                    keep = h[0][:, 1] < AJ_DENSE
                    same(d, [x[keep] for x in h])
                if mname == 'two halves':
                    assert got[0].tolist() == [[0, 1]]
                if mname.startswith('every voxel'):
                    # the most pairs a grid can hold: every facet counts, and is a pair of its own unless two voxels meet
                    # more than once through a short axis
                    if min(shape) > 1:
                        assert got[1].sum() == len(dirs) * int(np.prod(shape))
                    assert got[1].sum() >= len(got[0]) > 0 and (min(shape) < 3 or len(got[0]) == got[1].sum())


def test_area_and_position_are_the_host_expressions():
    shape, lname = (12, 10, 14), 'tric'
    lat = LATTICES[lname]
    rho = densities(shape)['smooth']
    lab, (n,) = label_maps(shape)['runs of five along z']
    off = np.array([0.125, -0.25, 0.0625])
    a = adjacency.adjacency(rho, lab, lat, n, voxel_offset=off)
    dirs, areas = directions(shape, lname)
    want = reference_adjacency(rho, lab, n, dirs)
    same((a.pairs, a.facets, a.saddle_density, a.saddle_facet), want)
    assert np.array_equal(a.dirs, dirs) and np.array_equal(a.areas, areas) and len(dirs) > 3
    area = np.zeros(len(a))
    for k in range(len(dirs)):
        area = want[1][:, k] * areas[k] if k == 0 else area + want[1][:, k] * areas[k]
    assert np.array_equal(a.area, area) and np.all(a.area > 0)
    v = np.stack(np.unravel_index(want[3] // 8, shape), axis=1)
    d = dirs[want[3] % 8].astype(np.int64)
    assert np.array_equal(a.saddle_voxels[:, 0], v) and np.array_equal(a.saddle_voxels[:, 1], (v + d) % np.array(shape))
    vl = lat / np.array(shape, float)[:, None]
    pos = np.empty((len(a), 3))
    for j in range(3):
        c = lat[0, j] * v[:, 0].astype(float) / float(shape[0])
        c = c + lat[1, j] * v[:, 1].astype(float) / float(shape[1])
        c = c + lat[2, j] * v[:, 2].astype(float) / float(shape[2])
        c = c + 0.5 * ((d[:, 0] * vl[0, j] + d[:, 1] * vl[1, j]) + d[:, 2] * vl[2, j])
        pos[:, j] = c + off[j]
    assert np.array_equal(a.saddle_position, pos)
    for (x, y), s, (v0, v1) in zip(a.pairs, a.saddle_density, a.saddle_voxels):
        assert lab[tuple(v0)] != lab[tuple(v1)] and {lab[tuple(v0)], lab[tuple(v1)]} == {x, y}
        assert s == min(rho[tuple(v0)], rho[tuple(v1)])


def test_every_label_dtype_in(ctx):
    shape, lname, n = (5, 7, 11), 'tric', 6
    rho = densities(shape)['smooth']
    dirs, _ = directions(shape, lname)
    setup(ctx, shape, rho)
    base, _ = label_maps(shape)['vacuum, labels beyond n and an absent label']
    for dt in INTS:
        lab = base.astype(np.int64)
        lab[lab == np.iinfo(np.int32).max] = np.iinfo(dt).max        # the largest label the dtype holds, far above n
        lab = lab.astype(dt)
        ctx.upload_labels(lab)
        same(ctx.adjacency(dirs, n), reference_adjacency(rho, lab, n, dirs))


# ---- purity, repeatability ---------------------------------------------------------------------------------------------------------
def test_twice_the_same_and_nothing_resident_is_written(ctx):
    shape, lname = (12, 10, 14), 'tric'
    rho = densities(shape)['signed']
    dirs, _ = directions(shape, lname)
    lab, ns = label_maps(shape)['random, both sides of the dense limit']
    setup(ctx, shape, rho, lab)
    for n in ns + [int(np.prod(shape))]:
        a = ctx.adjacency(dirs, n)
        b = ctx.adjacency(dirs, n)
        same(a, b)
        assert len(a[0]) > 0
        assert np.array_equal(ctx.download_labels(np.int32), lab)
        assert np.array_equal(ctx.download_density().view(np.uint64), rho.view(np.uint64))


# ---- device arrays, residency ---------------------------------------------------------------------------------------------------------
def test_device_array_input():
    if torch is None or not torch.cuda.is_available():
        pytest.skip('torch does not see the GPU')
    shape, lname = (12, 10, 14), 'tric'
    rho = densities(shape)['smooth']
    lab, (n,) = label_maps(shape)['random, 3 labels']
    host = adjacency.adjacency(rho, lab, LATTICES[lname], n)
    drho = torch.as_tensor(rho.copy(), device='cuda')
    dlab = torch.as_tensor(lab.copy(), device='cuda')
    assert device.is_device_array(drho) and device.is_device_array(dlab)
    dev = adjacency.adjacency(drho, dlab, LATTICES[lname], n)
    f32 = adjacency.adjacency(drho.to(torch.float32), dlab.to(torch.int64), LATTICES[lname], n)
    want = reference_adjacency(rho, lab, n, host.dirs)
    for got in (host, dev):
        same((got.pairs, got.facets, got.saddle_density, got.saddle_facet), want)
    same((f32.pairs, f32.facets, f32.saddle_density, f32.saddle_facet),
         reference_adjacency(rho.astype(np.float32).astype(np.float64), lab, n, host.dirs))
    assert np.array_equal(dev.saddle_position, host.saddle_position) and np.array_equal(dev.area, host.area)


def test_inside_resident_a_second_call_uploads_nothing(monkeypatch):
    shape, lname = (12, 10, 14), 'cubic'
    rho = np.ascontiguousarray(densities(shape)['smooth'].copy())
    lab, (n,) = label_maps(shape)['slabs of two planes']
    lab = lab.copy()
    ctx = _lib.default_context()
    calls = []
    for name in ('upload_density', 'upload_labels', 'import_density', 'import_labels'):
        orig = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    with utils.resident(rho):
        first = adjacency.adjacency(rho, lab, LATTICES[lname], n)
        assert sorted(calls) == ['upload_density', 'upload_labels']
        mem = ctx.memory_stats()
        second = adjacency.adjacency(rho, lab, LATTICES[lname], n)
        assert sorted(calls) == ['upload_density', 'upload_labels'], 'the second call uploads nothing'
        assert ctx.memory_stats() == mem, 'and allocates nothing'
    same((first.pairs, first.facets, first.saddle_density, first.saddle_facet),
         (second.pairs, second.facets, second.saddle_density, second.saddle_facet))
    same((first.pairs, first.facets, first.saddle_density, first.saddle_facet), reference_adjacency(rho, lab, n, first.dirs))
    assert lab.flags.writeable and rho.flags.writeable


# ---- error codes, timer, memory --------------------------------------------------------------------------------------------------------
def test_error_codes_and_bookkeeping():
    c = _lib.Context(0)
    try:
        shape, n = (5, 7, 11), 3
        rho = densities(shape)['smooth']
        lab, _ = label_maps(shape)['random, 3 labels']
        dirs = np.array([(0, 0, 1), (0, 1, 0), (1, 0, 0)], np.int32)

        def code(fn, *a):
            with pytest.raises(_lib.BaderHipError) as e:
                fn(*a)
            return e.value.code

        assert code(c.adjacency, dirs, n) == _lib.XB_E_STATE                     # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        assert code(c.adjacency, dirs, n) == _lib.XB_E_STATE                     # no density
        c.upload_density(rho)
        assert code(c.adjacency, dirs, n) == _lib.XB_E_STATE                     # no labels
        c.upload_labels(lab)
        np_ = C.c_int64(-5)
        raw = lambda d, k, m, out=np_: c.lib.xb_adjacency(c.h, None if d is None else d.ctypes.data_as(C.c_void_p), k, m,
                                                          None if out is None else C.byref(out))
        i32 = lambda rows: np.array(rows, np.int32)
        assert raw(dirs, 3, 0) == _lib.XB_E_ARG and raw(dirs, 3, -2) == _lib.XB_E_ARG            # n < 1
        assert raw(dirs, 0, n) == _lib.XB_E_ARG and raw(np.zeros((14, 3), np.int32), 14, n) == _lib.XB_E_ARG
        assert raw(i32([(0, 0, 1), (0, 0, 0)]), 2, n) == _lib.XB_E_ARG                           # the null direction
        assert raw(i32([(0, 0, 1), (0, 2, 0)]), 2, n) == _lib.XB_E_ARG                           # a step of two
        assert raw(i32([(0, 0, 1), (0, -2, 1)]), 2, n) == _lib.XB_E_ARG
        assert raw(i32([(0, 1, 1), (1, 0, 0), (0, 1, 1)]), 3, n) == _lib.XB_E_ARG                # given twice
        assert raw(i32([(0, 1, 1), (1, 0, 0), (0, -1, -1)]), 3, n) == _lib.XB_E_ARG              # together with its negative
        assert raw(None, 3, n) == _lib.XB_E_ARG and raw(dirs, 3, n, None) == _lib.XB_E_ARG       # null pointers
        assert raw(dirs, 3, 2 ** 31) == _lib.XB_E_LIMIT
        assert np_.value == -5
        # the 13 directions of the ABI and negative steps are fine
        all13 = i32([d for d in np.ndindex(3, 3, 3)]) - 1
        all13 = all13[[tuple(d) > tuple(-d) for d in all13]]
        assert all13.shape == (13, 3)
        same(c.adjacency(all13, n), reference_adjacency(rho, lab, n, all13))
        same(c.adjacency(-dirs, n), reference_adjacency(rho, lab, n, -dirs))
        # fetch with a short capacity, then with enough
        before = c.memory_stats()
        c.enable_timing(only=[_lib.XB_TIMER_ADJACENCY])
        c.kernel_time_reset()
        pairs, facets, saddle, sfacet = c.adjacency(dirs, n)
        ms, launches = c.kernel_time(_lib.XB_TIMER_ADJACENCY)
        assert launches >= 1 and ms > 0.0
        assert c.kernel_time(_lib.XB_TIMER_MOMENTS) == (0.0, 0)
        c.enable_timing(False)
        p = len(pairs)
        assert p == 3
        a, b = np.zeros(p, np.int32), np.zeros(p, np.int32)
        f, s, sf = np.zeros((p, 3), np.int64), np.zeros(p), np.zeros(p, np.int64)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        assert c.lib.xb_adjacency_fetch(c.h, ptr(a), ptr(b), ptr(f), ptr(s), ptr(sf), p - 1) == _lib.XB_E_ARG
        assert c.lib.xb_adjacency_fetch(c.h, ptr(a), None, ptr(f), ptr(s), ptr(sf), p) == _lib.XB_E_ARG
        assert not a.any() and not f.any()
        assert c.lib.xb_adjacency_fetch(c.h, ptr(a), ptr(b), ptr(f), ptr(s), ptr(sf), p + 4) == 0
        same((np.stack([a, b], axis=1), f, s, sf), (pairs, facets, saddle, sfacet))
        # the table: counted while it is there, gone after the release
        dense = c.memory_stats()
        assert dense[2] - before[2] >= 0 and dense[2] >= 3 * 5 * 8
        nvox = int(np.prod(shape))
        c.upload_labels(np.arange(nvox, dtype=np.int32).reshape(shape))
        c.adjacency(dirs, nvox)
        hashed = c.memory_stats()
        assert hashed[2] - dense[2] >= 2 * 3 * nvox * 8 and hashed[0] - dense[0] == hashed[2] - dense[2]
        c.adjacency_release()
        after = c.memory_stats()
        assert dense[2] - after[2] >= 3 * 5 * 8 and hashed[2] - after[2] >= 2 * 3 * nvox * 6 * 8
        assert c.lib.xb_adjacency_fetch(c.h, ptr(a), ptr(b), ptr(f), ptr(s), ptr(sf), p) == _lib.XB_E_STATE
        c.upload_labels(lab)
        same(c.adjacency(dirs, n), (pairs, facets, saddle, sfacet))          # the context works on
        # a slab context
        c.set_grid(shape, np.zeros(27), np.zeros(9), (1, 4))
        c.upload_density(rho)
        c.upload_labels(lab)
        assert code(c.adjacency, dirs, n) == _lib.XB_E_STATE
        # another grid forgets the old density and labels, and the table
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        c.upload_labels(lab)
        c.adjacency(dirs, n)
        assert c.memory_stats()[2] > after[2]
        c.set_grid((6, 5, 4), np.zeros(27), np.zeros(9))
        assert code(c.adjacency, dirs, n) == _lib.XB_E_STATE
    finally:
        c.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_bader_with_the_flag():
    """the 8-atom synthetic cell at 24^3, its density rounded to multiples of 2^-20 so that every charge sum is exact in any
    order and the flag-off attributes can be compared bit for bit between two runs (as tests/test_gpu_multipole.py does)"""
    shape, lat = (24, 24, 24), synth.CUBIC6
    rho = np.round(synth.synth_density(shape, lat) * 2.0 ** 20) / 2.0 ** 20
    atoms = synth.atoms_cartesian(synth.ATOMS8, lat)
    off = Bader({'charge': rho.copy()}, lat, atoms)
    off()
    on = Bader({'charge': rho.copy()}, lat, atoms, adjacency_flag=True)
    on()
    new = {'atoms_adjacency', 'atoms_bond_area', 'atoms_bond_density', 'atoms_bond_position', 'bader_adjacency', 'bader_persistence'}
    assert set(vars(on)) - set(vars(off)) == new | {'adjacency_flag', '_bader_maxima_voxels'} and not set(vars(off)) - set(vars(on))
    for name, want in vars(off).items():
        if name in ('_density', '_file_info', 'density', 'reference'):
            continue
        got = getattr(on, name)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and np.array_equal(got, want), name
        else:
            assert got == want, name
    n = atoms.shape[0]
    dirs, areas = adjacency.active_directions(lat / 24.0)
    for adj, lab, m in ((on.atoms_adjacency, on.atoms_volumes, n), (on.bader_adjacency, on.bader_volumes, on.bader_maxima.shape[0])):
        want = reference_adjacency(rho, lab, m, dirs)
        same((adj.pairs, adj.facets, adj.saddle_density, adj.saddle_facet), want)
        assert np.array_equal(adj.area, adjacency.facet_area(want[1], areas))
        voxels, pos = adjacency.saddle_geometry(want[3], dirs, shape, lat, on.voxel_offset)
        assert np.array_equal(adj.saddle_voxels, voxels) and np.array_equal(adj.saddle_position, pos)
    a = on.atoms_adjacency
    assert on.atoms_bond_area is a.area and on.atoms_bond_density is a.saddle_density and on.atoms_bond_position is a.saddle_position
    assert all(len(a.neighbours(i)) >= 1 for i in range(n)), 'each atom is adjacent to at least one other'
    # persistence: by hand from the reference pairs
    vox = on._bader_maxima_voxels
    top = rho[vox[:, 0], vox[:, 1], vox[:, 2]]
    pairs, _, saddle, _ = reference_adjacency(rho, on.bader_volumes, len(top), dirs)
    want = np.full(len(top), np.inf)
    for m in range(len(top)):
        s = [sd for (x, y), sd in zip(pairs.tolist(), saddle.tolist()) if m in (x, y) and top[x + y - m] > top[m]]
        if s:
            want[m] = top[m] - max(s)
    assert np.array_equal(on.bader_persistence, want)
    assert on.bader_persistence[int(np.argmax(top))] == np.inf

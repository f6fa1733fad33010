"""The isosurface kernels (csrc/k_isosurface.h) against the numpy restatement of tests/test_isosurface_cpu.py: counts, triangles,
wrap, cells, vertices and colour with ==, through the tiled and the gather route; area, volume and the per-label volumes against
math.fsum of the restated terms under the bound of tests/test_laplacian_cpu.py; the Euler characteristic of the GPU mesh against
the GPU critical points (an independent kernel); a field other than the density; call history; memory; error codes."""
import ctypes as C
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:         # pragma: no cover
    torch = None

import history_common as H
from pybader_amd import _lib, critical, device, isosurface, nci, synth, thread_handlers, utils
from test_critical_cpu import case
from test_gpu_history import Runner
from test_isosurface_cpu import (LAT, LEVEL_SETS, as_mesh, colour_field, first_difference, levels, restate, restated_case,
                                 sums_difference)
from test_laplacian_cpu import N_LABELS, ST_BINS, SUM_SHAPES
from test_multipole_cpu import LATTICES, density, label_map

pytestmark = pytest.mark.gpu
DEGENERATE = ['synth8', 'noise3', 'noise2', 'noise1x2x9']       # axes below 4 among them: only the == comparison applies
MESH_CASES = LEVEL_SETS + [(name, 'q0.6') for name in DEGENERATE]


def lattice_of(name):
    return LAT.get(name, synth.TRICLINIC)


@functools.lru_cache(maxsize=None)
def restated_any(name, what):
    if name in LAT:
        return restated_case(name, what, True)
    rho = case(name)
    return restate(rho, float(np.quantile(rho, 0.6)), lattice_of(name), colour_field(rho.shape))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gather', [False, True], ids=['tiled', 'gather'])
@pytest.mark.parametrize('name,what', MESH_CASES)
def test_the_mesh_equals_the_restatement(ctx, name, what, gather):
    rho, want = case(name), restated_any(name, what)
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    g = ctx.device_copy(colour_field(rho.shape))
    got = ctx.isosurface(lattice_of(name), want.level, None, g, 0, gather)
    assert first_difference(got, want, f'{name} {what}') is None
    assert sums_difference(got, want, f'{name} {what}') is None
    ctx.isosurface_release()


def test_an_empty_mesh_and_a_full_cell(ctx):
    rho, lat = case('constant'), synth.TRICLINIC
    ctx.set_grid(rho.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    ctx.upload_labels(np.zeros(rho.shape, np.int32))
    for gather in (False, True):
        for level, full in ((0.25, True), (0.5, False)):
            want = restate(rho, level, lat, labels=np.zeros(rho.shape, np.int32), n=1)
            vert, col, tri, wrap, cell, area, volume, vbl = ctx.isosurface(lat, level, None, None, 1, gather)
            assert vert.shape == (0, 3) and col is None and tri.shape == (0, 3) and wrap.shape == cell.shape == (0,) and area == 0.0
            assert volume == want.volume and vbl[0] == want.volume_by_label[0] and (volume > 0) == full
    zs = case('zeros_spike')
    ctx.set_grid(zs.shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(zs)
    for level in (0.0, -0.0):
        out = ctx.isosurface(synth.CUBIC6, level)
        assert out[0].shape[0] == 0 and out[6] == restate(zs, level, synth.CUBIC6).volume > 0
    ctx.isosurface_release()


def same_but_nan(a, b):
    """the same NaNs in the same places, the same bits everywhere else (the payload of a NaN is no part of the definition)"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


@pytest.mark.parametrize('gather', [False, True], ids=['tiled', 'gather'])
@pytest.mark.parametrize('what,value,level', [('nan', float('nan'), 0.5), ('+inf', float('inf'), 2.0), ('-inf', float('-inf'), 0.5)])
def test_a_voxel_that_is_not_finite(ctx, what, value, level, gather):
    """ones with one NaN, +inf or -inf voxel, at a tile's corner and in its middle: a NaN is outside by the plain comparison, t is
    what the one division gives (NaN or 0) -- integers with ==, vertices and colour bit for bit where they are numbers"""
    shape, lat = (9, 10, 35), synth.TRICLINIC
    for at in ((8, 9, 34), (0, 0, 0), (3, 4, 17)):
        rho = np.ones(shape)
        rho[at] = value
        g = colour_field(shape)
        want = restate(rho, level, lat, g)
        assert want.crossing == 14 and want.triangles.shape[0] == 24
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        ctx.upload_density(rho)
        vert, col, tri, wrap, cell, area, volume, _ = ctx.isosurface(lat, level, None, ctx.device_copy(g), 0, gather)
        assert np.array_equal(tri, want.triangles) and np.array_equal(wrap, want.wrap) and np.array_equal(cell, want.cells), (what, at)
        assert same_but_nan(vert, want.vertices) and same_but_nan(col, want.colour), (what, at)
        assert np.isnan(vert).any() and np.isnan(area) == np.isnan(want.area) and np.isnan(volume) == np.isnan(want.volume)
    ctx.isosurface_release()


def test_the_nci_mask_on_values_that_are_not_finite(ctx):
    shape = (5, 6, 7)
    rho = np.full(shape, 0.01)
    rho[1, 2, 3] = 0.5                                         # at or above rho_cut
    s = np.full(shape, 0.25)
    s[0, 0, 0], s[0, 0, 1], s[0, 0, 2], s[0, 0, 3], s[1, 2, 3] = np.inf, np.nan, 100.0, 99.0, 0.1
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    d = ctx.device_copy(s)
    ctx.isosurface_nci_mask(d, 0.05)
    want = s.copy()
    want[0, 0, 0] = want[0, 0, 1] = want[1, 2, 3] = _lib.ISO_NCI_RAISED
    assert np.array_equal(d.to_host(), want)


# ---- the sums ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sum_case(shape, lname, n):
    rho, lab = density(shape), label_map(shape, n)
    return rho, lab, restate(rho, float(np.quantile(rho, 0.4)), LATTICES[lname], labels=lab, n=n)


@pytest.mark.parametrize('n', N_LABELS)
@pytest.mark.parametrize('shape', SUM_SHAPES)
def test_sums_on_both_sides_of_the_lds_limit_through_both_routes(ctx, shape, n):
    assert N_LABELS == [2, ST_BINS, ST_BINS + 1, 3000]
    for lname in LATTICES:
        rho, lab, want = sum_case(shape, lname, n)
        assert want.triangles.shape[0] > 1000 and (want.share_count > 0).sum() >= min(n, 2)
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        ctx.upload_density(rho)
        ctx.upload_labels(lab)
        for gather in (False, True):
            got = ctx.isosurface(LATTICES[lname], want.level, None, None, n, gather)
            what = f'{shape} {lname} n {n} gather {gather}'
            assert first_difference(got, want, what) is None
            assert sums_difference(got, want, what) is None
    ctx.isosurface_release()


# ---- the Euler characteristic against the critical points of the GPU ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['synth40x36x44', 'rough', 'plateau'])
def test_euler_characteristic_is_twice_the_alternating_sum_of_the_gpu_critical_points(name):
    rho = case(name)
    cp = critical.critical_points(rho)
    for what, level in levels(name):
        keep = rho.reshape(-1)[cp.lin] >= level
        full, ring, bond = cp.masks[keep] == _lib.XB_CRITICAL_FULL, cp.ring[keep].astype(np.int64), cp.bond[keep].astype(np.int64)
        alt = int(full.sum() - bond.sum() + ring.sum() - (cp.masks[keep] == 0).sum())
        m = isosurface.isosurface(rho, LAT[name], level)
        assert m.euler == 2 * alt, (name, what)
        assert m.euler == as_mesh(restated_case(name, what), LAT[name]).euler


# ---- a field other than the density ---------------------------------------------------------------------------------------------------
NCI_SHAPE = (24, 20, 28)


@functools.lru_cache(maxsize=None)
def nci_density():
    a = synth.synth_density(NCI_SHAPE)
    a.flags.writeable = False
    return a


def same_mesh(a, b):
    """the bit-defined parts of two meshes agree (area and volume are float atomics in any order: held to the restatement instead)"""
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ('vertices', 'colour', 'triangles', 'wrap', 'cells', 'positions'))


def as_tuple(m):
    return m.vertices, m.colour, m.triangles, m.wrap, m.cells, m.area, m.volume, m.volume_by_label


def test_the_reduced_gradient_on_the_device_coloured_by_sign_lambda2_rho():
    rho, lat = nci_density(), synth.TRICLINIC
    c = _lib.default_context()
    c.set_grid(NCI_SHAPE, np.zeros(27), np.zeros(9))
    rho_dev = c.device_copy(rho)
    s, x = nci.nci_fields(rho_dev, lat)
    assert isinstance(s, device.DeviceArray) and isinstance(x, device.DeviceArray)
    s_host, x_host = s.to_host(), x.to_host()
    level = float(np.quantile(s_host[np.isfinite(s_host)], 0.3))
    want = restate(s_host, level, lat, x_host)
    assert want.triangles.shape[0] > 1000
    for gather in (False, True):
        m = isosurface.isosurface(s, lat, level, colour=x, gather=gather, density=rho_dev)
        got = (m.vertices, m.colour, m.triangles, m.wrap, m.cells, m.area, m.volume, m.volume_by_label)
        assert first_difference(got, want, f'gather {gather}') is None and sums_difference(got, want, f'gather {gather}') is None
    # a host field beside the resident density goes through a scratch upload: the same mesh
    h = isosurface.isosurface(s_host, lat, level, colour=x_host, density=rho)
    assert same_mesh(h, m) and sums_difference(as_tuple(h), want, 'the host field') is None


def test_nci_isosurface_on_the_host_route_equals_the_device_route():
    rho, lat = nci_density(), synth.TRICLINIC
    s_cut, rho_cut = 0.5, 0.3
    a = nci.nci_isosurface(rho, lat, s_cut, rho_cut)
    c = _lib.default_context()
    b = nci.nci_isosurface(c.device_copy(rho), lat, s_cut, rho_cut)
    assert len(a) > 100 and same_mesh(a, b)
    s, x = nci.nci_fields(rho, lat)
    masked = np.where((rho >= rho_cut) | ~(s < _lib.ISO_NCI_RAISED), _lib.ISO_NCI_RAISED, s)
    want = restate(masked, s_cut, lat, x)
    got = (a.vertices, a.colour, a.triangles, a.wrap, a.cells, a.area, a.volume, a.volume_by_label)
    assert first_difference(got, want, 'nci_isosurface') is None and sums_difference(got, want, 'nci_isosurface') is None
    assert sums_difference(as_tuple(b), want, 'nci_isosurface, device route') is None
    assert np.isfinite(a.vertices).all() and ((rho >= rho_cut) & (s < s_cut)).any()      # (the mask removes the nuclei's shells)
    with pytest.raises(ValueError):
        nci.nci_isosurface(rho, lat, _lib.ISO_NCI_RAISED, rho_cut)


def test_a_field_made_on_another_stream_is_ordered_before_the_kernels():
    """a torch tensor filled on a non-blocking stream, handed in inside device.on_stream: the context's stream waits for it"""
    if torch is None or not torch.cuda.is_available():
        pytest.skip('torch sees no device')
    rho, lat = nci_density(), synth.TRICLINIC
    level = float(np.quantile(rho, 0.6))
    want = restate(rho, level, lat, colour_field(rho.shape))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.zeros(1 << 26, device='cuda', dtype=torch.float64)
        for _ in range(8):
            big += 1.0                                          # work queued ahead of the field on the side stream
        f = torch.as_tensor(rho.copy(), device='cuda').contiguous() + big[:rho.size].reshape(rho.shape) * 0.0      # (x + 0.0 is x)
        g = torch.as_tensor(colour_field(rho.shape).copy(), device='cuda').contiguous() + 0.0
        with device.on_stream(side.cuda_stream):
            m = isosurface.isosurface(f, lat, level, colour=g, density=rho)
    assert first_difference(as_tuple(m), want, 'side stream') is None


# ---- call history -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def history_case(grid):
    rho, lab, n = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms')
    return restate(rho, float(np.quantile(rho, 0.7)), H.LAT, colour_field(rho.shape), lab, n)


def iso_call(grid, gather):
    """one isosurface call through the public function on density A and the atom map of a grid of history_common -> None, or
    what differs from the restatement"""
    rho, lab, n, want = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms'), history_case(grid)
    m = isosurface.isosurface(rho, H.LAT, want.level, colour=colour_field(rho.shape), volumes=lab, n=n, gather=gather)
    got = (m.vertices, m.colour, m.triangles, m.wrap, m.cells, m.area, m.volume, m.volume_by_label)
    return first_difference(got, want, f'isosurface on {grid}') or sums_difference(got, want, f'isosurface on {grid}')


@pytest.mark.parametrize('other', sorted(H.KINDS))
def test_call_history_does_not_matter(other, monkeypatch):
    """the isosurface directly before and directly after every other analysis, on G1 -> G2 -> G1 of history_common.GRIDS and inside
    utils.resident(), on the default context: both sides' results are unchanged (the per-voxel words live in the shared scratch)"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    run = Runner()
    bad = []
    try:
        for grid in ('G1', 'G2', 'G1'):
            for step in (lambda: iso_call(grid, False), lambda: run.checked(other, grid, 'A', 'atoms'), lambda: iso_call(grid, False),
                         lambda: run.checked(other, grid, 'A', 'atoms'), lambda: iso_call(grid, True)):
                msg = step()
                if msg:
                    bad.append(f'{grid}: {msg}')
        with utils.resident(H.density('G1', 'A')):
            for step in (lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: iso_call('G1', False),
                         lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: iso_call('G1', False)):
                msg = step()
                if msg:
                    bad.append(f'resident(A): {msg}')
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, ' | '.join(bad[:4])


def test_the_mesh_is_counted_and_released():
    name, what = 'rough', 'q0.6'
    rho, want = case(name), restated_case(name, what, True)
    V, T = want.vertices.shape[0], want.triangles.shape[0]
    c = _lib.Context(0)
    try:
        c.set_grid(rho.shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        g = c.device_copy(colour_field(rho.shape))
        before = c.memory_stats()
        c.isosurface(LAT[name], want.level)
        after = c.memory_stats()
        assert after[2] - before[2] == 24 * V + 34 * T and after[0] - before[0] == after[2] - before[2]
        c.isosurface(LAT[name], want.level, None, g)
        assert c.memory_stats()[2] - before[2] == 32 * V + 34 * T
        c.isosurface(LAT[name], 2.0 * float(rho.max()))                          # an empty mesh: one element per array
        assert c.memory_stats()[2] - before[2] == 24 + 34
        c.isosurface_release()
        assert c.memory_stats() == before
        c.isosurface_release()                                                  # (twice is fine)
        # any writer of the density discards the kept result
        counts = c.isosurface(LAT[name], want.level)
        c.upload_density(rho)
        with pytest.raises(_lib.BaderHipError) as e:
            c.isosurface_fetch(counts[0].shape[0], counts[2].shape[0])
        assert e.value.code == _lib.XB_E_STATE
        # ... and so does handing out the density's pointer: whoever holds it may write
        counts = c.isosurface(LAT[name], want.level)
        assert c.isosurface_fetch(counts[0].shape[0], counts[2].shape[0])[2].shape[0] == T
        assert c.lib.xb_density_ptr(c.h)
        with pytest.raises(_lib.BaderHipError) as e:
            c.isosurface_fetch(counts[0].shape[0], counts[2].shape[0])
        assert e.value.code == _lib.XB_E_STATE
    finally:
        c.close()


# ---- error codes --------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        shape = (8, 8, 8)
        rho, lat = case('synth8'), synth.CUBIC6
        level = float(np.quantile(rho, 0.6))
        state, arg, limit = _lib.XB_E_STATE, _lib.XB_E_ARG, _lib.XB_E_LIMIT
        lib, h = c.lib, c.h
        lp = (C.c_double * 9)(*np.asarray(lat, dtype=np.float64).reshape(-1))
        flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)          # a singular lattice
        counts = (C.c_int64 * 2)(-7, -7)
        assert lib.xb_isosurface(h, None, None, lp, level, 0, 0, counts) == state              # no grid
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        assert lib.xb_isosurface(h, None, None, lp, level, 0, 0, counts) == state              # no density
        c.upload_density(rho)
        assert lib.xb_isosurface(h, None, None, lp, level, 2, 0, counts) == state              # no labels with n >= 1
        sc = (C.c_double * 2)()
        one = np.zeros(8)
        assert lib.xb_isosurface_fetch(h, 0, one.ctypes.data, None, one.ctypes.data, one.ctypes.data, one.ctypes.data, 0, 0, sc, None, 0) == state
        c.upload_labels(np.zeros(shape, np.int32))
        d, e = device.DeviceArray(c, shape, np.float64), device.DeviceArray(c, shape, np.float64)
        vd, ve = C.c_void_p(d.ptr), C.c_void_p(e.ptr)
        assert lib.xb_isosurface(h, None, None, None, level, 0, 0, counts) == arg              # null pointers
        assert lib.xb_isosurface(h, None, None, lp, level, 0, 0, None) == arg
        assert lib.xb_isosurface(h, None, None, lp, level, 0, 2, counts) == arg                # unknown flag bits
        for bad in (float('nan'), float('inf'), float('-inf')):
            assert lib.xb_isosurface(h, None, None, lp, bad, 0, 0, counts) == arg             # a level that is not finite
        assert lib.xb_isosurface(h, None, None, lp, level, -1, 0, counts) == arg
        assert lib.xb_isosurface(h, None, None, flat, level, 0, 0, counts) == arg              # a lattice xb_stencil_coeffs refuses
        assert lib.xb_isosurface(h, C.c_void_p(rho.ctypes.data), None, lp, level, 0, 0, counts) == arg       # a host pointer
        assert lib.xb_isosurface(h, C.c_void_p(d.ptr + 8), None, lp, level, 0, 0, counts) == arg             # past its allocation
        assert lib.xb_isosurface(h, C.c_void_p(d.ptr + 4), None, lp, level, 0, 0, counts) == arg             # not aligned
        big = device.DeviceArray(c, (2 * rho.size - 1,), np.float64)
        assert lib.xb_isosurface(h, C.c_void_p(big.ptr), C.c_void_p(big.ptr + 8 * (rho.size - 1)), lp, level, 0, 0, counts) == arg   # overlapping
        assert lib.xb_isosurface(h, None, None, lp, level, 2 ** 31, 0, counts) == limit
        assert tuple(counts) == (-7, -7)
        # a mesh, and the fetch: capacity too small writes nothing
        assert lib.xb_device_write(h, vd, C.c_void_p(rho.ctypes.data), rho.nbytes) == 0
        assert lib.xb_isosurface(h, vd, None, lp, level, 1, 0, counts) == 0
        V, T = counts[0], counts[1]
        want = restate(rho, level, lat)
        assert (V, T) == (want.vertices.shape[0], want.triangles.shape[0]) and T > 0
        vert, tri = np.full((V, 3), -7.0), np.full((T, 3), -7, np.int64)
        wrap, cell, vbl = np.full(T, 7, np.uint16), np.full(T, -7, np.int64), np.full(1, -7.0)
        p = lambda a: C.c_void_p(a.ctypes.data)       # noqa: E731
        pv = vbl.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.xb_isosurface_fetch(h, 0, p(vert), None, p(tri), p(wrap), p(cell), V - 1, T, sc, pv, 1) == arg
        assert lib.xb_isosurface_fetch(h, 0, p(vert), None, p(tri), p(wrap), p(cell), V, T - 1, sc, pv, 1) == arg
        assert lib.xb_isosurface_fetch(h, 0, p(vert), None, p(tri), p(wrap), p(cell), V, T, sc, pv, 0) == arg        # no room for the labels
        assert lib.xb_isosurface_fetch(h, 0, p(vert), None, p(tri), p(wrap), p(cell), V, T, sc, None, 1) == arg
        assert lib.xb_isosurface_fetch(h, 0, None, None, p(tri), p(wrap), p(cell), V, T, sc, pv, 1) == arg
        assert lib.xb_isosurface_fetch(h, 0, p(vert), p(vert), p(tri), p(wrap), p(cell), V, T, sc, pv, 1) == arg     # no colour was made
        assert lib.xb_isosurface_fetch(h, 1, p(vert), None, p(tri), p(wrap), p(cell), V, T, sc, pv, 1) == arg        # host pointers as device arrays
        assert (vert == -7.0).all() and (tri == -7).all() and (wrap == 7).all() and (cell == -7).all() and vbl[0] == -7.0
        assert lib.xb_isosurface_fetch(h, 0, p(vert), None, p(tri), p(wrap), p(cell), V, T, sc, pv, 1) == 0
        assert np.array_equal(vert, want.vertices) and np.array_equal(tri, want.triangles)
        # into device arrays
        dv, dt = device.DeviceArray(c, (V, 3), np.float64), device.DeviceArray(c, (T, 3), np.int64)
        dw, dc = device.DeviceArray(c, (T,), np.uint16), device.DeviceArray(c, (T,), np.int64)
        q = lambda a: C.c_void_p(a.ptr)               # noqa: E731
        assert lib.xb_isosurface_fetch(h, 1, q(dv), None, q(dt), q(dw), q(dc), V, T, sc, pv, 1) == 0
        assert np.array_equal(dv.to_host(), want.vertices) and np.array_equal(dt.to_host(), want.triangles)
        assert np.array_equal(dw.to_host(), want.wrap) and np.array_equal(dc.to_host(), want.cells)
        assert lib.xb_isosurface_fetch(h, 1, q(dv), None, q(dt), q(dw), q(dw), V, T, sc, pv, 1) == arg               # two destinations overlap
        # the mask of the NCI surface, and the upload
        assert lib.xb_isosurface_nci_mask(h, None, 0.05) == arg
        assert lib.xb_isosurface_nci_mask(h, C.c_void_p(rho.ctypes.data), 0.05) == arg
        assert lib.xb_isosurface_nci_mask(h, vd, float('nan')) == arg
        assert lib.xb_isosurface_nci_mask(h, C.c_void_p(d.ptr + 8), 0.05) == arg
        assert lib.xb_device_write(h, None, C.c_void_p(rho.ctypes.data), 8) == arg
        assert lib.xb_stream_wait(None, None) == arg and lib.xb_stream_wait(h, None) == 0       # (None: the legacy default stream)
        assert lib.xb_device_write(h, ve, None, 8) == arg
        assert lib.xb_device_write(h, ve, C.c_void_p(rho.ctypes.data), rho.nbytes + 8) == arg
        with pytest.raises(ValueError):
            isosurface.isosurface(rho, lat, level, volumes=np.zeros((3, 3, 3), np.int32), n=2)
        # a slab is refused; the whole grid works again
        c.set_grid(shape, np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(rho)
        assert lib.xb_isosurface(h, None, None, lp, level, 0, 0, counts) == state
        assert lib.xb_isosurface_nci_mask(h, vd, 0.05) == state
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        assert first_difference(c.isosurface(lat, level), want, 'the whole grid again') is None
    finally:
        c.close()


# ---- Bader(isosurface_level=...) ------------------------------------------------------------------------------------------------------
def test_bader_with_the_option(monkeypatch):
    """the run of tests/test_gpu_all_flags.py (fields rounded so that its sums are exact) with and without isosurface_level: every
    other attribute is unchanged, the new ones equal the restatement on the run's own atoms_volumes"""
    import test_gpu_all_flags as AF
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    off = AF.make('default')
    off()
    rho = AF.field('charge')
    level = float(np.quantile(rho, 0.8))
    on = AF.make('default', isosurface_level=level)
    on()
    new = {'isosurface_level', 'isosurface', 'isosurface_area', 'isosurface_volume', 'atoms_isosurface_volume'}
    assert set(vars(on)) - set(vars(off)) == new and off.isosurface_level is None
    AF.same_exact_attributes(on, off, 'isosurface_level on against off')
    want = restate(rho, level, AF.LAT, labels=np.asarray(AF.host(on.atoms_volumes)), n=AF.N_ATOMS)
    assert want.triangles.shape[0] > 1000
    got = as_tuple(on.isosurface)[:7] + (on.atoms_isosurface_volume,)
    assert first_difference(got, want, 'Bader') is None and sums_difference(got, want, 'Bader') is None
    assert (on.isosurface_area, on.isosurface_volume) == (on.isosurface.area, on.isosurface.volume)

"""xb_nci_field / xb_nci_sum / xb_nci_hist and what stands on them (-m gpu) against the numpy restatement of
tests/test_nci_cpu.py.

x = sign(lambda2) rho, the counts of the region and the histogram are compared with == : every operation that decides them is
bit-defined (include/bader_hip.h).  XB_STENCIL_GATHER is the second implementation: everything runs through the tiles and
through the gather.  The field s passes through sqrt and cbrt on both sides; THE BOUND on it is

    |got - want| <= 16 * 2**-52 * want

twice the sum of the documented bounds of sqrt (0.5 ulp), cbrt (1 ulp), two multiplications and a division (0.5 ulp each) on
each side, in units of 2**-52 -- and the two routes must give the same bits as each other.  THE BOUND of the sums, per key
3 a + class, for the sum of rho and the sum of rho^2 alike (tests/test_gpu_laplacian.py's, taken from there):

    |got - fsum(terms) * vv| <= (count + 2) * 2**-53 * fsum(|terms|) * |vv|

tests/test_nci_cpu.py::test_the_bound_notices_a_voxel_in_the_wrong_class (collected here as well) shows for every input used
here that one voxel in the wrong class breaks this bound."""
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
from pybader_amd import _lib, device, nci, thread_handlers, utils
from test_gpu_history import Runner
from test_laplacian_cpu import grouped, restated_values, sum_bound
from test_multipole_cpu import VV, label_map
from test_nci_cpu import (HISTORY_CUTS, HISTORY_EDGES, LABELS_LDS, LATS, S_REL, SUM_CUTS, check_s, check_sums, classes, density,
                          fields_difference, histogram, histogram_difference, keys, region, regions_difference, restated, sum_inputs,
                          sum_reference, thresholds, values)
from test_nci_cpu import test_the_bound_notices_a_voxel_in_the_wrong_class  # noqa: F401 -- runs here too

pytestmark = pytest.mark.gpu
FIELD_SHAPES = [(13, 17, 19), (20, 9, 33), (1, 2, 5), (2, 1, 40), (16, 16, 64)]
LDS_BINS = _lib.XB_NCI_HIST_LDS_BINS


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
    diff = np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ from the restatement, first at {np.argwhere(diff)[0].tolist()}'


# ---- the fields -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', list(LATS))
@pytest.mark.parametrize('shape', FIELD_SHAPES)
def test_fields_equal_the_restatement_through_both_routes(ctx, shape, lname):
    rho, lat, v = density('holes', shape, lname), LATS[lname], values('holes', shape, lname)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(rho)
    s_tile, x_tile = ctx.nci_field(lat)
    s_gather, x_gather = ctx.nci_field(lat, gather=True)
    same_bits(x_tile, v['x'], f'{shape} {lname} x (tiles, host output)')
    same_bits(x_gather, v['x'], f'{shape} {lname} x (gather, host output)')
    check_s(s_tile, v, f'{shape} {lname} (tiles)')
    same_bits(s_gather, s_tile, f'{shape} {lname} s: the gather against the tiles')
    for gather in (False, True):
        s_dev, x_dev = ctx.nci_field(lat, gather=gather, on_device=True)
        assert all(isinstance(a, device.DeviceArray) and a.shape == shape and a.dtype == np.float64 for a in (s_dev, x_dev))
        same_bits(x_dev.to_host(), v['x'], f'{shape} {lname} x (gather {gather}, device output)')
        same_bits(s_dev.to_host(), s_tile, f'{shape} {lname} s (gather {gather}, device output) against the host output')
    assert np.array_equal(ctx.download_density().view(np.uint64), rho.view(np.uint64)), 'the resident density is not written'
    assert (~v['pos']).any() and (v['sigma'][v['pos']] < 0).any()


def test_fields_of_a_constant_density(ctx):
    shape = (5, 6, 7)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(np.full(shape, 0.03125))
    for gather in (False, True):
        s, x = ctx.nci_field(LATS['tric'], gather=gather)
        assert not s.any() and not x.any() and not np.signbit(x).any()
        ctx.upload_labels(np.zeros(shape, np.int32))
        count, charge, _ = ctx.nci_sum(LATS['tric'], 1, VV, 0.5, 0.05, 0.01, gather)
        assert count.tolist() == [[0, 210, 0]] and charge[0, 1] == 210 * 0.03125 * VV


def test_fields_of_device_tensors_and_a_host_array_through_the_python_layer():
    shape, lname = (20, 9, 33), 'tric'
    rho, lat = density('holes', shape, lname), LATS[lname]
    s, x = nci.nci_fields(rho, lat)
    assert isinstance(s, np.ndarray) and isinstance(x, np.ndarray)
    v = values('holes', shape, lname)
    same_bits(x, v['x'], 'host array')
    check_s(s, v, 'host array')
    with utils.resident(rho):
        for gather in (True, False):
            s2, x2 = nci.nci_fields(rho, lat, gather=gather)
            same_bits(x2, v['x'], f'resident, gather {gather}')
            same_bits(s2, s, f'resident, gather {gather}: s')
    if not have_torch():
        pytest.skip('the host array passed; torch with a GPU is needed for a device tensor')
    rho32 = rho.astype(np.float32)
    v32 = restated(rho32.astype(np.float64), lat)
    perm = torch.as_tensor(np.ascontiguousarray(rho.transpose(2, 0, 1)), device='cuda').permute(1, 2, 0)
    assert tuple(perm.shape) == shape and not perm.is_contiguous()
    for what, t, want in (('float32 tensor', torch.as_tensor(rho32.copy(), device='cuda'), v32), ('permuted float64 tensor', perm, v)):
        for gather in (False, True):
            sd, xd = nci.nci_fields(t, lat, gather=gather)
            assert isinstance(sd, device.DeviceArray) and isinstance(xd, device.DeviceArray)
            same_bits(xd.to_host(), want['x'], f'{what}, gather {gather}')
            check_s(sd.to_host(), want, f'{what}, gather {gather}')
            back = torch.as_tensor(xd, device='cuda')        # (the result publishes the interface: no copy)
            assert back.dtype == torch.float64 and tuple(back.shape) == shape


# ---- the region's sums ------------------------------------------------------------------------------------------------------------
def test_sums_on_every_input_through_both_routes(ctx):
    assert LABELS_LDS == 85
    resident = None
    for what, kind, shape, lname, lab, n in sum_inputs():
        rho, v = density(kind, shape, lname), values(kind, shape, lname)
        if resident != (kind, shape, lname):
            ctx.set_grid(shape, np.zeros(27), np.zeros(9))
            ctx.upload_density(rho)
            resident = (kind, shape, lname)
        ctx.upload_labels(lab)
        for gather in (False, True):
            cnt = check_sums(ctx.nci_sum(LATS[lname], n, VV, *SUM_CUTS, gather), v, lab, n, f'{what}, gather {gather}')
        assert all(cnt[c::3].sum() >= 20 for c in range(3)), 'every class holds voxels'
    assert np.array_equal(ctx.download_labels(np.int32), lab) and np.array_equal(ctx.download_density(), rho), 'nothing resident is written'


@pytest.mark.parametrize('cuts', [(0.5, 0.05, 0.01), (0.5, 0.3, 0.02), (0.3, 0.5, 0.0), (0.0, 1.0, 0.01), (2.0, 0.0, 0.01)])
def test_sums_with_other_thresholds_through_the_python_layer(cuts):
    shape, lname, n = (20, 9, 33), 'cubic', 3
    rho, v = density('holes', shape, lname), values('holes', shape, lname)
    lab = label_map(shape, n)
    for gather in (False, True):
        r = nci.nci_regions(rho, lab.astype(np.int8), LATS[lname], n, VV, *cuts, gather=gather)
        cnt = check_sums((r.count, r.charge, r.charge2), v, lab, n, f'cuts {cuts}, gather {gather}', cuts)
        assert np.array_equal(r.volume, r.count.astype(np.float64) * VV) and (r.s_cut, r.rho_cut, r.rho_split) == cuts
    if cuts[0] == 0.0 or cuts[1] == 0.0:
        assert not cnt.any(), 'nothing lies below a zero threshold'
    else:
        assert cnt.sum() > 0, 'the restated region is no empty set'
    empty = nci.nci_regions(rho, lab, LATS[lname], 0, VV)
    assert empty.count.shape == empty.charge.shape == empty.volume.shape == (0, 3)


def test_the_buffer_is_counted():
    shape = (13, 17, 19)
    c = _lib.Context(0)
    try:
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(density('holes', shape, 'tric'))
        c.upload_labels(label_map(shape, 2))
        before = c.memory_stats()
        c.nci_sum(LATS['tric'], 3000, VV, *SUM_CUTS)
        after = c.memory_stats()
        assert after[2] - before[2] == 72 * 3000 and after[0] - before[0] == after[2] - before[2]
        c.nci_sum(LATS['tric'], 2, VV, *SUM_CUTS)                          # (a smaller n fits the buffer)
        c.nci_hist(LATS['tric'], np.linspace(0.0, 2.0, 101), np.linspace(-1.0, 1.0, 201))     # (100 x 200 bins + 302 edges: so does this)
        c.nci_field(LATS['tric'])                                          # (the fields go through scratch and a temporary)
        assert c.memory_stats() == after
        c.nci_hist(LATS['tric'], np.linspace(0.0, 2.0, 201), np.linspace(-1.0, 1.0, 201))
        assert c.memory_stats()[2] - before[2] == 8 * (200 * 200 + 402)
    finally:
        c.close()


# ---- the histogram ----------------------------------------------------------------------------------------------------------------
def edge_on_a_voxel(v):
    """(e, flat index): a threshold e with T(e) * r8 == q EXACTLY at a voxel with rho > 0 -- the voxel's own s from the
    restatement, moved by a few ulps until the products meet.  The voxel then lies ON the edge: `<=` puts it into the bin that
    starts there, `<` would put it below."""
    s, q, r8, pos, x = (v[k].reshape(-1) for k in ('s', 'q', 'r8', 'pos', 'x'))
    for i in np.flatnonzero(pos & (s > 0.2) & (s < 1.5) & (np.abs(x) < 0.19)):      # (inside the x edges of hist_edges)
        e = s[i]
        for _ in range(16):
            e = np.nextafter(e, 0.0)
        for _ in range(33):
            if thresholds(e) * r8[i] == q[i]:
                return float(e), int(i)
            e = np.nextafter(e, np.inf)
    raise AssertionError('no voxel whose own s can be met exactly')


@functools.lru_cache(maxsize=None)
def hist_edges(shape, lname, n_s, n_x):
    """edges with voxels outside on every side; with two bins or more along an axis, one inner s edge exactly at a voxel's own
    value and one inner x edge exactly at a voxel's x (each voxel inside the other axis' edges, so that it is counted)"""
    v = values('holes', shape, lname)
    e, i = edge_on_a_voxel(v)
    s_edges = np.linspace(0.15, 2.0, n_s + 1)
    if n_s >= 2:
        s_edges[np.argmin(np.abs(s_edges[1:-1] - e)) + 1] = e
    x, s = v['x'].reshape(-1), v['s'].reshape(-1)
    x_edges = np.linspace(-0.2, 0.2, n_x + 1)
    j = int(np.flatnonzero(v['pos'].reshape(-1) & (x > 0.01) & (x < 0.19) & (s > 0.2) & (s < 1.5))[0])
    if n_x >= 2:
        x_edges[np.argmin(np.abs(x_edges[1:-1] - x[j])) + 1] = x[j]
    assert (np.diff(s_edges) > 0).all() and (np.diff(x_edges) > 0).all()
    return s_edges, x_edges, e, i, j


@pytest.mark.parametrize('bins', [(4, 5), (32, 32), (33, 32), (1, LDS_BINS), (LDS_BINS + 1, 1), (64, 48)])
@pytest.mark.parametrize('shape,lname', [((20, 9, 33), 'tric'), ((13, 17, 19), 'cubic')])
def test_histogram_on_both_sides_of_the_lds_limit(ctx, shape, lname, bins):
    n_s, n_x = bins
    v = values('holes', shape, lname)
    s_edges, x_edges, e, i, j = hist_edges(shape, lname, n_s, n_x)
    want = histogram(v, s_edges, x_edges)
    # the edges do what they are there for: voxels outside on every side, and the voxel on the s edge counted from that edge up
    t = thresholds(s_edges)
    q, r8, x, pos = (v[k].reshape(-1) for k in ('q', 'r8', 'x', 'pos'))
    assert (pos & (q < t[0] * r8)).any() and (pos & (t[-1] * r8 <= q)).any() and (x < x_edges[0]).any() and (x >= x_edges[-1]).any()
    if n_s >= 2:
        assert t[int(np.flatnonzero(s_edges == e)[0])] * r8[i] == q[i]
    if n_x >= 2:
        assert (x_edges == x[j]).sum() == 1
    assert 0 < want.sum() < int(pos.sum())
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(density('holes', shape, lname))
    for gather in (False, True):
        got = ctx.nci_hist(LATS[lname], s_edges, x_edges, gather)
        assert got.dtype == np.int64 and got.shape == (n_s, n_x)
        assert np.array_equal(got, want), f'{shape} {lname} {bins}, gather {gather}: {int((got != want).sum())} bins differ'
    assert (n_s * n_x <= LDS_BINS) == (bins in [(4, 5), (32, 32), (1, LDS_BINS)])


def test_the_histogram_pins_less_or_equal(ctx):
    """the voxel on the s edge and the voxel on the x edge: counted with `<` instead of `<=` each would land one bin lower, and
    the restated histogram would differ from the device's"""
    shape, lname = (20, 9, 33), 'tric'
    v = values('holes', shape, lname)
    s_edges, x_edges, e, i, j = hist_edges(shape, lname, 4, 5)
    t = thresholds(s_edges)
    q, r8, x, pos = (v[k].reshape(-1) for k in ('q', 'r8', 'x', 'pos'))
    ks = sum((tj * r8 < q).astype(np.int64) for tj in t) - 1                 # the wrong rule
    kx = sum((xj < x).astype(np.int64) for xj in x_edges) - 1
    ok = pos & (ks >= 0) & (ks < 4) & (kx >= 0) & (kx < 5)
    strict = np.zeros((4, 5), np.int64)
    np.add.at(strict, (ks[ok], kx[ok]), 1)
    want = histogram(v, s_edges, x_edges)
    assert not np.array_equal(strict, want)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ctx.upload_density(density('holes', shape, lname))
    assert np.array_equal(nci.nci_histogram(density('holes', shape, lname), LATS[lname], s_edges, x_edges), want)
    assert np.array_equal(ctx.nci_hist(LATS[lname], s_edges, x_edges), want)


# ---- error codes --------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    c = _lib.Context(0)
    try:
        shape = (8, 8, 8)
        rho = np.ascontiguousarray(density('rough', shape, 'cubic'))
        lat = LATS['cubic']
        n_vox = rho.size
        se, xe = np.array([0.0, 0.5, 1.0]), np.array([-0.1, 0.0, 0.1])
        calls = (lambda: c.nci_field(lat), lambda: c.nci_sum(lat, 2, VV, 0.5, 0.05, 0.01), lambda: c.nci_hist(lat, se, xe))
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
            c.nci_sum(lat, 2, VV, 0.5, 0.05, 0.01)
        assert e.value.code == _lib.XB_E_STATE                      # no labels
        c.upload_labels(np.zeros(shape, np.int32))
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        lp = (C.c_double * 9)(*lat.reshape(-1))
        flat = (C.c_double * 9)(1, 2, 3, 2, 4, 6, 0, 0, 1)          # a singular lattice
        out_s, out_x = np.full(n_vox, -7.0), np.full(n_vox, -7.0)
        ps, px = out_s.ctypes.data, out_x.ctypes.data
        ds, dx = device.DeviceArray(c, shape, np.float64), device.DeviceArray(c, shape, np.float64)
        vs, vx = C.c_void_p(ds.ptr), C.c_void_p(dx.ptr)
        lib, h, arg, limit = c.lib, c.h, _lib.XB_E_ARG, _lib.XB_E_LIMIT
        # the field: a null lattice, outputs mixed, incomplete or missing, unknown flag bits, a singular lattice, host pointers as
        # device outputs, a device output one element past its allocation, one not aligned, the two the same
        assert lib.xb_nci_field(h, None, 0, ps, px, None, None) == arg
        assert lib.xb_nci_field(h, lp, 0, ps, px, vs, vx) == arg
        assert lib.xb_nci_field(h, lp, 0, ps, None, None, vx) == arg
        assert lib.xb_nci_field(h, lp, 0, ps, None, None, None) == arg
        assert lib.xb_nci_field(h, lp, 0, None, None, vs, None) == arg
        assert lib.xb_nci_field(h, lp, 0, None, None, None, None) == arg
        assert lib.xb_nci_field(h, lp, 2, ps, px, None, None) == arg
        assert lib.xb_nci_field(h, flat, 0, ps, px, None, None) == arg
        assert lib.xb_nci_field(h, lp, 0, None, None, ps, px) == arg
        assert n_vox * 8 == ds.nbytes == 4096
        assert lib.xb_nci_field(h, lp, 0, None, None, vs, C.c_void_p(dx.ptr + 8)) == arg
        assert lib.xb_nci_field(h, lp, 0, None, None, C.c_void_p(ds.ptr + 4), vx) == arg
        assert lib.xb_nci_field(h, lp, 0, None, None, vs, vs) == arg
        assert (out_s == -7.0).all() and (out_x == -7.0).all(), 'a refused call writes nothing'
        # the sums: null pointers, unknown flag bits, n < 1, thresholds that are negative or not finite, a singular lattice, n
        # beyond the limit
        cnt, ch, ch2 = np.full(6, -7, np.int64), np.full(6, -7.0), np.full(6, -7.0)
        pc, pch, pch2 = cnt.ctypes.data_as(pi), ch.ctypes.data_as(pd), ch2.ctypes.data_as(pd)
        good = (0.5, 0.05, 0.01)
        assert lib.xb_nci_sum(h, None, 2, VV, *good, 0, pc, pch, pch2) == arg
        assert lib.xb_nci_sum(h, lp, 2, VV, *good, 0, None, pch, pch2) == arg
        assert lib.xb_nci_sum(h, lp, 2, VV, *good, 0, pc, None, pch2) == arg
        assert lib.xb_nci_sum(h, lp, 2, VV, *good, 0, pc, pch, None) == arg
        assert lib.xb_nci_sum(h, lp, 2, VV, *good, 4, pc, pch, pch2) == arg
        assert lib.xb_nci_sum(h, lp, 0, VV, *good, 0, pc, pch, pch2) == arg
        for k in range(3):
            for bad in (-0.25, float('nan'), float('inf')):
                cuts = list(good)
                cuts[k] = bad
                assert lib.xb_nci_sum(h, lp, 2, VV, *cuts, 0, pc, pch, pch2) == arg, (k, bad)
        assert lib.xb_nci_sum(h, flat, 2, VV, *good, 0, pc, pch, pch2) == arg
        assert lib.xb_nci_sum(h, lp, (2 ** 31 - 1) // 3 + 1, VV, *good, 0, pc, pch, pch2) == limit
        assert (cnt == -7).all() and (ch == -7.0).all() and (ch2 == -7.0).all()
        # the histogram: null pointers, unknown flag bits, fewer than one bin, edges that are not finite, not strictly increasing, s
        # edges below zero, a singular lattice, more bins than the limit
        hist = np.full(4, -7, np.int64)
        ph = hist.ctypes.data_as(pi)
        e_s, e_x = se.ctypes.data_as(pd), xe.ctypes.data_as(pd)
        assert lib.xb_nci_hist(h, None, e_s, 2, e_x, 2, 0, ph) == arg
        assert lib.xb_nci_hist(h, lp, None, 2, e_x, 2, 0, ph) == arg
        assert lib.xb_nci_hist(h, lp, e_s, 2, None, 2, 0, ph) == arg
        assert lib.xb_nci_hist(h, lp, e_s, 2, e_x, 2, 0, None) == arg
        assert lib.xb_nci_hist(h, lp, e_s, 2, e_x, 2, 8, ph) == arg
        assert lib.xb_nci_hist(h, lp, e_s, 0, e_x, 2, 0, ph) == arg
        assert lib.xb_nci_hist(h, lp, e_s, 2, e_x, -1, 0, ph) == arg
        assert lib.xb_nci_hist(h, flat, e_s, 2, e_x, 2, 0, ph) == arg
        for bad_s, bad_x in (([0.0, 0.5, 0.5], None), ([0.0, 0.7, 0.5], None), ([0.0, float('nan'), 1.0], None),
                             ([0.0, 0.5, float('inf')], None), ([-0.1, 0.5, 1.0], None), (None, [-0.1, -0.1, 0.1]),
                             (None, [0.1, 0.0, -0.1]), (None, [-0.1, float('nan'), 0.1]), (None, [float('-inf'), 0.0, 0.1])):
            bs = np.array(bad_s if bad_s is not None else se)
            bx = np.array(bad_x if bad_x is not None else xe)
            assert lib.xb_nci_hist(h, lp, bs.ctypes.data_as(pd), 2, bx.ctypes.data_as(pd), 2, 0, ph) == arg, (bad_s, bad_x)
        big = _lib.XB_NCI_BINS_MAX
        assert lib.xb_nci_hist(h, lp, e_s, big + 1, e_x, 1, 0, ph) == limit        # (refused before an edge is read)
        assert lib.xb_nci_hist(h, lp, e_s, 1, e_x, big + 1, 0, ph) == limit
        assert lib.xb_nci_hist(h, lp, e_s, 4097, e_x, 4096, 0, ph) == limit
        assert (hist == -7).all()
        with pytest.raises(_lib.BaderHipError) as e:
            c.nci_hist(lat, [0.0], xe)
        assert e.value.code == arg
        with pytest.raises(ValueError):
            nci.nci_regions(rho, np.zeros((3, 3, 3), np.int32), lat, 2, VV)
        # a slab is refused; the whole grid works again
        c.set_grid(shape, np.zeros(27), np.zeros(9), (2, 5))
        c.upload_density(rho)
        c.upload_labels(np.zeros(shape, np.int32))
        for call in calls:
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code == _lib.XB_E_STATE
        c.set_grid(shape, np.zeros(27), np.zeros(9))
        c.upload_density(rho)
        same_bits(c.nci_field(lat)[1], restated(rho, lat)['x'], 'the whole grid again')
    finally:
        c.close()


# ---- call history -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def history_values(grid):
    return restated(H.density(grid, 'A'), H.LAT)


def nci_call(kind, grid):
    """one of the three calls through the public functions on density A and the atom map of a grid of history_common -> None, or
    what differs from the restatement"""
    rho, lab, n, v = H.density(grid, 'A'), H.labels(grid, 'atoms'), H.n_of(grid, 'atoms'), history_values(grid)
    if kind == 'fields':
        s, x = nci.nci_fields(rho, H.LAT)
        return fields_difference(s, x, v, f'nci_fields on {grid}')
    if kind == 'regions':
        r = nci.nci_regions(rho, lab, H.LAT, n, VV, *HISTORY_CUTS)
        return regions_difference(r.count, r.charge, r.charge2, sum_reference(v, lab, n, HISTORY_CUTS), f'nci_regions on {grid}')
    got = nci.nci_histogram(rho, H.LAT, *HISTORY_EDGES)
    return histogram_difference(got, histogram(v, *HISTORY_EDGES), f'nci_histogram on {grid}')


@pytest.mark.parametrize('other', ['basin_laplacian', 'critical', 'voronoi'])
@pytest.mark.parametrize('kind', ['fields', 'regions', 'histogram'])
def test_call_history_does_not_matter(kind, other, monkeypatch):
    """each call directly before and directly after xb_laplacian_sum, xb_critical_points and xb_voronoi_assign (which rewrites the
    device labels), on G1 -> G2 -> G1 of history_common.GRIDS, on the default context: both sides' results are unchanged"""
    H.cache_facet_areas(monkeypatch)
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    run = Runner()
    bad = []
    try:
        for grid in ('G1', 'G2', 'G1'):
            for step in (lambda: nci_call(kind, grid), lambda: run.checked(other, grid, 'A', 'atoms'), lambda: nci_call(kind, grid),
                         lambda: run.checked(other, grid, 'A', 'atoms')):
                msg = step()
                if msg:
                    bad.append(f'{grid}: {msg}')
        with utils.resident(H.density('G1', 'A')):
            for step in (lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: nci_call(kind, 'G1'),
                         lambda: run.checked(other, 'G1', 'A', 'atoms'), lambda: nci_call(kind, 'G1')):
                msg = step()
                if msg:
                    bad.append(f'resident(A): {msg}')
    finally:
        c = _lib.default_context()
        c.pinned_density = c.resident_density = None
        c.drop_label_token()
    assert not bad, ' | '.join(bad[:4])


# ---- Bader(nci_flag=True) -------------------------------------------------------------------------------------------------------------
NCI_ATTRIBUTES = {'nci_flag', 'nci_s_cut', 'nci_rho_cut', 'nci_rho_split', 'atoms_nci_count', 'atoms_nci_volume', 'atoms_nci_charge',
                  'atoms_bond_nci'}
# the two Gaussian atoms of tests/test_gpu_all_flags.py stand in no background: s grows without bound in their tails and the
# default thresholds leave the region empty.  With these the attractive and the van der Waals class hold voxels on the charge
# density and on the reference alike (no voxel of such a density has two positive curvatures at a density above the split)
BADER_CUTS = {'nci_s_cut': 20.0, 'nci_rho_cut': 0.5, 'nci_rho_split': 0.002}


@pytest.mark.parametrize('profile', ['default', 'reference and vacuum', 'permuted float32 tensor'])
def test_bader_with_the_flag_and_every_other_flag(profile, monkeypatch):
    """every analysis flag of tests/test_gpu_all_flags.py with and without nci_flag: without it the run is what that file pins
    (its restatements, on the right fields); with it every one of those attributes is unchanged, and the new ones equal the direct
    calls and the restatement on the REFERENCE density and the run's own atoms_volumes"""
    H.cache_facet_areas(monkeypatch)
    if AF.PROFILES[profile].get('tensor') and not have_torch():
        pytest.skip('torch sees no device')
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    flags = {f: True for f in AF.FLAGS}
    off = AF.make(profile, **flags)
    off()
    AF.verify(off, profile, 'every flag, nci_flag off')
    assert off.nci_flag is False and not NCI_ATTRIBUTES & set(vars(off))
    on = AF.make(profile, nci_flag=True, **BADER_CUTS, **flags)
    on()
    AF.verify(on, profile, 'every flag and nci_flag')
    assert set(vars(on)) - set(vars(off)) == NCI_ATTRIBUTES
    AF.same_exact_attributes(on, off, f'{profile}: nci_flag on against off')
    # the new attributes: the restatement on the reference, and the direct calls
    ref, dens, _, _ = AF.fields_of(profile)
    cuts = (on.nci_s_cut, on.nci_rho_cut, on.nci_rho_split)
    assert cuts == tuple(BADER_CUTS.values())
    v = restated(ref, AF.LAT)
    lab = np.asarray(AF.host(on.atoms_volumes))
    vv, n = on.voxel_volume, AF.N_ATOMS
    k = keys(v, lab, n, *cuts)
    s1, cnt, mag1 = grouped(v['rho'], k, 3 * n)
    print(profile, 'atoms_nci_count', on.atoms_nci_count.tolist(), 'atoms_bond_nci', on.atoms_bond_nci.tolist())
    assert on.atoms_nci_count.shape == (n, 3) and np.array_equal(on.atoms_nci_count.reshape(-1), cnt)
    assert cnt[0::3].sum() > 100 and cnt[1::3].sum() > 100, 'two classes hold voxels'
    assert np.array_equal(on.atoms_nci_volume, on.atoms_nci_count.astype(np.float64) * vv)
    lim = sum_bound(cnt, mag1, vv)
    assert np.all(np.abs(on.atoms_nci_charge.reshape(-1) - s1 * vv) <= lim)
    direct = nci.nci_regions(on.reference, on.atoms_volumes, AF.LAT, n, vv, *cuts)
    assert np.array_equal(direct.count, on.atoms_nci_count) and np.array_equal(direct.volume, on.atoms_nci_volume)
    assert np.all(np.abs(direct.charge - on.atoms_nci_charge).reshape(-1) <= 2 * lim)      # (two runs of float atomics)
    if AF.PROFILES[profile].get('reference'):       # ... and the charge density's regions are others
        assert not np.array_equal(grouped(dens, keys(restated(dens, AF.LAT), lab, n, *cuts), 3 * n)[1], cnt)
    lin = on.atoms_bond_graph.voxel
    want = np.where(region(v, cuts[0], cuts[1]), classes(v, cuts[2]), -1).reshape(-1)[lin]
    assert on.atoms_bond_nci.dtype == np.int8 and on.atoms_bond_nci.shape == (len(on.atoms_bond_graph),)
    assert np.array_equal(on.atoms_bond_nci, want)
    assert np.array_equal(nci.bond_classes(on.reference, AF.LAT, lin, *cuts), want)
    ten = np.ascontiguousarray(restated_values(ref, AF.LAT).reshape(10, -1).T[lin])
    assert np.array_equal(nci.point_classes(ten, *cuts), want)
    # without critical_flag there are no bond voxels to classify
    lean = AF.make(profile, nci_flag=True, **BADER_CUTS)
    lean()
    assert not hasattr(lean, 'atoms_bond_nci') and np.array_equal(lean.atoms_nci_count, on.atoms_nci_count)

"""Device arrays in, device arrays out (-m gpu): pybader_amd.device, the xb_import_* / xb_export_* entry points and the
same-named Python calls with a torch tensor as the density.  Every tensor is made with torch; the library itself never
imports it."""
import itertools

import numpy as np
import pytest
import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)

from conftest import case_density, load_golden
from rough_common import load_rough
from pybader_amd import _lib, device, synth, thread_handlers, utils
from pybader_amd.interface import Bader
from pybader_amd.utils import dtype_calc

pytestmark = pytest.mark.gpu

SHAPES = [(40, 48, 56), (64, 64, 64), (33, 17, 50)]
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


class Raw:
    """a hand-made interface over memory some tensor owns (offset pointers, negative strides: what torch cannot express)"""

    def __init__(self, owner, ptr, shape, byte_strides, typestr, readonly=False):
        self.owner = owner
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), readonly), 'version': 2,
                                         'strides': None if byte_strides is None else tuple(byte_strides)}


def special_values(shape, dtype, seed):
    """random values with -0.0, +-inf, subnormals, the extremes of the dtype and a few NaNs strewn in"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(dtype)
    fi = np.finfo(dtype)
    specials = [-0.0, 0.0, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
                fi.tiny / 3, fi.eps, np.nan]
    if dtype == np.float64:
        f4 = np.finfo(np.float32)
        specials += [float(f4.max), float(f4.tiny), float(f4.smallest_subnormal)]
    flat = a.reshape(-1)
    where = rng.choice(flat.size, size=4 * len(specials), replace=False)
    flat[where] = np.tile(np.array(specials, dtype), 4)
    return a


def assert_same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), 'NaN positions differ'
    g, w = got.view(np.uint64), want.view(np.uint64)
    assert np.array_equal(g[~nan], w[~nan]), f'{int((g[~nan] != w[~nan]).sum())} values differ in their bits'


def layouts(shape, np_dtype, seed):
    """(name, device array of logical shape `shape`, expected host array) for every layout of the issue"""
    out = []
    for perm in itertools.permutations(range(3)):            # identity = contiguous
        base = special_values(tuple(shape[p] for p in perm), np_dtype, seed)
        inv = tuple(np.argsort(perm))
        t = torch.from_numpy(base).to(DEV).permute(*inv)
        out.append((f'perm{perm}', t, base.transpose(inv)))
    for ax in range(3):
        big = list(shape)
        big[ax] *= 2
        base = special_values(tuple(big), np_dtype, seed + 1)
        sl = [slice(None)] * 3
        sl[ax] = slice(None, None, 2)
        out.append((f'step2_axis{ax}', torch.from_numpy(base).to(DEV)[tuple(sl)], base[tuple(sl)]))
        one = list(shape)
        one[ax] = 1
        base = special_values(tuple(one), np_dtype, seed + 2)
        out.append((f'expand_axis{ax}', torch.from_numpy(base).to(DEV).expand(*shape), np.broadcast_to(base, shape)))
        base = special_values(shape, np_dtype, seed + 3)       # a flipped axis: offset pointer + negative stride, raw
        t = torch.from_numpy(base).to(DEV)
        bs = list(base.strides)
        ptr = t.data_ptr() + (shape[ax] - 1) * bs[ax]
        bs[ax] = -bs[ax]
        out.append((f'flip_axis{ax}', Raw(t, ptr, shape, bs, base.dtype.str), np.flip(base, ax)))
    return out


# ---- 1. import is exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('np_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', SHAPES)
def test_import_is_exact(ctx, shape, np_dtype):
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    for gather_only in (0, _lib.XB_CHECK_IO_GATHER):             # the LDS tile, then the plain gather, on permuted layouts
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, gather_only)
        try:
            for name, arr, host in layouts(shape, np_dtype, seed=sum(shape)):
                ctx.import_density(arr)
                want = np.ascontiguousarray(host).astype(np.float64)
                try:
                    assert_same_bits(ctx.download_density(), want)
                except AssertionError as e:
                    raise AssertionError(f'{name} {np.dtype(np_dtype).name} {shape} option {gather_only}: {e}') from None
        finally:
            ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)


def test_import_of_an_unaligned_contiguous_float32_view(ctx):
    """a contiguous float32 array whose pointer is not 16-byte aligned and whose size is no multiple of four"""
    shape = (33, 17, 50)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    n = int(np.prod(shape))
    base = special_values((n + 3,), np.float32, 7)
    t = torch.from_numpy(base).to(DEV)
    for off in (0, 1, 3):
        ctx.import_density(t[off:off + n].view(*shape))
        assert_same_bits(ctx.download_density(), base[off:off + n].reshape(shape).astype(np.float64))


# ---- 2. same answers as the host path ------------------------------------------------------------------------------------
def load_case(name):
    if name.startswith('r'):
        g, rho = load_rough(name)
        atoms = np.asarray(g['atoms_cart'])
    else:
        g = load_golden(name)
        rho = case_density(g)
        atoms = synth.atoms_cartesian(g['atoms'], g['lattice'])
    tol = float(g['vacuum_tol'])
    return g, rho, atoms, ({} if np.isnan(tol) else {'vacuum_tol': tol})



EXACT = ('bader_maxima', 'bader_atoms', 'bader_distance', 'atoms_surface_distance')
SUMS = ('bader_charge', 'bader_volume', 'atoms_charge', 'atoms_volume')


def compare_runs(dev, host, maps):
    for slot in maps:
        d, h = getattr(dev, slot), getattr(host, slot)
        assert isinstance(d, device.DeviceArray) and isinstance(h, np.ndarray), slot
        assert d.dtype == h.dtype and d.shape == h.shape, slot
        assert np.array_equal(d.to_host(), h), slot
    for slot in EXACT:
        assert np.array_equal(getattr(dev, slot), getattr(host, slot)), slot
    for slot in SUMS:
        if hasattr(host, slot):
            np.testing.assert_allclose(getattr(dev, slot), getattr(host, slot), rtol=1e-12, atol=1e-12, err_msg=slot)
    assert (dev.vacuum_charge, dev.vacuum_volume) == pytest.approx((host.vacuum_charge, host.vacuum_volume), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize('name', ['c40x48x56_tric', 'c64_cubic', 'c48_cubic_vac', 'r48_sig5_vac', 'c128_216atoms'])
def test_bader_on_a_device_density_equals_the_host_run(name):
    thread_handlers.VERBOSE = False
    g, rho, atoms, kw = load_case(name)
    for np_dtype in (np.float64, np.float32):
        src = rho.astype(np_dtype)
        host = Bader({'charge': src.astype(np.float64)}, g['lattice'], atoms, **kw)
        host()
        host_log = thread_handlers.refine.last_log
        dev = Bader({'charge': torch.from_numpy(src).to(DEV)}, g['lattice'], atoms, **kw)
        dev()
        assert thread_handlers.refine.last_log == host_log
        compare_runs(dev, host, ('bader_volumes', 'atoms_volumes'))
        if name == 'c64_cubic' and np_dtype is np.float64:
            assert np.array_equal(dev.bader_volumes.to_host(), g['ng_changed_2'])       # the golden map the parity tests pin
    # the speed profile: assignment, atom map, refinement of the atom map
    host = Bader({'charge': rho}, g['lattice'], atoms, speed_flag=True, **kw)
    host()
    host_log = thread_handlers.refine.last_log
    dev = Bader({'charge': torch.from_numpy(rho).to(DEV)}, g['lattice'], atoms, speed_flag=True, **kw)
    dev()
    assert thread_handlers.refine.last_log == host_log and not hasattr(dev, 'bader_volumes')
    compare_runs(dev, host, ('atoms_volumes',))


def test_a_permuted_float32_density_through_the_same_named_calls():
    """vacuum_assign / bader_calc / refine / charge_sum / assign_to_atoms / surface_distance / volume_mask one by one, the density a
    permuted float32 tensor, the label maps handed on as device arrays and as torch tensors"""
    thread_handlers.VERBOSE = False
    g, rho, atoms, _ = load_case('c40x48x56_tric')
    src = rho.astype(np.float32)
    wide = src.astype(np.float64)
    t = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0)
    assert tuple(t.shape) == rho.shape and not t.is_contiguous()
    dm, tg, vv = g['dist_mat'], g['T_grad'], float(g['voxel_volume'])
    hv, hc, hvol = utils.vacuum_assign(wide, np.zeros(rho.shape, np.int32), np.float64('nan'), wide, vv)
    dv, dc, dvol = utils.vacuum_assign(t, None, np.float64('nan'), t, vv)
    assert isinstance(dv, device.DeviceArray) and dv.dtype == np.dtype(dtype_calc(-rho.size)) and (dc, dvol) == (hc, hvol)
    hmax, hlab = thread_handlers.bader_calc('neargrid', wide, hv, dm, tg, 1)
    dmax, dlab = thread_handlers.bader_calc('neargrid', t, dv, dm, tg, 1)
    assert np.array_equal(dmax, hmax) and dlab.dtype == hlab.dtype and np.array_equal(dlab.to_host(), hlab)
    lab_t = torch.as_tensor(dlab, device=DEV)                  # a torch view of the result, handed back in
    thread_handlers.refine('neargrid', ('all', -1), wide, hlab, dm, tg, 1)
    host_log = thread_handlers.refine.last_log
    thread_handlers.refine('neargrid', ('all', -1), t, lab_t, dm, tg, 1)
    assert thread_handlers.refine.last_log == host_log and np.array_equal(lab_t.cpu().numpy(), hlab)
    n = hmax.shape[0]
    hch, hvo, dch, dvo = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    utils.charge_sum(hch, hvo, vv, wide, hlab)
    utils.charge_sum(dch, dvo, vv, t, lab_t)
    np.testing.assert_allclose(dch, hch, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dvo, hvo, rtol=1e-12, atol=1e-12)
    hm = utils.volume_mask(hlab, wide, 1)
    dmask = utils.volume_mask(lab_t, t, 1)
    assert isinstance(dmask, device.DeviceArray) and dmask.dtype == np.float64 and np.array_equal(dmask.to_host(), hm)
    bmax_cart = np.dot(np.divide(hmax, rho.shape), g['lattice'])
    ha, hd, hav = thread_handlers.assign_to_atoms(bmax_cart, atoms, g['lattice'], hlab, 1)
    da, dd, dav = thread_handlers.assign_to_atoms(bmax_cart, atoms, g['lattice'], lab_t, 1)
    assert np.array_equal(da, ha) and np.array_equal(dd, hd) and dav.dtype == hav.dtype and np.array_equal(dav.to_host(), hav)
    hs = thread_handlers.surface_distance(wide, hav, g['lattice'], atoms, 1)
    ds = thread_handlers.surface_distance(t, dav, g['lattice'], atoms, 1)
    assert np.array_equal(ds, hs)


# ---- 3. results are device arrays of the right kind ------------------------------------------------------------------------
def test_results_are_device_arrays_torch_wraps_without_a_copy():
    thread_handlers.VERBOSE = False
    g, rho, atoms, _ = load_case('c64_cubic')
    t = torch.from_numpy(rho).to(DEV)
    bmax, lab = thread_handlers.bader_calc_refine('neargrid', 'neargrid', ('changed', 2), t, None, g['dist_mat'], g['T_grad'], 1)
    assert isinstance(bmax, np.ndarray) and isinstance(lab, device.DeviceArray)
    assert lab.dtype == np.dtype(dtype_calc(-bmax.shape[0])) and lab.shape == rho.shape
    wrapped = torch.as_tensor(lab, device=DEV)
    assert wrapped.data_ptr() == lab.__cuda_array_interface__['data'][0] == lab.ptr
    assert tuple(wrapped.shape) == rho.shape and np.array_equal(wrapped.cpu().numpy(), g['ng_changed_2'])
    again = device.describe(lab)
    assert again.c_contiguous and again.dtype == lab.dtype and not again.readonly
    ptr = lab.ptr
    del lab                                                       # the wrapper keeps the memory alive
    assert wrapped.data_ptr() == ptr and np.array_equal(wrapped.cpu().numpy(), g['ng_changed_2'])


def test_export_labels_and_volume_into_the_callers_tensors(ctx):
    g = load_golden('c64_cubic')
    rho = case_density(g)
    ctx.set_grid(rho.shape, g['dist_mat'], g['T_grad'])
    ctx.upload_density(rho)
    ctx.vacuum_assign(None, 1.0)
    ctx.assign('neargrid')
    for tdt, ndt in ((torch.int8, np.int8), (torch.int16, np.int16), (torch.int32, np.int32), (torch.int64, np.int64)):
        out = torch.full(rho.shape, 77, dtype=tdt, device=DEV)
        assert ctx.export_labels(out=out) is out
        assert np.array_equal(out.cpu().numpy(), ctx.download_labels(ndt))
        flat = torch.full((rho.size + 3,), 77, dtype=tdt, device=DEV)       # a destination that is not 16-byte aligned
        view = flat[1:1 + rho.size].view(*rho.shape)
        ctx.export_labels(out=view)
        assert np.array_equal(view.cpu().numpy(), ctx.download_labels(ndt))
        assert flat[0].item() == 77 and flat[-1].item() == 77 and flat[-2].item() == 77
    want = ctx.volume_mask(3)
    o64 = torch.empty(rho.shape, dtype=torch.float64, device=DEV)
    ctx.export_volume(3, out=o64)
    assert np.array_equal(o64.cpu().numpy().view(np.uint64), want.view(np.uint64))
    o32 = torch.empty(rho.shape, dtype=torch.float32, device=DEV)
    ctx.export_volume(3, out=o32)
    assert np.array_equal(o32.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    own = ctx.export_volume(3, dtype=np.float32)
    assert isinstance(own, device.DeviceArray) and np.array_equal(own.to_host(), want.astype(np.float32))


@pytest.mark.parametrize('tdt', [torch.int8, torch.int16, torch.int32, torch.int64])
def test_import_labels_then_refine_equals_refine_of_the_uploaded_map(ctx, tdt):
    g = load_golden('c64_cubic')
    rho = case_density(g)
    ctx.set_grid(rho.shape, g['dist_mat'], g['T_grad'])
    ctx.upload_density(rho)
    ctx.upload_labels(g['ng_main'])
    want_log = ctx.refine('changed', 2)
    want = ctx.download_labels(np.int32)
    ctx.import_labels(torch.from_numpy(np.ascontiguousarray(g['ng_main'])).to(DEV).to(tdt))
    assert np.array_equal(ctx.download_labels(np.int32), g['ng_main'])
    assert ctx.refine('changed', 2) == want_log
    assert np.array_equal(ctx.download_labels(np.int32), want) and np.array_equal(want, g['ng_changed_2'])


# ---- 4. ordering -------------------------------------------------------------------------------------------------------
def test_ordering_against_the_producers_stream():
    """The density is the end of a chain of torch kernels on a non-default stream (128 rolls by one plane: every
    intermediate is a shifted density, whose maxima and labels differ), handed in with no synchronisation; the label tensor
    is reduced by torch on that stream right after the call.  Both results must equal a fully synchronised run's.
    A CHECK, NOT A PROOF: without the events the kernels might still happen to run in the right order and this test
    would pass by luck; what it guards against is an ordering that is plainly absent."""
    thread_handlers.VERBOSE = False
    g, rho, atoms, _ = load_case('c128_216atoms')
    args = ('neargrid', 'neargrid', ('changed', 2))
    base = torch.from_numpy(rho).to(DEV)
    weights = torch.arange(rho.size, dtype=torch.int64, device=DEV).view(*rho.shape) % 1009

    def produce():
        t = base
        for _ in range(rho.shape[0]):
            t = torch.roll(t, 1, 0)
        return t

    torch.cuda.synchronize()
    t = produce()
    torch.cuda.synchronize()
    smax, slab = thread_handlers.bader_calc_refine(*args, t, None, g['dist_mat'], g['T_grad'], 1)
    torch.cuda.synchronize()
    want_sum = int((torch.as_tensor(slab, device=DEV).to(torch.int64) * weights).sum().item())
    want_lab = slab.to_host()
    del t, slab
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), device.on_stream(stream.cuda_stream):
        t = produce()
        amax, alab = thread_handlers.bader_calc_refine(*args, t, None, g['dist_mat'], g['T_grad'], 1)
        total = (torch.as_tensor(alab, device=DEV).to(torch.int64) * weights).sum()
        got_sum = int(total.item())                                # (read on the same stream)
    assert np.array_equal(amax, smax) and np.array_equal(amax, g['ng_bader_max'])
    assert got_sum == want_sum
    with device.on_stream(stream.cuda_stream):
        assert np.array_equal(alab.to_host(), want_lab)


# ---- 5. errors cost nothing ------------------------------------------------------------------------------------------------
def segment_of(ptr):
    for seg in torch.cuda.memory_snapshot():
        if seg['address'] <= ptr < seg['address'] + seg['total_size']:
            return seg['address'], seg['address'] + seg['total_size']
    raise AssertionError('no segment of the caching allocator holds the tensor')


def test_errors_are_error_codes_and_cost_nothing(ctx):
    """every refusal is XB_E_ARG from the host-side checks (nothing is queued for a refused call: host_interop.h checks
    first), and the context works on as before"""
    shape = (20, 24, 28)
    nx, ny, nz = shape
    n = nx * ny * nz
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    good_np = special_values(shape, np.float64, 11)
    good = torch.from_numpy(good_np).to(DEV)
    labels = torch.zeros(shape, dtype=torch.int32, device=DEV)

    def refused(call, *args, **kw):
        with pytest.raises(_lib.BaderHipError) as e:
            call(*args, **kw)
        assert e.value.code == _lib.XB_E_ARG, e.value
        ctx.import_density(good)                                   # the next valid call on the same context succeeds
        assert_same_bits(ctx.download_density(), good_np)
        ctx.import_labels(labels)
        assert not ctx.download_labels(np.int32).any()

    refused(ctx.import_density, Raw(good_np, good_np.ctypes.data, shape, None, '<f8'))                # a host pointer
    refused(ctx.export_labels, out=Raw(good_np, good_np.ctypes.data, shape, None, '<i4'))
    lo, hi = segment_of(good.data_ptr())
    # every second x-plane (a stride of two planes): placed so that its last element is the last of the allocation it is
    # taken, ONE element further it is refused; the same at the front with a flipped z axis
    strides = (8 * 2 * ny * nz, 8 * nz, 8)
    span = 8 * ((nx - 1) * 2 * ny * nz + ny * nz)
    assert hi - span >= lo
    ctx.import_density(Raw(good, hi - span, shape, strides, '<f8'))
    refused(ctx.import_density, Raw(good, hi - span + 8, shape, strides, '<f8'))
    flipped = (8 * ny * nz, 8 * nz, -8)
    ctx.import_density(Raw(good, lo + 8 * (nz - 1), shape, flipped, '<f8'))
    refused(ctx.import_density, Raw(good, lo + 8 * (nz - 2), shape, flipped, '<f8'))
    refused(ctx.import_density, Raw(good, good.data_ptr(), shape, (2 ** 62, 8 * nz, 8), '<f8'))
    refused(ctx.import_density, Raw(good, good.data_ptr(), shape, (-2 ** 62, 8 * nz, 8), '<f8'))
    refused(ctx.import_density, torch.zeros((20, 24, 29), dtype=torch.float64, device=DEV))          # not the grid's shape
    refused(ctx.import_labels, torch.zeros((20, 24), dtype=torch.int32, device=DEV))
    refused(ctx.import_density, torch.zeros(shape, dtype=torch.float16, device=DEV))                 # float16
    refused(ctx.import_density, labels)                                                              # labels are no density
    refused(ctx.export_volume, 0, out=labels)
    refused(ctx.export_labels, out=Raw(labels, labels.data_ptr(), shape, None, '<i4', readonly=True))   # a read-only destination
    refused(ctx.export_labels, out=torch.zeros((28, 24, 20), dtype=torch.int32, device=DEV).permute(2, 1, 0))   # not contiguous
    resident = Raw(ctx, ctx.lib.xb_labels_ptr(ctx.h), shape, None, '<i4')
    refused(ctx.export_labels, out=resident)                                                         # aliases the resident labels
    refused(ctx.import_labels, resident)
    refused(ctx.import_density, Raw(ctx, ctx.lib.xb_density_ptr(ctx.h), shape, None, '<f8'))
    fresh = _lib.Context(0)                                                                          # no grid yet
    try:
        with pytest.raises(_lib.BaderHipError) as e:
            fresh.shape = shape
            fresh.import_density(good)
        assert e.value.code == _lib.XB_E_ARG
    finally:
        fresh.close()


# ---- 6. host waits -----------------------------------------------------------------------------------------------------
def test_host_waits_of_a_device_side_run_do_not_exceed_the_host_sides():
    thread_handlers.VERBOSE = False
    g, rho, atoms, _ = load_case('c64_cubic')
    ctx = _lib.default_context()
    args = ('neargrid', 'neargrid', ('changed', 2))
    t = torch.from_numpy(rho).to(DEV)
    counts = {}
    for rounds in range(2):                                         # (the first round allocates; the second is the steady state)
        w0 = ctx.host_waits()
        thread_handlers.bader_calc_refine(*args, rho, np.zeros(rho.shape, np.int32), g['dist_mat'], g['T_grad'], 1)
        w1 = ctx.host_waits()
        thread_handlers.bader_calc_refine(*args, t, torch.zeros(rho.shape, dtype=torch.int32, device=DEV), g['dist_mat'], g['T_grad'], 1)
        w2 = ctx.host_waits()
        thread_handlers.bader_calc_refine(*args, t, None, g['dist_mat'], g['T_grad'], 1)
        w3 = ctx.host_waits()
        counts = {'host': w1 - w0, 'device': w2 - w1, 'device, no map handed in': w3 - w2}
        print('host waits per bader_calc_refine:', counts)
    assert counts['device'] <= counts['host'] and counts['device, no map handed in'] <= counts['device']
    hb = Bader({'charge': rho}, g['lattice'], atoms)
    w0 = ctx.host_waits()
    hb()
    w1 = ctx.host_waits()
    Bader({'charge': t}, g['lattice'], atoms)()
    w2 = ctx.host_waits()
    print('host waits per Bader run: host', w1 - w0, 'device', w2 - w1)
    assert w2 - w1 <= w1 - w0

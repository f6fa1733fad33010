"""Elongated grids (surface slabs, wires), where the kernel forms chosen from a grid's SHAPE meet: the 512-voxel windows of the
packed walker, the 24-bit index products, the 32-bit record offsets of the lean kernels and the tile counts that become gridDim.y
and gridDim.z.  tests/elongated_common.py builds the densities and names the shapes; tests/test_elongated_cpu.py pins the
constructions to the CPU oracle and the shapes to the thresholds as the sources state them.  Every comparison is exact.

    window seams     the long walk on x, y and z at 504, 512, 520 and 640 voxels, 1032 on x; the tile density on 528 x 528 x 16
                     (window origins non-zero in x and y at once): four forms -- cross-check 0, XB_CHECK_BRICK_LOOKUP,
                     XB_CHECK_GENERIC_WALKER, XB_CHECK_GENERIC_RETRACE -- equal to each other and to the oracle
    16 x 16 x 524288     N == 2^27: packed walker and lean retrace with 32-bit record offsets up to 2^32 - 32
    512 x 512 x 528      N == 2^27 + 2^22: packed walker with 64-bit offsets, generic retrace
    4096 x 4080 x 16     x * ny + y up to 16 711 679: the top of the 24-bit operand; packed walker, generic retrace
    4096 x 4096 x 16     nx * ny == 2^24: use24 off; generic walker under cross-check 0, generic retrace
    per-axis limits      a longer x or y axis than the tile launches' gridDim.z / gridDim.y allow is refused by xb_set_grid; the
                         longest accepted 16 x 16 cross-sections (derived from what the context reads) give the predicted map
    walk list            16 x 16 x 8192, 16 x 16 x 8200, 8208 x 16 x 16: the last axis a Morton code of the walk list holds, and beyond
nz >= 2^24, the other half of use24, cannot be reached below the int32 limit with 16-voxel axes (16 * 16 * 2^24 == 2^32), and
below 16 voxels an assignment leaves no region labels and the lean kernels are never chosen: not chased.

The big shapes have no oracle run.  Their expectation is the tile predictor (elongated_common.predicted_maxima): the library's
`maxima_lin[labels]` against it in slabs of x-planes (bounded host memory), maxima() as a set against the lifted tile maxima, and
the numbering without a sort -- a label is at most one above the largest label before it in C order, which with the two
equalities above is the numbering by first voxel.  Refinement logs are the closed form of elongated_common.tile_logs.

What the first run on an MI355X showed.  A BUG: every grid with an axis of more than 8192 voxels was assigned wrongly, without an
error -- 16 x 16 x 524288 came back with 64 basins instead of 65 536, 16 x 524288 x 16 with 34, 262144 x 16 x 16 with 20 of 32 768.
The walk list enumerates Morton codes of the brick coordinates, `1u << 3 * bits` of them; from 11 bits per axis on that count
wraps (and compact3 unpacks ten bits), so the list held a few bricks of the grid's corner and the rest was never traced.  Such grids
now take the list in linear brick order (host_stages.h, launch_walk_list); the three walk-list cases keep the bound.  Everything
else equalled its reference at once.  After the fix (slow_path_stats (0, 0) everywhere, no retrace on an overflow list):
    long walks, all 13: 2 basins, box_stats (0, 0); per form 2 traces of the form's walker (packed and lookup with 32-bit offsets)
        and 2 first retraces -- lean under cross-check 0 and XB_CHECK_GENERIC_WALKER, generic under XB_CHECK_BRICK_LOOKUP and
        XB_CHECK_GENERIC_RETRACE; logs [(64 L, 0), (0, 0)]; 0.9 s per case, 1.4 s at 640, 4.1 s at 1032 (the oracle)
    528 x 528 x 16: n_maxima 2178, box_stats (2178, 0), 3 first retraces per form, log [(2108304, 0), (0, 0)]; 2.1 s
    shape              n_maxima  box_stats    traces  offsets  first retraces  log                        wall / card
    16 x 16 x 524288     65 536  (65535, 0)   packed  32 bit   3 lean          [(33554432, 0), (0, 0)]    25.0 s / 0.08 s  (three forms)
    512 x 512 x 528      67 584  (65535, 0)   packed  64 bit   3 generic       [(65421312, 0), (0, 0)]    10.5 s / 0.09 s  (three forms)
    4096 x 4080 x 16    130 560  (65535, 0)   packed  64 bit   3 generic       [(126382080, 0), (0, 0)]    9.6 s / 0.08 s
    4096 x 4096 x 16    131 072  (65535, 0)   generic  --      3 generic       [(126877696, 0), (0, 0)]   10.9 s / 0.08 s
    262144 x 16 x 16     32 768  (32768, 0)   packed  32 bit   3 lean          [(25657344, 0), (0, 0)]     5.5 s / 0.02 s
    16 x 524288 x 16     65 536  (65535, 0)   packed  32 bit   3 lean          [(51118080, 0), (0, 0)]     5.8 s / 0.04 s
    (2 traces per form everywhere; under XB_CHECK_GENERIC_WALKER 2 generic traces, under XB_CHECK_GENERIC_RETRACE 3 generic retraces;
    box_stats: every region dies in the kill iteration -- a basin is its tile shifted by (6, 7, 3), no brick lies inside one -- so
    every voxel is walked; `card` is the wall time of assign + refine + assign_refine, the rest is the host: tiling, upload and the
    slab-wise comparison of nine (three) maps)
    axis limits read from the device: nx <= 262 144, ny <= 524 288 (maxGridSize 65 536 for y and z); the walk-list cases 0.1 - 0.3 s
16 x 16 x 524288 is the one case above 20 s: 2^27 voxels is the threshold itself, and it runs the three forms the issue asks for, nine
maps of 2^27 labels compared on the host; the card's share is 0.08 s.

No mutation was run.  The two that merely change which kernel is chosen -- `c->N <= (1LL << 27)` with `<`, use24 with `<=` -- leave
every map right (at 4096 x 4096 x 16 x * ny + y still fits 24 bits) and fail assert_kernels alone, by reading it.  The forms that
read or write out of bounds -- from the code:
    pw_rebase with nb1 / nb2 swapped (bader_kernels.h): the window's brick index wb decomposes as (wb / nb2) / nb1, (wb / nb2) %
        nb1, wb % nb2; swapped, a y-long grid (nb1 = 64 at 16 x 512 x 16, nb2 = 2) would take by = (wb / 64) % 2 and rebuild lb
        from a brick up to 63 * 8 voxels off on y: the record offsets it then forms lie outside the brick's window and, at the far
        end of the grid, outside the table.  Every y- and x-long seam case here would differ from the oracle before that.
    the 32-bit offset form above 2^27 (host_stages.h, `wlen * nyz <= 1 << 27 ? 4 : 3`; k_edges.h, `(unsigned)l << 5`): at
        512 x 512 x 528 the records of the last 2^22 voxels have offsets from 2^32 on, which wrap to the table's first 128 MiB --
        reads of other voxels' records, and walkers that follow them anywhere: those voxels' maxima would differ from the
        predictor; the lean retrace also writes labels through such an offset.  16 x 16 x 524288 holds the form at its last offset.
    a per-axis limit one tile too generous: gridDim.z = 65 537 is refused by the launch or not, which is the question the issue
        forbids to put to the card; the refusal test reads the limit and the message instead."""
import time

import numpy as np
import pytest

import torch  # noqa: F401  (before the library: see conftest)
import elongated_common as ec
from pybader_amd import _lib

pytestmark = pytest.mark.gpu

MODE = ('changed', 2)
FORMS = {'default': 0, 'lookup': _lib.CROSS_CHECK_BRICK_LOOKUP, 'generic_walker': _lib.XB_CHECK_GENERIC_WALKER,
         'generic_retrace': _lib.CROSS_CHECK_GENERIC_RETRACE}


def assert_same(got, want, what):
    """np.array_equal, and on a mismatch where the two differ"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    where = [tuple(int(c) for c in np.unravel_index(i, got.shape)) for i in diff[:8]]
    first = [(w, int(got[w]), int(want[w])) for w in where]
    raise AssertionError(f'{what}: {diff.size} of {got.size} entries differ, first (index, library, expected): {first}')


def counters(c):
    """(packed, lookup, generic traces; lean traces with 32-bit, with 64-bit offsets; lean, generic first retraces; slow path of
    the assignment, of the refinement)"""
    return c.trace_stats() + c.trace_offset_stats() + c.retrace_stats() + c.slow_path_stats()


def delta(c, before):
    return tuple(int(a) - int(b) for a, b in zip(counters(c), before))


def assert_kernels(d, bits, want, what):
    """d: what the calls added to counters(); want: ec.forms(shape).  Under cross-check 0 the walker, its offset form and the retrace
    kernel are the shape's; under a cross-check bit the replaced kernel must not have run."""
    packed, off32, lean = want
    tp, tl, tg, o32, o64, rl, rg = d[:7]
    assert tp + tl + tg >= 1 and rl + rg >= 1, (what, d)
    if bits & _lib.XB_CHECK_GENERIC_WALKER or not packed:
        assert tp == tl == 0 and o32 == o64 == 0, (what, d)
    elif bits & _lib.CROSS_CHECK_BRICK_LOOKUP:
        assert tp == tg == 0, (what, d)
    else:
        assert tl == tg == 0, (what, d)
    if packed and not bits & _lib.XB_CHECK_GENERIC_WALKER:
        assert (o32, o64) == ((tp + tl, 0) if off32 else (0, tp + tl)), (what, d)
    if bits & _lib.CROSS_CHECK_GENERIC_RETRACE or not lean:
        assert rl == 0, (what, d)
    elif bits == 0:
        assert rl >= 1 and rg == 0, (what, d)


# ---- the tile density against its predictor, in slabs ------------------------------------------------------------------------

_density = {}


def density(shape):
    """one tiled density at a time (2 GiB at the largest shape)"""
    if shape not in _density:
        _density.clear()
        _density[shape] = ec.tiled_density(shape)
    return _density[shape]


def check_tile_map(ctx, shape, what):
    """the resident labels and maxima of a neargrid assignment of the tile density against the predictor"""
    n = ctx.n_maxima
    assert n == ec.n_tiles(shape), (what, n, ec.n_tiles(shape))
    mx = ctx.maxima()
    assert_same(ec.sort_rows(mx), ec.lifted_maxima(shape), what + ': maxima as a set')
    maxima_lin = np.ravel_multi_index(tuple(mx.T), shape).astype(np.int32)
    nx, ny, nz = shape
    planes = max(1, (1 << 23) // (ny * nz))
    buf = np.empty((planes, ny, nz), np.int32)
    wrong, first, order, running = 0, [], [], -1
    for xa in range(0, nx, planes):
        xb = min(nx, xa + planes)
        lab = buf[:xb - xa]
        ctx.copy_planes(0, 0, lab, xa, xb)
        assert lab.min() >= 0 and lab.max() < n, (what, xa, int(lab.min()), int(lab.max()), n)
        got, want = maxima_lin[lab], ec.predicted_maxima(shape, xa, xb)
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        wrong += bad.size
        for i in bad[:8 - len(first)]:
            w = np.unravel_index(i, lab.shape)
            first.append(((xa + int(w[0]), int(w[1]), int(w[2])), int(got[w]), int(want[w])))
        flat = lab.reshape(-1)
        top = np.maximum(np.maximum.accumulate(flat), running)
        before = np.concatenate(([running], top[:-1]))
        jump = np.flatnonzero(flat > before + 1)
        order += [(xa * ny * nz + int(i), int(flat[i]), int(before[i])) for i in jump[:4 - len(order)]]
        running = int(top[-1])
    assert not wrong, f'{what}: the maximum of {wrong} of {ec.n_voxels(shape)} voxels differs, first (voxel, library, expected): {first}'
    assert not order and running == n - 1, f'{what}: labels are not numbered by first voxel, first (voxel, label, largest before): {order}, last {running}'


def run_tile_shape(shape, forms):
    """assign, refine and assign_refine of the tile density on `shape` under each cross-check form: every map against the predictor,
    every log against the closed form, the kernels that ran against what the shape selects"""
    t0 = time.time()
    want = ec.forms(shape)
    rho = density(shape)
    card = 0.0
    ctx = _lib.Context(0)
    try:
        ctx.set_grid(shape, *ec.matrices(shape))
        ctx.upload_density(rho)
        log_want = ec.tile_logs(shape)[MODE]
        for form in forms:
            bits = FORMS[form]
            what = f'{ec.ids(shape)} {form}'
            ctx.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
            before = counters(ctx)
            ctx.vacuum_assign(None, 1.0)
            t = time.time()
            n = ctx.assign('neargrid')
            card += time.time() - t
            stats = ctx.box_stats()
            check_tile_map(ctx, shape, what + ' assign')
            t = time.time()
            log = ctx.refine(*MODE)
            card += time.time() - t
            assert log == log_want, (what, log, log_want)
            check_tile_map(ctx, shape, what + ' refine')
            ctx.vacuum_assign(None, 1.0)
            t = time.time()
            n2, log2 = ctx.assign_refine('neargrid', *MODE)
            card += time.time() - t
            assert n2 == n and log2 == log_want, (what, n2, log2, log_want)
            check_tile_map(ctx, shape, what + ' assign_refine')
            d = delta(ctx, before)
            print(f'{what}: n_maxima {n}, box_stats {stats}, traces (packed, lookup, generic) {d[:3]}, lean offsets (32, 64 bit) {d[3:5]}, '
                  f'first retraces (lean, generic) {d[5:7]}, slow path (assign, refine) {d[7:]}, log {log}')
            assert_kernels(d, bits, want, what)
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
        print(f'{ec.ids(shape)}: {time.time() - t0:.1f} s, of which {card:.2f} s in assign / refine / assign_refine; memory {ctx.memory_stats()[0] / 2**30:.2f} GiB')
    finally:
        ctx.close()


@pytest.mark.parametrize('shape', list(ec.THRESHOLD_SHAPES), ids=ec.ids)
def test_thresholds_crossed_with_the_tile_density(shape):
    """2^27 voxels and just above; the top of the 24-bit operand and nx * ny == 2^24.  The first two also under the generic retrace
    and the generic walker."""
    assert ec.forms(shape) == ec.THRESHOLD_SHAPES[shape]
    small = ec.n_voxels(shape) <= ec.LEAN_VOXELS + (1 << 22)
    run_tile_shape(shape, ('default', 'generic_retrace', 'generic_walker') if small else ('default',))


@pytest.mark.parametrize('shape', ec.MORTON_SHAPES, ids=ec.ids)
def test_walk_list_order_beyond_the_morton_codes(shape):
    """1024 bricks on an axis are the last the walk list's Morton codes hold; an axis of 1025 (z) or 1026 (x) bricks takes the
    list in linear order.  (Found by this module's first run: the code count `1u << 3 * bits` wrapped from 11 bits per axis on, the
    list held a few bricks of the grid's corner and 16 x 16 x 524288 came back with 64 of its 65 536 basins.)"""
    run_tile_shape(shape, ('default',))


# ---- per-axis limits -------------------------------------------------------------------------------------------------------

def test_axis_limits_fail_loudly_and_leave_the_context_usable():
    """a longer x or y axis than the tile launches' gridDim allows: XB_E_LIMIT from xb_set_grid, with the axis and the limit in the
    message, before anything is allocated and without a launch; z has no limit of its own; the context then works"""
    ctx = _lib.Context(0)
    nx_max, ny_max = ctx.axis_limits()
    print('axis limits (nx, ny):', nx_max, ny_max)
    assert nx_max >= 1024 and ny_max >= 1024 and nx_max % ec.RELABEL_X == 0 and ny_max % ec.BRK == 0
    dm, tg = ec.matrices((16, 16, 16))
    ctx.set_grid((16, 16, 16), dm, tg)
    held = ctx.memory_stats()[0]
    for axis, limit in ((0, nx_max), (1, ny_max)):
        shape = [3, 3, 3]
        shape[axis] = limit + 1
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.set_grid(tuple(shape), dm, tg)
        print('refusal:', e.value)
        assert e.value.code == _lib.XB_E_LIMIT
        assert f'axis {"xy"[axis]} of {limit + 1} voxels' in str(e.value) and f'limit of {limit} voxels on {"xy"[axis]}' in str(e.value)
        assert ctx.memory_stats()[0] == held, 'refused before anything is allocated'
    shape = [3, 3, 3]
    shape[0] = nx_max                 # the limit itself is accepted (no tile launch here: the longest-axis tests run those)
    ctx.set_grid(tuple(shape), dm, tg)
    ctx.set_grid((3, 3, 2 * max(nx_max, ny_max)), dm, tg)     # z: no limit of its own
    small = (32, 48, 24)
    ctx.set_grid(small, *ec.matrices(small))
    ctx.upload_density(ec.tiled_density(small))
    ctx.vacuum_assign(None, 1.0)
    ctx.assign('neargrid')
    check_tile_map(ctx, small, 'after the refusals')
    ctx.close()


@pytest.mark.parametrize('axis', [0, 1], ids=['x', 'y'])
def test_longest_accepted_axis_gives_the_predicted_map(axis):
    """the longest x- and y-elongated grids of whole tiles with a 16 x 16 cross-section that xb_set_grid accepts (262144 x 16 x 16
    and 16 x 524288 x 16 where the device bounds gridDim.y and gridDim.z by 65 536): gridDim.z / gridDim.y of the edge sweep, the
    relabel and pass A at their largest"""
    ctx = _lib.Context(0)
    limits = ctx.axis_limits()
    ctx.close()
    shape = ec.longest_shapes(*limits)[axis]
    print('longest accepted', 'xy'[axis], 'axis:', shape, 'of the limit', limits[axis])
    assert shape[axis] <= limits[axis] and (shape[axis] + ec.TILE[axis] > limits[axis] or ec.n_voxels(shape) == 1 << 27)
    run_tile_shape(shape, ('default',))


# ---- window seams: the long walk on every axis, four forms, the oracle --------------------------------------------------------

@pytest.fixture(scope='module')
def seam_ctx():
    c = _lib.Context(0)
    c.set_option(_lib.XB_OPT_DEBUG, _lib.DEBUG_KEEP_RETRACE_OVERFLOW)
    yield c
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    c.set_option(_lib.XB_OPT_DEBUG, 0)
    c.close()
    _density.clear()


def run_form(c, rho, dm, tg, bits):
    """assign + refine, then both in one call, under one cross-check form: the results to compare and what the calls added to
    counters() and deferred_stats()"""
    c.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
    c.retrace_overflow()
    before, deferred = counters(c), c.deferred_stats()
    c.set_grid(rho.shape, dm, tg)
    c.upload_density(rho)
    c.vacuum_assign(None, 1.0)
    n = c.assign('neargrid')
    res = {'n': n, 'maxima': np.ravel_multi_index(tuple(c.maxima().T), rho.shape), 'assign': c.download_labels(np.int32), 'box_stats': c.box_stats()}
    res['log'] = c.refine(*MODE)
    res.update(refined=c.download_labels(np.int32), known=c.download_known(), overflow=np.sort(c.retrace_overflow()))
    c.vacuum_assign(None, 1.0)
    n2, log2 = c.assign_refine('neargrid', *MODE)
    res.update(fused_n=n2, fused_log=log2, fused=c.download_labels(np.int32), fused_overflow=np.sort(c.retrace_overflow()))
    d = delta(c, before)
    res['slow_path'] = d[7:] + (c.deferred_stats() - deferred,)
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    return res, d


def run_all_forms(c, rho, dm, tg, o, what):
    """the four forms on one context: each equal to the default form item by item, the default form equal to the oracle's side `o`
    (maxima, assign, refined, log), and every form ran the kernels it stands for -- the lean retrace on every one of these shapes"""
    got = {}
    for form, bits in FORMS.items():
        got[form], d = run_form(c, rho, dm, tg, bits)
        print(f'{what} {form}: traces (packed, lookup, generic) {d[:3]}, lean offsets (32, 64 bit) {d[3:5]}, first retraces (lean, generic) {d[5:7]}, '
              f'slow path / deferred {got[form]["slow_path"]}, overflow {got[form]["overflow"].size}')
        assert_kernels(d, bits, (True, True, True), f'{what} {form}')
    a = got['default']
    for form in FORMS:
        for key, x in got[form].items():
            if isinstance(x, np.ndarray):
                assert_same(x, a[key], f'{what} {form} against the default form: {key}')
            else:
                assert x == a[key], (what, form, key, x, a[key])
    assert a['n'] == o['maxima'].shape[0] == a['fused_n']
    assert_same(a['maxima'], o['maxima'], what + ': maxima')
    assert_same(a['assign'], o['assign'], what + ': assignment')
    assert a['log'] == o['log'] == a['fused_log'], (what, a['log'], a['fused_log'], o['log'])
    assert_same(a['refined'], o['refined'], what + ': refined map')
    assert_same(a['fused'], o['refined'], what + ': map of assign_refine')
    return a


@pytest.mark.parametrize('axis,length', ec.SEAM_CASES, ids=lambda p: str(p))
def test_window_seams_on_every_axis(seam_ctx, axis, length):
    """lengths below, at and above one 512-voxel window, between one and two, and above two: pw_win's regimes (top = n - 512 is 0,
    0, 8, 128, 520), pw_rebase with the window's brick index decomposed along x, y and z, borrows out of the x field"""
    rho, dm, tg = ec.long_walk(axis, length)
    from rough_common import rank_labels
    lab, maxima = rank_labels(ec.oracle_own_map(rho, 0.1))
    refined, log = ec.oracle_refine(rho, lab, MODE, 0.1)
    assert maxima.shape[0] == 2 and np.all(np.unravel_index(maxima, rho.shape)[axis] == length - 10), 'two ridges, one maximum each'
    assert log == [(64 * length, 0), (0, 0)] and np.array_equal(refined, lab)
    o = {'maxima': maxima, 'assign': lab.astype(np.int32), 'refined': refined, 'log': log}
    a = run_all_forms(seam_ctx, rho, dm, tg, o, f'long walk axis {"xyz"[axis]} L {length}')
    assert a['box_stats'][1] == 0, 'no brick is certified: every voxel is walked'


def test_window_seams_in_two_fields_at_once(seam_ctx):
    """the tile density on 528 x 528 x 16: windows with non-zero origins on x and y together; against the oracle directly and
    against the tile predictor, which the big shapes rely on"""
    shape = ec.SEAM_TILE_SHAPE
    rho = density(shape)
    dm, tg = ec.matrices(shape)
    F = ec.oracle_own_map(rho)
    assert_same(F, ec.predicted_maxima(shape, 0, shape[0]), 'the oracle against the tile predictor')
    from rough_common import rank_labels
    lab, maxima = rank_labels(F)
    refined, log = ec.oracle_refine(rho, lab, MODE)
    assert log == ec.tile_logs(shape)[MODE] and np.array_equal(refined, lab)
    o = {'maxima': maxima, 'assign': lab.astype(np.int32), 'refined': refined, 'log': log}
    a = run_all_forms(seam_ctx, rho, dm, tg, o, ec.ids(shape))
    print(f'{ec.ids(shape)}: n_maxima {a["n"]}, box_stats {a["box_stats"]}')
    check_tile_map(seam_ctx, shape, ec.ids(shape) + ' against the predictor')

"""The fixed capacities of the assignment pipeline, crossed: one case below, one at and one above each count at which
xb_assign / xb_assign_refine switch to a second code path (tests/capacity_common.py names them and builds the two densities;
tests/test_capacity_cpu.py pins the constructions to the CPU oracle and the shapes to the counts).

    XB_BOXES_MAX   = 1024 regions   LDS tables of k_grow_finish / k_relabel_regions_brick, else global lookups
    XB_SORT_MAX    = 2048 maxima    k_number_maxima's LDS sort, else the bitmap numbering (k_rank_*); xb_assign_refine redoes
                                    the refinement iteration it queued behind an assignment that ended this way
    1024 block sums per round       k_rank_blocks' carry: more than 2^25 voxels with more than 2048 maxima
    XB_REGIONS_MAX = 65 535 seeds   further seed bricks get region id 0 and are walked
    max_cap        = 2^22 maxima    XB_E_LIMIT above it; the context stays usable

Every comparison is exact.  Density A has a closed-form map (every basin is its 8^3 brick), so the cases of 33 and 35 million
voxels need no oracle; density B's oracle maps are computed once per module.

What the first run on an MI355X showed (all 18 cases equal to their references; slow_path_stats is (assignment, refinement)):
    density A, every shape and method: n_maxima == bricks, box_stats == (min(bricks, 65 535), 512 * that), slow_path_stats (0, 0);
        bricks without a region: 0 up to 64 512 bricks, 1 at 65 536, 2 049 at 67 584; refinement logs [(296 * bricks, 0), (0, 0)]
        from xb_assign_refine and from xb_assign + xb_refine alike (2040, 2048 and 2057 maxima).
    density B, 256x512x256 ongrid: n_maxima 4 194 304, box_stats (0, 0); 264x512x256: "4325376 maxima exceed the table capacity
        4194304"; afterwards 2 200 791 056 device bytes held, as on a fresh context.
    density B, 64x64x128: n_maxima 65 536; neargrid + refine: [(458752, 0), (0, 0)] ('changed') and [(458752, 0), (458752, 0)]
        ('all'), 22 397 walkers per assignment and as many retraces per iteration through the exact slow path; ongrid + refine:
        [(458752, 233725), (455531, 0)] and [(458752, 233725), (458752, 0)], 44 688 / 44 794 slow-path retraces per call.
    The neargrid refusals above max_cap (assign_neargrid_tail) stay uncovered: how many of B's wandering trajectories the walkers
    hand to the slow path at 2^25 voxels is unmeasured, so B runs under neargrid only where that list holds the whole grid.
With `carry += total` taken out of k_rank_blocks (a scratch build; the sorted list zeroed first, since k_reset_first reads every slot
of it and the dropped carry leaves slots unwritten) both 264x512x256 cases fail on their maxima and both 256x512x256 cases pass.

The comparisons on the region tables that no mutation was run for, because the wrong form indexes out of bounds -- from the code:
    k_grow_finish, `l <= XB_BOXES_MAX` -> s_first[l - 1]: the LDS array has XB_BOXES_MAX ints, l - 1 <= 1023.  With `<` region 1024
        would reach neither branch, its first brick stay INT_MAX, k_note_regions skip it: n_maxima 1023 at 64x64x128 and 64x128x64.
    k_relabel_regions_brick, `b <= XB_BOXES_MAX ? s_rank[b - 1] : rank[box_max[b - 1]]`: s_rank is filled for i < min(regions, 1024),
        so b == 1024 reads a filled slot exactly when there are 1024 regions or more; both routes hold the same rank.
    k_seed_bricks, `k < XB_REGIONS_MAX` -> box_max[k], id k + 1: box_max is the 2^16 ints in front of box_first and the preset of
        box_first covers ids 1 .. 65 535; with `<=` id 65 536 would never be noted (FS_N_BOXES is capped) and its brick relabelled
        with INT_MAX: the map at 256x512x256 would differ."""
import time

import numpy as np
import pytest

import torch  # noqa: F401  (before the library: see conftest)
import capacity_common as cc
from pybader_amd import _lib

REGIONS_ON = _lib.XB_REGIONS_BOXES | _lib.XB_REGIONS_BRICKS   # the default of XB_OPT_REGIONS; 0: plain full trajectories

pytestmark = pytest.mark.gpu


def ids(shape):
    return 'x'.join(str(s) for s in shape)


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


_density_a = {}


def density_a(shape):
    """one density A at a time (277 MB at the largest shape)"""
    if shape not in _density_a:
        _density_a.clear()
        _density_a[shape] = cc.density_a(shape)
    return _density_a[shape]


def assign(ctx, method):
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign(method)
    return n, ctx.maxima(), ctx.download_labels(np.int32)


def check_a(ctx, shape, method, regions, what):
    """one assignment of density A (resident on ctx) against the closed form; with regions the brick labels' invariants"""
    bricks = cc.n_bricks(shape)
    ctx.set_option(_lib.XB_OPT_REGIONS, regions)
    n, mx, lab = assign(ctx, method)
    assert n == bricks, (what, n, bricks)
    assert_same(mx, cc.maxima_a(shape), what + ': maxima')
    assert_same(lab, cc.labels_a(shape), what + ': map')
    del lab
    if not regions:
        assert ctx.box_stats() == (0, 0), what
        return None
    n_regions = min(bricks, cc.XB_REGIONS_MAX)
    blab = ctx.brick_labels()
    stats = ctx.box_stats()
    print(f'{what}: n_maxima {n}, box_stats {stats}, bricks without a region {int((blab == 0).sum())}')
    assert blab.shape == tuple(s // 8 for s in shape)
    assert stats[0] == n_regions, (what, stats)
    # every seed brick beyond the table is walked; the others are certified, each for a region of its own
    assert int((blab == 0).sum()) == bricks - n_regions, what
    assert_same(np.sort(blab.reshape(-1))[bricks - n_regions:], np.arange(1, n_regions + 1), what + ': brick labels are a permutation of the region ids')
    assert stats[1] == 512 * n_regions, (what, stats)
    return blab


# ---- XB_BOXES_MAX and XB_SORT_MAX: small grids, both methods, with and without trapping regions --------------------------------

SMALL = [*cc.REGION_SHAPES.values(), cc.REGION_SHAPE_SMALL, *cc.SORT_SHAPES.values()]


@pytest.mark.parametrize('shape', SMALL, ids=ids)
def test_region_and_sort_boundaries(shape):
    """1008 / 1024 / 1056 regions (and 1024 on the small_grid form of the brick kernels), 2040 / 2048 / 2057 maxima"""
    dm, tg = cc.matrices(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.upload_density(density_a(shape))
    for method in ('neargrid', 'ongrid'):
        for regions in (REGIONS_ON, 0):
            check_a(ctx, shape, method, regions, f'{ids(shape)} {method} regions={regions}')
    print(f'{ids(shape)}: slow_path_stats {ctx.slow_path_stats()}')
    ctx.close()


@pytest.mark.parametrize('shape', list(cc.SORT_SHAPES.values()), ids=ids)
def test_assign_refine_at_the_sort_boundary(shape):
    """xb_assign_refine queues the first refinement iteration behind the assignment; above XB_SORT_MAX maxima the assignment does
    not end the way that iteration took for granted and it is redone.  Either way: what xb_assign + xb_refine return on a fresh
    context, and density A's map is the refinement's fixed point (tests/test_capacity_cpu.py: so says the oracle)."""
    dm, tg = cc.matrices(shape)
    res = []
    for fused in (True, False):
        ctx = _lib.Context(0)
        ctx.set_grid(shape, dm, tg)
        ctx.upload_density(density_a(shape))
        ctx.vacuum_assign(None, 1.0)
        if fused:
            n, log = ctx.assign_refine('neargrid', 'changed', 2)
        else:
            n = ctx.assign('neargrid')
            log = ctx.refine('changed', 2)
        res.append((n, log, ctx.maxima(), ctx.download_labels(np.int32), ctx.box_stats()))
        ctx.close()
    (n1, log1, mx1, lab1, st1), (n2, log2, mx2, lab2, st2) = res
    print(f'{ids(shape)}: assign_refine n {n1} log {log1} box_stats {st1}; assign + refine n {n2} log {log2} box_stats {st2}')
    assert n1 == n2 == cc.n_bricks(shape) and log1 == log2 and st1 == st2
    assert log1[0] == (cc.edges_a(shape), 0) and all(ch == 0 for _, ch in log1), log1
    for what, mx, lab in (('assign_refine', mx1, lab1), ('assign + refine', mx2, lab2)):
        assert_same(mx, cc.maxima_a(shape), f'{ids(shape)} {what}: maxima')
        assert_same(lab, cc.labels_a(shape), f'{ids(shape)} {what}: map')


# ---- XB_REGIONS_MAX and k_rank_blocks' carry: density A at 33 to 35 million voxels ----------------------------------------------

LARGE = [(cc.SEED_SHAPES[64512], 'neargrid'),    # 64 512 seeds: all fit; n_blocks = 1008
         (cc.SEED_SHAPES[65536], 'neargrid'),    # 65 536 seeds: one beyond the table; n_blocks = 1024, the round that fits exactly
         (cc.SEED_SHAPES[65536], 'ongrid'),      # ... through assign_ongrid_fused's own seeding
         (cc.CARRY_SHAPE, 'neargrid'),           # n_blocks = 1056: the carry; 2049 seeds beyond the table
         (cc.CARRY_SHAPE, 'ongrid')]


@pytest.mark.parametrize('shape,method', LARGE, ids=lambda p: ids(p) if isinstance(p, tuple) else p)
def test_seed_table_and_rank_carry(shape, method):
    t0 = time.time()
    dm, tg = cc.matrices(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.upload_density(density_a(shape))
    blab = check_a(ctx, shape, method, REGIONS_ON, f'{ids(shape)} {method}')
    bricks = cc.n_bricks(shape)
    if bricks == 64512:
        assert ctx.box_stats()[0] == 64512 and blab.min() == 1
    elif bricks == 65536:
        assert ctx.box_stats()[0] == 65535 and int((blab == 0).sum()) == 1 and ctx.n_maxima == 65536
    print(f'{ids(shape)} {method}: slow_path_stats {ctx.slow_path_stats()}, memory {ctx.memory_stats()[0] / 2**30:.2f} GiB, {time.time() - t0:.1f} s')
    ctx.close()


# ---- max_cap: density B, ongrid --------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def b_ongrid_at_capacity():
    t0 = time.time()
    rho = cc.density_b(cc.B_FITS_SHAPE)
    bmax, lab = cc.oracle_ongrid(rho, cc.B_FITS_SHAPE)
    print(f'oracle ongrid on density B at {ids(cc.B_FITS_SHAPE)}: {time.time() - t0:.1f} s')
    yield rho, bmax, lab
    _density_a.clear()      # (when the module is done: the cached large density goes with the oracle's arrays)


def test_maxima_table_full_then_exceeded_then_used_again(b_ongrid_at_capacity):
    """2^22 maxima fill the table exactly; 4 325 376 are refused with XB_E_LIMIT and the count in the message; the same context then
    assigns another density at that shape, by both methods, and holds what a fresh context holds after the same calls."""
    rho, bmax, want = b_ongrid_at_capacity
    shape = cc.B_FITS_SHAPE
    ctx = _lib.Context(0)
    ctx.set_grid(shape, *cc.matrices(shape))
    ctx.upload_density(rho)
    n, mx, lab = assign(ctx, 'ongrid')
    print(f'density B {ids(shape)} ongrid: n_maxima {n}, box_stats {ctx.box_stats()}, slow_path_stats {ctx.slow_path_stats()}')
    assert n == 4194304 == cc.MAX_CAP == bmax.shape[0]
    assert_same(mx, bmax, 'density B at the table capacity: maxima')
    assert_same(lab, want, 'density B at the table capacity: map')
    del lab, mx

    over = cc.B_OVER_SHAPE
    ctx.set_grid(over, *cc.matrices(over))
    ctx.upload_density(cc.density_b(over))
    ctx.vacuum_assign(None, 1.0)
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.assign('ongrid')
    print('refusal:', e.value)
    assert e.value.code == _lib.XB_E_LIMIT
    assert '4325376' in str(e.value) and 'maxima exceed the table capacity' in str(e.value)

    def both_methods(c):
        c.upload_density(density_a(over))
        for method in ('ongrid', 'neargrid'):
            check_a(c, over, method, REGIONS_ON, f'{ids(over)} {method} after the refusal' if c is ctx else f'{ids(over)} {method} fresh')
        return c.memory_stats()[0]
    held = both_methods(ctx)
    ctx.close()
    fresh = _lib.Context(0)
    fresh.set_grid(over, *cc.matrices(over))
    held_fresh = both_methods(fresh)
    fresh.close()
    print(f'device bytes held: {held} after the refusal, {held_fresh} on a fresh context')
    assert held == held_fresh


# ---- density B under neargrid, where the slow path's list holds the whole grid ----------------------------------------------

@pytest.fixture(scope='module')
def b_small():
    t0 = time.time()
    shape = cc.B_NEARGRID_SHAPE
    rho = cc.density_b(shape)
    out = {'rho': rho, 'ongrid': cc.oracle_ongrid(rho, shape), 'neargrid': cc.oracle_neargrid(rho, shape)}
    for method in ('ongrid', 'neargrid'):
        for mode in ('changed', 'all'):
            out[method, mode] = cc.oracle_refine(rho, out[method][1], shape, (mode, 2))
    print(f'oracle maps and refinements of density B at {ids(shape)}: {time.time() - t0:.1f} s')
    return out


@pytest.mark.parametrize('method', ['neargrid', 'ongrid'])
def test_density_b_assign_and_refine(b_small, method):
    """N / 8 maxima, 7 / 8 of the voxels edge voxels: the assignment against the oracle, then the refinement in both modes, maps and
    logs.  The own-trajectory map is the refinement's fixed point; the ongrid map is not (233 725 voxels move in the first
    iteration, none in the second)."""
    shape = cc.B_NEARGRID_SHAPE
    bmax, want = b_small[method]
    ctx = _lib.Context(0)
    ctx.set_grid(shape, *cc.matrices(shape))
    ctx.upload_density(b_small['rho'])
    for mode in ('changed', 'all'):
        n, mx, lab = assign(ctx, method)
        assert n == cc.n_voxels(shape) // 8 == bmax.shape[0]
        assert_same(mx, bmax, f'density B {method}: maxima')
        assert_same(lab, want, f'density B {method}: map')
        log = ctx.refine(mode, 2)
        want_map, want_log = b_small[method, mode]
        print(f'density B {ids(shape)} {method} + refine({mode}, 2): n_maxima {n}, log {log}, box_stats {ctx.box_stats()}, slow_path_stats {ctx.slow_path_stats()}')
        assert log == want_log, (log, want_log)
        assert_same(ctx.download_labels(np.int32), want_map, f'density B {method} + refine({mode}, 2): map')
        if method == 'ongrid':
            assert log[0][1] == 233725 and log[1][1] == 0
        else:
            assert all(ch == 0 for _, ch in log)
    ctx.close()

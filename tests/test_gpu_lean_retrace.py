"""GPU tests (-m gpu) of the lean retrace of one GPU (k_refine_trace_lean, round 10) against the generic retrace kernel it stands
in for (k_refine_trace, XB_CHECK_GENERIC_RETRACE) and against the CPU oracle.

Every case runs the same calls twice on one context -- the default form, then with XB_CHECK_GENERIC_RETRACE set -- and compares
both, bit for bit, with each other and with the oracle: the maxima, the label map, the flags (`known`) after the refinement, the
refinement log, slow_path_stats(), deferred_stats() and -- call by call, as sorted sets -- the voxels the retraces put on their
overflow lists (retrace_overflow(), kept under DEBUG_KEEP_RETRACE_OVERFLOW).  retrace_stats() says which kernel the first
retraces of the edge lists were launched as: every case asserts that the default form took the lean kernel where its case holds
and nowhere else, and that the second form never took it.

The lean kernel's case needs the region labels of a neargrid assignment, which only grids of at least 16 voxels per axis get: on
16 x 8 x 80 and 8 x 16 x 24 (an axis one brick wide) both forms run the generic kernel, and the test asserts exactly that."""
import numpy as np
import pytest

import rough_common
from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform

pytestmark = pytest.mark.gpu

REFINES = (('changed', 2), ('all', -1))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    c.set_option(_lib.XB_OPT_DEBUG, _lib.DEBUG_KEEP_RETRACE_OVERFLOW)
    yield c
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    c.set_option(_lib.XB_OPT_DEBUG, 0)
    c.close()


def seeded_case(seed, shape):
    """tests/test_gpu_neighbour_bits.py's seeded_case: a seeded multi-atom density on a seeded skewed lattice"""
    rng = np.random.default_rng(seed)
    lat = synth.CUBIC6 * (0.8 + 0.4 * rng.random()) + 0.8 * (rng.random((3, 3)) - 0.5)
    na = int(rng.integers(2, 5))
    atoms = np.concatenate([rng.random((na, 3)), 0.5 + 0.3 * rng.random((na, 1)), 1 + 7 * rng.random((na, 1))], axis=1)
    rho = synth.synth_density(shape, lat, atoms)
    vl = np.divide(lat, shape)
    return rho, distance_matrix(vl), gradient_transform(vl)


def oracle_refine(rho, start, dm, tg, mode):
    import oracle
    v = start.copy()
    log = []
    oracle.refine('neargrid', mode, rho, v, dm, tg, 1, log=log)
    return v, [tuple(x) for x in log]


_oracle = {}


def oracle_case(key, rho, dm, tg):
    """the oracle's side of a case without vacuum, computed once: the assignment (labels + maxima) and its refinements"""
    if key not in _oracle:
        vol0 = np.zeros(rho.shape, np.int32)
        want, maxima = rough_common.rank_labels(rough_common.own_map(rho, vol0, dm, tg, main_ties=True))
        _oracle[key] = {'assign': want, 'maxima': maxima,
                        'refined': {mode: oracle_refine(rho, want.astype(np.int32), dm, tg, mode) for mode in REFINES}}
    return _oracle[key]


def counters(c):
    return c.slow_path_stats() + (c.deferred_stats(),) + c.retrace_stats()


def overflow_set(c):
    """the voxels the retraces since the last call put on their overflow lists, sorted (the order of a list is the atomics')"""
    return np.sort(c.retrace_overflow())


def both_forms(ctx, run, lean):
    """run(ctx) under the default form and under XB_CHECK_GENERIC_RETRACE; the two outcomes are equal item by item, and so is
    what each added to slow_path_stats() and deferred_stats().  lean: the default form must have launched the lean kernel
    (True: at least once; 'only': and the generic one never) or must not have (False); the second form never does.  Returns the
    default form's items, then what it added to (assign slow path, refine slow path, deferred, lean launches, generic launches)."""
    out, launches = [], []
    for bits in (0, _lib.CROSS_CHECK_GENERIC_RETRACE):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
        ctx.retrace_overflow()
        before = counters(ctx)
        res = run(ctx)
        d = tuple(int(x) - int(y) for x, y in zip(counters(ctx), before))
        out.append(res + [d[:3]])
        launches.append(d[3:])
    ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    print('first retraces launched (lean, generic): default form', launches[0], 'under XB_CHECK_GENERIC_RETRACE', launches[1])
    assert sum(launches[0]) == sum(launches[1]) > 0 and launches[1][0] == 0, launches
    assert (launches[0][0] > 0) == bool(lean), launches
    assert lean != 'only' or launches[0][1] == 0, launches
    a, b = out
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k
    return a


def load(ctx, rho, dm, tg):
    ctx.set_grid(rho.shape, dm, tg)
    ctx.upload_density(rho)
    ctx.vacuum_assign(None, 1.0)


def assign_refine_all(ctx, rho, dm, tg):
    """[n, maxima, labels] of an assignment, then per mode of REFINES [log, labels, known] of a fresh assignment refined, then
    [n, log, labels] of the two in one call (the fused step of the benchmark); after each refinement the sorted overflow set"""
    res = []
    for mode in REFINES:
        load(ctx, rho, dm, tg)
        n = ctx.assign('neargrid')
        if not res:
            res += [n, np.ravel_multi_index(tuple(ctx.maxima().T), rho.shape), ctx.download_labels(np.int64)]
        res += [ctx.refine(*mode), ctx.download_labels(np.int64), ctx.download_known(), overflow_set(ctx)]
    load(ctx, rho, dm, tg)
    n, log = ctx.assign_refine('neargrid', *REFINES[0])
    res += [n, log, ctx.download_labels(np.int64), overflow_set(ctx)]
    return res


def check_assign_refine(got, o):
    assert got[0] == o['maxima'].shape[0] and np.array_equal(got[1], o['maxima'])
    assert np.array_equal(got[2], o['assign'])
    for k, mode in enumerate(REFINES):
        v, log = o['refined'][mode]
        assert got[3 + 4 * k] == log, mode
        assert np.array_equal(got[4 + 4 * k], v), mode
    base = 3 + 4 * len(REFINES)
    v, log = o['refined'][REFINES[0]]
    assert got[base] == got[0] and got[base + 1] == log and np.array_equal(got[base + 2], v)


# Seeds chosen ON THE CPU (the oracle alone): the first seed of seeded_case, counted from 1, whose first ('changed', 2) iteration
# relabels voxels -- so the second iteration, the edge_check and the host-driven retrace launch, has work.  16 x 16 x 80 is the
# smallest grid that takes the bit sweep, and two bricks wide in x and y: the low and the high neighbour of a brick are ONE brick.
# 16 x 8 x 80 and 8 x 16 x 24 have an axis one brick wide, below the 16 voxels per axis from which an assignment leaves region
# labels: the lean kernel's case does not hold, both forms must run the generic kernel (last entry: is the lean kernel taken).
SEEDED = {'16x8x80': (167, (16, 8, 80), False), '16x16x80': (154, (16, 16, 80), 'only'), '8x16x24': (687, (8, 16, 24), False)}


@pytest.mark.parametrize('name', list(SEEDED))
def test_seeded_small_grids_both_forms_equal_the_oracle(ctx, name):
    """1. the smallest whole-brick grids: the smallest grid of the bit sweep, on which both launch sites take the lean kernel, and
    two grids with an axis one brick wide, on which it must not be chosen."""
    seed, shape, lean = SEEDED[name]
    rho, dm, tg = seeded_case(seed, shape)
    o = oracle_case(name, rho, dm, tg)
    log = o['refined'][REFINES[0]][1]
    print(name, 'oracle log', log)
    assert log[0][1] > 0 and len(log) == 2, 'the seed is chosen so that the first iteration changes labels and a second runs'
    got = both_forms(ctx, lambda c: assign_refine_all(c, rho, dm, tg), lean)
    print(name, 'slow path / deferred', got[-1])
    check_assign_refine(got, o)


def test_triclinic_32_both_forms_equal_the_oracle(ctx):
    """2. a triclinic 32^3 cell: the full T_grad product."""
    shape = (32, 32, 32)
    rho = synth.synth_density(shape, synth.TRICLINIC)
    vl = np.divide(synth.TRICLINIC, shape)
    dm, tg = distance_matrix(vl), gradient_transform(vl)
    o = oracle_case('tric32', rho, dm, tg)
    got = both_forms(ctx, lambda c: assign_refine_all(c, rho, dm, tg), 'only')
    print('tric32 oracle log', o['refined'][REFINES[0]][1], 'slow path / deferred', got[-1])
    check_assign_refine(got, o)


def test_plateaus_both_forms_equal_the_oracle(ctx):
    """3. a quantised density (32 x 24 x 24): plateaus, so records with the stay code, ongrid moves and retraces that end on a
    maximum; the refinement rebuilds the table under its own tie rule -- of whole bricks on the whole grid, so pass B writes the
    neighbour bits again and the labels are still the assignment's: the lean kernel is taken at every launch."""
    g, rho = rough_common.load_rough('r32_quant8')
    assert rho.shape == (32, 24, 24) and rough_common.vac_tol(g) is None
    o = oracle_case('r32_quant8', rho, g['dist_mat'], g['T_grad'])
    got = both_forms(ctx, lambda c: assign_refine_all(c, rho, g['dist_mat'], g['T_grad']), 'only')
    print('r32_quant8 oracle log', o['refined'][REFINES[0]][1], 'slow path / deferred', got[-1])
    check_assign_refine(got, o)


def test_rough_density_retraces_reach_the_overflow_list(ctx):
    """4. a noisy density (40^3): retraces dip below a density passed more than two steps ago, the two-voxel window cannot decide
    and they go to the overflow list -- the same voxels under either form (the sorted lists of every call are compared), with the
    same labels in the end.  The lean kernel is taken at every launch."""
    g, rho = rough_common.load_rough('r40_noise04')
    assert rough_common.vac_tol(g) is None
    o = oracle_case('r40_noise04', rho, g['dist_mat'], g['T_grad'])
    got = both_forms(ctx, lambda c: assign_refine_all(c, rho, g['dist_mat'], g['T_grad']), 'only')
    print('r40_noise04 oracle log', o['refined'][REFINES[0]][1], 'slow path / deferred', got[-1])
    assert got[-1][1] > 0, 'no retrace reached the overflow list'
    check_assign_refine(got, o)


@pytest.mark.parametrize('guard', ['upload_labels', 'ongrid_assign', 'cut_bricks'])
def test_lean_retrace_is_not_taken_where_its_case_does_not_hold(ctx, guard):
    """5. labels from outside, an ongrid assignment's labels, a grid that cuts its last bricks (20 x 16 x 80): the refinement equals
    the oracle's under both forms -- the lean kernel's preconditions (the last neargrid assignment's labels, whole bricks with
    valid neighbour bits) do not hold and it must not run."""
    import oracle
    shape = (20, 16, 80) if guard == 'cut_bricks' else (16, 16, 80)
    rho, dm, tg = seeded_case(SEEDED['16x16x80'][0], shape)
    o = oracle_case(guard + '%dx%dx%d' % shape, rho, dm, tg)
    vol0 = np.zeros(shape, np.int32)
    if guard == 'cut_bricks':
        start = o['assign'].astype(np.int32)
        want = o['refined']
    else:
        _, omain = oracle.bader_calc('ongrid', rho, vol0, dm, tg, 1)
        start = omain.astype(np.int32)
        assert not np.array_equal(start, o['assign']), 'a different map'
        want = {mode: oracle_refine(rho, start, dm, tg, mode) for mode in REFINES}

    def run(c):
        res = []
        for mode in REFINES:
            load(c, rho, dm, tg)
            c.assign('neargrid')
            if guard == 'upload_labels':
                c.upload_labels(start)
            elif guard == 'ongrid_assign':
                c.upload_labels(vol0)
                c.assign('ongrid')
            res += [c.refine(*mode), c.download_labels(np.int32), c.download_known(), overflow_set(c)]
        return res
    got = both_forms(ctx, run, False)
    for k, mode in enumerate(REFINES):
        v, log = want[mode]
        assert got[4 * k] == log and np.array_equal(got[4 * k + 1], v), mode

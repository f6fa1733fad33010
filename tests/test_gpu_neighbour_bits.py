"""GPU tests (-m gpu) of the neighbour bits pass B writes into every record (key bits 11-17: which neighbour bricks hold no
records) and of the lean walker / lean retrace that read them instead of a brick label / brick byte per step.

Every case runs the same calls twice -- the default form, then with XB_CHECK_BRICK_LOOKUP set (the per-step lookups) -- and
compares both, bit for bit (labels, maxima, refinement logs), with each other and with the CPU oracle: the own-trajectory map
ranked by first voxel for an assignment, oracle.refine for a refinement."""
import numpy as np
import pytest

import rough_common
from conftest import case_density, load_golden
from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform

pytestmark = pytest.mark.gpu

REFINES = (('changed', 2), ('all', -1))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    c.close()


def seeded_case(seed, shape):
    """a seeded multi-atom density on a seeded skewed lattice (the style of test_gpu_parity.random_case, fewer and wider atoms:
    small grids still grow trapping regions)"""
    rng = np.random.default_rng(seed)
    lat = synth.CUBIC6 * (0.8 + 0.4 * rng.random()) + 0.8 * (rng.random((3, 3)) - 0.5)
    na = int(rng.integers(2, 5))
    atoms = np.concatenate([rng.random((na, 3)), 0.5 + 0.3 * rng.random((na, 1)), 1 + 7 * rng.random((na, 1))], axis=1)
    rho = synth.synth_density(shape, lat, atoms)
    vl = np.divide(lat, shape)
    return rho, distance_matrix(vl), gradient_transform(vl)


def golden_case(name):
    g = load_golden(name)
    t = float(g['vacuum_tol'])
    return case_density(g), g['dist_mat'], g['T_grad'], None if np.isnan(t) else t


_oracle = {}


def oracle_case(key, rho, dm, tg, tol):
    """the oracle's side of a case, computed once: vacuum map, assignment (labels + maxima), the refinements of that assignment,
    the sequential main map and the ongrid map"""
    if key in _oracle:
        return _oracle[key]
    import oracle
    vol0 = np.zeros(rho.shape, np.int32)
    vol0, _, _ = oracle.vacuum_assign(rho, vol0, float('nan') if tol is None else tol, rho, 1.0)
    want, maxima = rough_common.rank_labels(rough_common.own_map(rho, vol0, dm, tg, main_ties=True))
    o = {'vol0': vol0, 'assign': want, 'maxima': maxima}
    o['refined'] = {mode: oracle_refine(rho, want.astype(np.int32), dm, tg, mode) for mode in REFINES}
    _oracle[key] = o
    return o


def oracle_refine(rho, start, dm, tg, mode):
    import oracle
    v = start.copy()
    log = []
    oracle.refine('neargrid', mode, rho, v, dm, tg, 1, log=log)
    return v, [tuple(x) for x in log]


def both_forms(ctx, run):
    """run(ctx) under the default form and under XB_CHECK_BRICK_LOOKUP; the two outcomes are equal item by item"""
    out = []
    for bits in (0, _lib.CROSS_CHECK_BRICK_LOOKUP):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
        out.append(run(ctx))
    ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    a, b = out
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    return a


def load(ctx, rho, dm, tg, tol):
    ctx.set_grid(rho.shape, dm, tg)
    ctx.upload_density(rho)
    ctx.vacuum_assign(tol, 1.0)


def assign_refine_all(ctx, rho, dm, tg, tol):
    """[n, maxima, labels] of an assignment, then per mode of REFINES [log, labels] of a fresh assignment refined"""
    res = []
    for mode in REFINES:
        load(ctx, rho, dm, tg, tol)
        n = ctx.assign('neargrid')
        if not res:
            res += [n, np.ravel_multi_index(tuple(ctx.maxima().T), rho.shape), ctx.download_labels(np.int64)]
        res += [ctx.refine(*mode), ctx.download_labels(np.int64)]
    return res


def check_assign_refine(got, o):
    assert got[0] == o['maxima'].shape[0] and np.array_equal(got[1], o['maxima'])
    assert np.array_equal(got[2], o['assign'])
    for k, mode in enumerate(REFINES):
        v, log = o['refined'][mode]
        assert got[3 + 2 * k] == log, mode
        assert np.array_equal(got[4 + 2 * k], v), mode


# Seeds chosen ON THE GPU (region growth has no CPU restatement): for each shape with an axis of 32 voxels or more the seed of
# seeded_case, of 1..8, that leaves the most voxels in trapping regions while others are walked, 0 < box_stats()[1] < N (2048
# of 12288 and 2560 of 30720 voxels) -- so walkers do arrive in a trapping region.  16^3 (two bricks per axis: the low and the
# high neighbour of a brick are one brick) is too small for a region and runs for the wrap alone.
SEEDED = {'16x16x16': (1, (16, 16, 16)), '24x16x32': (6, (24, 16, 32)), '16x24x80': (7, (16, 24, 80))}
GOLDENS = ['c64_cubic', 'c40x48x56_tric']   # (a triclinic and a cubic lattice: both Grid forms of pass B)


@pytest.mark.parametrize('name', list(SEEDED) + GOLDENS)
def test_assign_and_refine_both_forms_equal_the_oracle(ctx, name):
    """1. assign, then refine ('changed', 2) and ('all', -1): two bricks per axis, the small_grid form, the non-small form, and
    the goldens' lattices."""
    if name in SEEDED:
        seed, shape = SEEDED[name]
        rho, dm, tg = seeded_case(seed, shape)
        tol = None
    else:
        rho, dm, tg, tol = golden_case(name)
    o = oracle_case(name, rho, dm, tg, tol)
    stats = []

    def run(c):
        res = assign_refine_all(c, rho, dm, tg, tol)
        stats.append(c.box_stats()[1])
        return res
    check_assign_refine(both_forms(ctx, run), o)
    print(name, 'voxels in trapping regions', stats, 'of', rho.size)
    if max(rho.shape) >= 32:
        assert all(0 < s < rho.size for s in stats), stats


@pytest.mark.parametrize('name', ['24x16x32', '16x24x80'])
def test_refine_from_sequential_and_ongrid_maps(ctx, name):
    """2. refinement from the oracle's sequential main map (upload_labels: the flag-mode table of the mixed bricks, no
    regions_ok, deferred retraces) and from an ongrid assignment of the library's own (the band-brick table)."""
    import oracle
    seed, shape = SEEDED[name]
    rho, dm, tg = seeded_case(seed, shape)
    vol0 = np.zeros(shape, np.int32)
    _, main = oracle.bader_calc('neargrid', rho, vol0, dm, tg, 1)
    omax, omain = oracle.bader_calc('ongrid', rho, vol0, dm, tg, 1)
    want = {(tag, mode): oracle_refine(rho, start, dm, tg, mode) for tag, start in (('main', main), ('ongrid', omain)) for mode in REFINES}

    def run(c):
        res = []
        for mode in REFINES:
            load(c, rho, dm, tg, None)
            c.upload_labels(main)
            res += [c.refine(*mode), c.download_labels(main.dtype)]
        for mode in REFINES:
            load(c, rho, dm, tg, None)
            c.assign('ongrid')
            res += [c.maxima(), c.download_labels(omain.dtype), c.refine(*mode), c.download_labels(omain.dtype)]
        return res
    got = both_forms(ctx, run)
    for k, mode in enumerate(REFINES):
        v, log = want[('main', mode)]
        assert got[2 * k] == log and np.array_equal(got[2 * k + 1], v), ('main', mode)
        v, log = want[('ongrid', mode)]
        base = 2 * len(REFINES) + 4 * k
        assert np.array_equal(got[base], omax) and np.array_equal(got[base + 1], omain)
        assert got[base + 2] == log and np.array_equal(got[base + 3], v), ('ongrid', mode)


def test_quantised_density_rebuilds_the_bits_under_the_other_tie_rule(ctx):
    """3. axis ties (32 x 24 x 24, quantised): the assignment's table obeys methods.py:324, the refinement rebuilds the same
    bricks under refinement.py:111 -- pass B in flag mode rewrites the bits."""
    g, rho = rough_common.load_rough('r32_quant8')
    assert rho.shape == (32, 24, 24)
    tol = rough_common.vac_tol(g)
    o = oracle_case('r32_quant8', rho, g['dist_mat'], g['T_grad'], tol)
    check_assign_refine(both_forms(ctx, lambda c: assign_refine_all(c, rho, g['dist_mat'], g['T_grad'], tol)), o)


def vacuum_brick_case():
    """32^3, two narrow atoms in one corner region and a tolerance above the background: whole 8^3 bricks lie below it"""
    shape = (32, 32, 32)
    atoms = np.array([[0.25, 0.25, 0.25, 0.35, 6.0], [0.45, 0.3, 0.35, 0.3, 4.0]])
    rho = synth.synth_density(shape, synth.TRICLINIC, atoms)
    vl = np.divide(synth.TRICLINIC, shape)
    return rho, distance_matrix(vl), gradient_transform(vl), 2.0 * synth.BACKGROUND


@pytest.mark.parametrize('name', ['c48_cubic_vac', 'vacuum_bricks_32'])
def test_vacuum_bricks_both_forms_equal_the_oracle(ctx, name):
    """4. XB_NOREC neighbours: bricks below the vacuum tolerance hold no records and are no region; a walker that steps into one
    goes to the exact slow kernel in both forms."""
    rho, dm, tg, tol = golden_case(name) if name == 'c48_cubic_vac' else vacuum_brick_case()
    o = oracle_case(name, rho, dm, tg, tol)
    if name == 'vacuum_bricks_32':
        vac = (o['vol0'] == -1).reshape(4, 8, 4, 8, 4, 8).all(axis=(1, 3, 5))
        assert 0 < vac.sum() < vac.size, 'the case is built to have whole vacuum bricks next to others'
    check_assign_refine(both_forms(ctx, lambda c: assign_refine_all(c, rho, dm, tg, tol)), o)


@pytest.mark.parametrize('guard', ['upload_labels', 'ongrid_assign', 'drop_table'])
def test_stale_bits_are_never_trusted(ctx, guard):
    """5. whatever replaces the labels or drops the table after a neargrid assignment, the refinement that follows equals the
    oracle's: the bits of the assignment's table are not used for a table that no longer matches them."""
    import oracle
    seed, shape = SEEDED['16x24x80']
    rho, dm, tg = seeded_case(seed, shape)
    o = oracle_case('16x24x80', rho, dm, tg, None)
    vol0 = np.zeros(shape, np.int32)
    _, omain = oracle.bader_calc('ongrid', rho, vol0, dm, tg, 1)
    start = o['assign'].astype(np.int32) if guard == 'drop_table' else omain.astype(np.int32)
    assert guard == 'drop_table' or not np.array_equal(start, o['assign']), 'a different map'
    want = {mode: oracle_refine(rho, start, dm, tg, mode) for mode in REFINES}

    def run(c):
        res = []
        for mode in REFINES:
            load(c, rho, dm, tg, None)
            c.assign('neargrid')
            if guard == 'upload_labels':
                c.upload_labels(start)
            elif guard == 'ongrid_assign':
                c.upload_labels(vol0)
                c.assign('ongrid')
            else:
                c.set_option(_lib.XB_OPT_DROP_TABLE, 1)
            res += [c.refine(*mode), c.download_labels(np.int32)]
        return res
    got = both_forms(ctx, run)
    for k, mode in enumerate(REFINES):
        v, log = want[mode]
        assert got[2 * k] == log and np.array_equal(got[2 * k + 1], v), mode

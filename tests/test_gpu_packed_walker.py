"""GPU tests (-m gpu) of the lean walker on a packed position (k_trace.h, ng_walk_packed; bader_kernels.h, pw_*): the group
trace's walker wherever the records carry valid neighbour bits.

Every case runs the same calls in three forms -- the packed walker (cross-check 0), the lean walker with the brick-label lookup
(XB_CHECK_BRICK_LOOKUP) and the generic walker (XB_CHECK_GENERIC_WALKER) -- asserts with trace_stats() which walker ran, and
compares labels, maxima, slow_path_stats(), box_stats() and the log and labels of refine('changed', 2), bit for bit, with each
other and with the CPU oracle (the own-trajectory map ranked by first voxel, oracle.refine).

The packed position has no range limit: a walker that leaves its 512-voxel window takes a new one (pw_rebase).  The case
'16x16x640' makes walkers do that, with and without a periodic face in between; its slow-path counts equal the other forms' like
everyone else's.  The packing itself is checked at compile time (bader_kernels.h, pw_check)."""
import numpy as np
import pytest

import rough_common
from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform

pytestmark = pytest.mark.gpu

MODE = ('changed', 2)
FORMS = {'packed': 0, 'lookup': _lib.CROSS_CHECK_BRICK_LOOKUP, 'generic': _lib.XB_CHECK_GENERIC_WALKER}
RAN = {'packed': 0, 'lookup': 1, 'generic': 2}   # the slot of trace_stats() that counts the form's launches


def seeded_case(seed, shape):
    """a seeded multi-atom density on a seeded skewed lattice (as tests/test_gpu_neighbour_bits.py builds them)"""
    rng = np.random.default_rng(seed)
    lat = synth.CUBIC6 * (0.8 + 0.4 * rng.random()) + 0.8 * (rng.random((3, 3)) - 0.5)
    na = int(rng.integers(2, 5))
    atoms = np.concatenate([rng.random((na, 3)), 0.5 + 0.3 * rng.random((na, 1)), 1 + 7 * rng.random((na, 1))], axis=1)
    rho = synth.synth_density(shape, lat, atoms)
    vl = np.divide(lat, shape)
    return rho, distance_matrix(vl), gradient_transform(vl), None


def faces_case(lattice):
    """32^3, an atom on the cell's corner and one on the middle of each face pair: basins straddle all six periodic faces, and
    walkers cross each face in both directions"""
    shape = (32, 32, 32)
    atoms = np.array([[0.0, 0.0, 0.0, 0.6, 6.0], [0.0, 0.5, 0.5, 0.55, 5.0], [0.5, 0.0, 0.5, 0.5, 4.0], [0.5, 0.5, 0.0, 0.6, 7.0]])
    rho = synth.synth_density(shape, lattice, atoms)
    vl = np.divide(lattice, shape)
    return rho, distance_matrix(vl), gradient_transform(vl), None


def long_walk_case():
    """16 x 16 x 640: the density rises along z from its minimum at z = 30 to its crest at z = 630 and falls from there through
    the periodic face back to z = 30; a modulation across y puts two ridges (y = 0 and y = 8) and the surfaces between them
    (y = 4, y = 12) inside every brick, so no brick is certified.  Walkers from z = 31 travel 600 voxels up, through more than
    one 512-voxel window; walkers from z < 30 travel down through the face at z = 0 into the window at the grid's other end.
    (tests/elongated_common.py builds it for any long axis and length; tests/test_elongated_cpu.py pins this one to the values
    stated here, and tests/test_gpu_elongated.py runs the other axes and the lengths around a window.)"""
    import elongated_common
    return elongated_common.long_walk(2, 640) + (None,)


def quant_case():
    g, rho = rough_common.load_rough('r32_quant8')
    return rho, g['dist_mat'], g['T_grad'], rough_common.vac_tol(g)


# Seeds of seeded_case chosen ON THE GPU (the growth of trapping regions has no CPU restatement, so the test asserts it there):
# per shape the first seed with 0 < box_stats()[1] < N -- walkers exist, regions exist, and walkers arrive in them (512 of 4096,
# 4096 of 20480 and 2048 of 15360 voxels in regions; 16^3 rarely grows a region: seed 80 is the first of 1..3000 that does).
# With two bricks on an axis the low and the high neighbour are the same brick, and every move off a brick wraps.
CASES = {
    '16x16x16': lambda: seeded_case(SEEDS['16x16x16'], (16, 16, 16)),
    '16x16x80': lambda: seeded_case(SEEDS['16x16x80'], (16, 16, 80)),
    '24x16x40': lambda: seeded_case(SEEDS['24x16x40'], (24, 16, 40)),
    'faces_cubic': lambda: faces_case(synth.CUBIC6),
    'faces_triclinic': lambda: faces_case(synth.TRICLINIC),
    'quant8': quant_case,
    '16x16x640': long_walk_case,
}
SEEDS = {'16x16x16': 80, '16x16x80': 6, '24x16x40': 6}
SMALL = ('16x16x16', '16x16x80', '24x16x40')

_cases, _oracle = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def oracle_case(name):
    """the oracle's side of a case, computed once and never written to: vacuum map, assignment (labels + maxima) and its
    refinement"""
    if name in _oracle:
        return _oracle[name]
    import oracle
    rho, dm, tg, tol = case(name)
    vol0 = np.zeros(rho.shape, np.int32)
    vol0, _, _ = oracle.vacuum_assign(rho, vol0, float('nan') if tol is None else tol, rho, 1.0)
    want, maxima = rough_common.rank_labels(rough_common.own_map(rho, vol0, dm, tg, main_ties=True))
    v = want.astype(np.int32).copy()
    log = []
    oracle.refine('neargrid', MODE, rho, v, dm, tg, 1, log=log)
    for a in (want, maxima, v):
        a.setflags(write=False)
    _oracle[name] = {'assign': want, 'maxima': maxima, 'refined': v, 'log': [tuple(x) for x in log]}
    return _oracle[name]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    c.close()


def run_form(c, name, form):
    """assign + refine under one form on context c: (n, maxima, labels, slow-path walkers of the assignment, box_stats, refine
    log, refined labels, slow-path walkers of the refinement); asserts that the form's walker, and no other, traced"""
    rho, dm, tg, tol = case(name)
    c.set_option(_lib.XB_OPT_CROSS_CHECK, FORMS[form])
    c.set_grid(rho.shape, dm, tg)
    c.upload_density(rho)
    c.vacuum_assign(tol, 1.0)
    t0, s0 = c.trace_stats(), c.slow_path_stats()
    n = c.assign('neargrid')
    t1, s1 = c.trace_stats(), c.slow_path_stats()
    ran = [b - a for a, b in zip(t0, t1)]
    assert ran[RAN[form]] >= 1 and sum(ran) == ran[RAN[form]], (form, ran)
    res = [n, np.ravel_multi_index(tuple(c.maxima().T), rho.shape), c.download_labels(np.int64), s1[0] - s0[0], c.box_stats()]
    log = c.refine(*MODE)
    s2 = c.slow_path_stats()
    res += [log, c.download_labels(np.int64), s2[1] - s1[1]]
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    return res


def same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k


def check_oracle(got, o):
    assert got[0] == o['maxima'].shape[0] and np.array_equal(got[1], o['maxima'])
    assert np.array_equal(got[2], o['assign'])
    assert got[5] == o['log']
    assert np.array_equal(got[6], o['refined'])


@pytest.mark.parametrize('name', list(CASES))
def test_three_walkers_equal_each_other_and_the_oracle(ctx, name):
    """1. - 4.: the smallest grids that reach the kernel, the six faces on a cubic and a triclinic cell, the quantised density
    whose refinement rebuilds the table under its other tie rule (a second assignment after it must still be right), and the
    long walk through several windows.  Slow-path counts are EQUAL over the forms: the packed walker hands over nothing the
    lookup form decides."""
    o = oracle_case(name)
    rho = case(name)[0]
    if name == '16x16x640':
        assert o['maxima'].shape[0] == 2, 'two ridges, one maximum each'
        z = np.unravel_index(o['maxima'], rho.shape)[2]
        assert np.all(z == 630)
    got = {form: run_form(ctx, name, form) for form in FORMS}
    print(name, 'basins', got['packed'][0], 'slow-path walkers (assign, refine)', got['packed'][3], got['packed'][7], 'box_stats', got['packed'][4])
    same(got['packed'], got['lookup'])
    same(got['packed'], got['generic'])
    check_oracle(got['packed'], o)
    if name in SMALL:
        assert 0 < got['packed'][4][1] < rho.size, got['packed'][4]
    if name == '16x16x640':
        assert got['packed'][4][1] == 0, 'no brick is certified: every voxel is walked, from z = 31 over 600 voxels'
    if name == 'quant8':   # the refinement left the table under refinement.py:111; the next assignment rebuilds it
        again = run_form(ctx, name, 'packed')
        same(again, got['packed'])


@pytest.mark.parametrize('order', [('packed', 'lookup', 'generic'), ('generic', 'lookup', 'packed')])
def test_history_of_forms_on_one_context_does_not_matter(order):
    """5. the three forms one after another on ONE context, each with its refinement, on alternating cases: every result equals
    that of a fresh context."""
    names = ('24x16x40', 'faces_triclinic', '16x16x80')
    fresh = {}
    for form, name in zip(order, names):
        c = _lib.Context(0)
        try:
            fresh[form] = run_form(c, name, form)
        finally:
            c.close()
    c = _lib.Context(0)
    try:
        for form, name in zip(order, names):
            same(run_form(c, name, form), fresh[form])
        for form, name in zip(reversed(order), reversed(names)):
            same(run_form(c, name, form), fresh[form])
    finally:
        c.close()
    for form, name in zip(order, names):
        check_oracle(fresh[form], oracle_case(name))

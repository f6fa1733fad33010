"""Tests of the edge sweep by row bit masks (k_edge_sweep_bits: flags, dilation and edge list of the listed tiles in one
kernel) against the per-voxel sweep (k_edge_flag_listed + k_edge_dilate_tiles, CROSS_CHECK_VOXEL_SWEEP) and the CPU oracle.

The shapes are the smallest the bit form runs at (whole 4 x 8 x 64 tiles, nz >= 80): 16 x 16 x 128 (two z-tiles: both z-halos
of a tile lie in the one other tile through the wrap; four x-tiles: the two-voxel x-halo wraps; two y-tiles), 16 x 24 x 128
(three y-tiles) and 20 x 16 x 192 (nx a multiple of 4 but not of 8: the grid cuts bricks in x; three z-tiles).  Every GPU case
runs under both forms and proves through sweep_stats() which one ran.  The last test (no GPU) restates the 17-mask formula in
numpy against the brute-force 27-box test."""
import numpy as np
import pytest

import rough_common
from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform

SHAPES = {'16x16x128': (16, 16, 128), '16x24x128': (16, 24, 128), '20x16x192': (20, 16, 192)}
REFINES = (('changed', 2), ('all', -1))
TILE = (4, 8, 64)   # the tile the single-voxel and maximum cases are placed round: origin of the second tile per axis


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    c.close()


def seeded_case(seed, shape):
    """a seeded multi-atom density on a seeded skewed lattice (the style of test_gpu_neighbour_bits.seeded_case)"""
    rng = np.random.default_rng(seed)
    lat = synth.CUBIC6 * (0.8 + 0.4 * rng.random()) + 0.8 * (rng.random((3, 3)) - 0.5)
    na = int(rng.integers(2, 5))
    atoms = np.concatenate([rng.random((na, 3)), 0.5 + 0.3 * rng.random((na, 1)), 1 + 7 * rng.random((na, 1))], axis=1)
    rho = synth.synth_density(shape, lat, atoms)
    vl = np.divide(lat, shape)
    return rho, distance_matrix(vl), gradient_transform(vl)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = seeded_case(11, SHAPES[name])
    return _cases[name]


def load(ctx, rho, dm, tg):
    ctx.set_grid(rho.shape, dm, tg)
    ctx.upload_density(rho)
    ctx.vacuum_assign(None, 1.0)


def both_forms(ctx, run):
    """run(ctx) under the default form and under CROSS_CHECK_VOXEL_SWEEP: equal item by item, and the first took the bit form
    for every sweep, the second for none"""
    out, took = [], []
    for bits in (0, _lib.CROSS_CHECK_VOXEL_SWEEP):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
        s0 = ctx.sweep_stats()
        out.append(run(ctx))
        s1 = ctx.sweep_stats()
        took.append((s1[0] - s0[0], s1[1] - s0[1]))
    ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    assert took[0][0] > 0 and took[0][1] == 0, took
    assert took[1][0] == 0 and took[1][1] == took[0][0], took
    a, b = out
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    return a


def oracle_edges(rho, labels):
    import oracle
    known = np.zeros(rho.shape, np.int8)
    n = oracle.edge_find(known, rho, np.ascontiguousarray(labels, np.int32))
    return n, known


def half_space(shape, axis, start, length):
    """label 2 on [start, start + length) modulo the axis, 1 elsewhere: boundaries start-1|start and start+length-1|start+length"""
    lab = np.ones(shape, np.int32)
    idx = [slice(None)] * 3
    idx[axis] = (start + np.arange(length)) % shape[axis]
    lab[tuple(idx)] = 2
    return lab


def foreign_voxel_maps(shape):
    x0, y0, z0 = TILE
    spots = [(x0 + dx, y0 + dy, z0 + dz) for dx in (0, 3) for dy in (0, 7) for dz in (0, 63)]   # the tile's corners
    spots += [(x0, y0, z0 - 1), (x0, y0, z0 + 64), (x0 - 1, y0, z0), (x0 + 4, y0, z0), (x0, y0 - 1, z0), (x0, y0 + 8, z0)]   # its ring
    spots += [(x0 + 3, y0 + 7, z0 + 64), (x0 - 1, y0 - 1, z0 - 1)]   # ring corners: the side bits of a diagonal row
    for s in spots:
        lab = np.ones(shape, np.int32)
        lab[tuple(np.mod(s, shape))] = 3
        yield lab


def label_maps(kind, shape):
    rng = np.random.default_rng(5)
    if kind == 'random':          # every voxel an independent label of four: everything is an edge
        yield rng.integers(1, 5, shape).astype(np.int32)
    elif kind == 'blocks':        # 4-voxel blocks: triple and quadruple junctions
        small = rng.integers(1, 5, tuple(s // 4 for s in shape)).astype(np.int32)
        yield np.repeat(np.repeat(np.repeat(small, 4, 0), 4, 1), 4, 2)
    elif kind == 'half_spaces':   # a boundary on each tile face in turn, the wraps included: x 3|4, y 7|8, z 63|64, z nz-1|0
        yield half_space(shape, 0, 4, 5)
        yield half_space(shape, 1, 8, 3)
        yield half_space(shape, 2, 64, 64)     # 63|64 and 127|128 (16 x * x 128: 127|0)
        yield half_space(shape, 2, 0, 7)       # nz-1|0
        yield half_space(shape, 2, 127, 3)     # 126|127 and 129|130 (128: 1|2): one voxel inside the faces
    elif kind == 'foreign_voxel':
        yield from foreign_voxel_maps(shape)
    else:
        yield np.full(shape, 7, np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['random', 'blocks', 'half_spaces', 'foreign_voxel', 'uniform'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_label_maps_both_forms_equal_the_oracle(ctx, name, kind):
    """1. edge_find() on uploaded label maps (no -1, no table: every edge candidate takes the 27-point density test)."""
    rho, dm, tg = case(name)
    load(ctx, rho, dm, tg)
    for lab in label_maps(kind, rho.shape):
        def run(c):
            c.upload_labels(lab)
            return [c.edge_find(), c.download_known()]
        n, known = both_forms(ctx, run)
        want_n, want = oracle_edges(rho, lab)
        assert n == want_n and np.array_equal(known, want)
        if kind == 'uniform':
            assert n == 0 and (known == 2).all()
        elif kind == 'random':
            assert n > 0.99 * rho.size
        else:
            assert 0 < n < rho.size


def maximum_positions(shape):
    x0, y0, z0 = TILE
    i = (x0 + 1, y0 + 3, z0 + 26)   # an interior voxel of the tile
    return {'interior': (i, 0), 'x7': ((7, i[1], i[2]), 0), 'x8': ((8, i[1], i[2]), 0), 'xlast': ((shape[0] - 1, i[1], i[2]), 0),
            'x0': ((0, i[1], i[2]), 0), 'y15': ((i[0], 15, i[2]), 1), 'y8': ((i[0], 8, i[2]), 1), 'z63': ((i[0], i[1], 63), 2),
            'z64': ((i[0], i[1], 64), 2), 'z127': ((i[0], i[1], 127), 2), 'z0': ((i[0], i[1], 0), 2)}


@pytest.mark.gpu
@pytest.mark.parametrize('where', list(maximum_positions((16, 16, 128))))
@pytest.mark.parametrize('name', list(SHAPES))
def test_a_maximum_with_a_foreign_neighbour_is_no_edge(ctx, name, where):
    """2. refinement.py:374-383: two atoms centred on voxels, a half-space boundary one voxel from the first maximum, on either
    side of it along the axis under test.  The maximum sits inside a tile and on the tile faces, where it is a ring voxel of the
    neighbouring tile: it carries -1 (near an edge, no edge itself) and does not dilate.  Once on uploaded labels alone (the
    per-voxel test everywhere), once after a neargrid assignment (brick bytes and records, where the context keeps them)."""
    shape = SHAPES[name]
    m, axis = maximum_positions(shape)[where]
    other = tuple((np.array(m) + np.array(shape) // 2) % shape)
    atoms = np.array([[m[0] / shape[0], m[1] / shape[1], m[2] / shape[2], 0.45, 6.0],
                      [other[0] / shape[0], other[1] / shape[1], other[2] / shape[2], 0.4, 4.0]])
    rho = synth.synth_density(shape, synth.CUBIC6, atoms)
    vl = np.divide(synth.CUBIC6, shape)
    dm, tg = distance_matrix(vl), gradient_transform(vl)
    assert rho[m] == rho.max()
    for side in (1, -1):
        # foreign labels from m + 1 on (side 1) or up to m - 1 (side -1), a third of the axis long
        lab = half_space(shape, axis, m[axis] + 1 if side == 1 else m[axis] - shape[axis] // 3, shape[axis] // 3)
        want_n, want = oracle_edges(rho, lab)
        assert want[m] == -1, 'the case is built so that the maximum has a foreign neighbour and edges next to it'
        for assigned in (False, True):
            def run(c):
                load(c, rho, dm, tg)
                if assigned:
                    c.assign('neargrid')
                c.upload_labels(lab)
                return [c.edge_find(), c.download_known()]
            n, known = both_forms(ctx, run)
            assert known[m] == -1
            assert n == want_n and np.array_equal(known, want), (side, assigned)


def oracle_refine(rho, start, dm, tg, mode):
    """oracle.refine (thread_handlers.py:128-236) restated from its parts so that the last `known` comes back too"""
    import oracle
    v = start.copy()
    log = []
    check_mode, iters = mode
    known = np.zeros(rho.shape, np.int8)
    edges = oracle.edge_find(known, rho, v)
    if edges == 0:
        return v, log, known
    log.append((edges, oracle.refine_neargrid(known, known.copy(), rho, v, dm, tg)))
    it = 2
    while iters < 0 or it <= iters:
        if check_mode == 'all':
            known = np.zeros(rho.shape, np.int8)
            edges = oracle.edge_find(known, rho, v)
        else:
            _, edges = oracle.edge_check(known, rho, v)
        changed = oracle.refine_neargrid(known, known.copy(), rho, v, dm, tg)
        log.append((edges, changed))
        if changed == 0:
            break
        it += 1
    return v, log, known


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(SHAPES))
def test_assign_and_refine_both_forms_equal_the_oracle(ctx, name):
    """3. end to end: assign, then refine ('changed', 2) and ('all', -1) -- labels, maxima, logs and the last `known`.  (The
    assignment's oracle: the own-trajectory map ranked by first voxel, as in test_gpu_neighbour_bits.)"""
    rho, dm, tg = case(name)
    want, maxima = rough_common.rank_labels(rough_common.own_map(rho, np.zeros(rho.shape, np.int32), dm, tg, main_ties=True))

    def run(c):
        res = []
        for mode in REFINES:
            load(c, rho, dm, tg)
            res += [c.assign('neargrid'), np.ravel_multi_index(tuple(c.maxima().T), rho.shape), c.download_labels(np.int64)]
            res += [c.refine(*mode), c.download_labels(np.int32), c.download_known()]
        return res
    got = both_forms(ctx, run)
    for k, mode in enumerate(REFINES):
        n, got_maxima, assigned, log, labels, known = got[6 * k:6 * k + 6]
        assert n == maxima.shape[0] and np.array_equal(got_maxima, maxima) and np.array_equal(assigned, want)
        v, want_log, want_known = oracle_refine(rho, want.astype(np.int32), dm, tg, mode)
        assert log == want_log, mode
        assert np.array_equal(labels, v), mode
        assert np.array_equal(known, want_known), mode


# ---- 4. the formula, without a GPU ---------------------------------------------------------------------------------------
def brute_edges(lab):
    e = np.zeros(lab.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                e |= np.roll(lab, (dx, dy, dz), (0, 1, 2)) != lab
    return e


def dilate(e):
    n = np.zeros(e.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                n |= np.roll(e, (dx, dy, dz), (0, 1, 2))
    return n


def mask_edges(lab):
    """edge = ~uniform from 17 row masks, as k_edge_sweep_bits forms them (there a row of z is a 64-bit ballot)"""
    def r(a, s, ax):
        return np.roll(a, s, ax)
    T = (r(lab, 1, 2) == lab) & (r(lab, -1, 2) == lab)       # z - 1, z, z + 1 of the row carry one label
    Cy = lab == r(lab, -1, 1)                                 # row (x, y) against (x, y + 1) at the same z
    Cx = lab == r(lab, -1, 0)                                 # row (x, y) against (x + 1, y)
    P = T & r(T, 1, 1) & r(T, -1, 1) & Cy & r(Cy, 1, 1)       # the 9 voxels around (y, z) in plane x
    return ~(P & r(P, 1, 0) & r(P, -1, 0) & Cx & r(Cx, 1, 0))


def mask_edges_q(lab):
    """the kernel's shorter route to P: Q = Z(y-1) & Z(y) & Z(y+1) & Cy(y-1) & Cy(y) with Z[z] = l(z) == l(z + 1), P = Q & rotl(Q)"""
    def r(a, s, ax):
        return np.roll(a, s, ax)
    Z = lab == r(lab, -1, 2)
    Cy = lab == r(lab, -1, 1)
    Cx = lab == r(lab, -1, 0)
    Q = Z & r(Z, 1, 1) & r(Z, -1, 1) & Cy & r(Cy, 1, 1)
    P = Q & r(Q, 1, 2)
    return ~(P & r(P, 1, 0) & r(P, -1, 0) & Cx & r(Cx, 1, 0))


def test_the_mask_formula_equals_the_27_box_test():
    """200 random periodic label maps of 2-5 labels, 3-8 voxels per axis, every other one in 4-voxel blocks: the masks give the
    edges of the brute-force test, and so the same dilation."""
    rng = np.random.default_rng(3)
    for trial in range(200):
        shape = tuple(int(s) for s in rng.integers(3, 9, 3))
        k = int(rng.integers(2, 6))
        lab = rng.integers(0, k, shape)
        if trial % 2:
            lab = np.repeat(np.repeat(np.repeat(rng.integers(0, k, (2, 2, 2)), 4, 0), 4, 1), 4, 2)[:shape[0], :shape[1], :shape[2]]
        e0, e1, e2 = brute_edges(lab), mask_edges(lab), mask_edges_q(lab)
        assert np.array_equal(e0, e1) and np.array_equal(e0, e2), trial
        assert np.array_equal(dilate(e0), dilate(e1))

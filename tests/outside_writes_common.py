"""Shared by tests/test_outside_writes_cpu.py and tests/test_gpu_outside_writes.py: label writes from outside an assignment between
the steps of the ABI -- the inputs, each writer as data (which voxels or planes it writes, with what), the host-side image of
the write, and the oracle's expectation of the call that follows.  Every expectation is the oracle's on the patched map, built
as tests/soak_vs_oracle.py builds its own, and memoised.

Grid V: the 32^3 triclinic two-atom density of test_gpu_neighbour_bits.vacuum_brick_case with its tolerance 2 * BACKGROUND: 50 of
its 64 bricks lie wholly at or below the tolerance.  xb_vacuum_assign(tol or none), a writer, then an assignment.

Grid S: no vacuum, the three atoms of history_common.ATOMS_A.  xb_assign(neargrid), a writer, then a refinement.  On the
triclinic cell at ATOMS_A's own widths none of 16 x 16 x 128, 16 x 24 x 128 and 32 x 32 x 128 certifies a brick (measured on
an MI355X: box_stats() == (3, 0) on all three, with and without widening), so S is the smallest of them on the CUBIC cell with
the widths times 1.5, the narrowest of 1.5, 2, 2.5, 3 that does: 16 x 16 x 128 -- 13 certified bricks (6656 voxels: bricks
(0, 0, 1..6) and (1, 0, 9..15)), edge_find by row bit masks (3 maxima in 64 bricks)."""
import functools

import numpy as np

import oracle
from history_common import ATOMS_A
from pybader_amd import synth
from pybader_amd.interface import distance_matrix, gradient_transform
from rough_common import own_map, rank_labels
from test_gpu_neighbour_bits import vacuum_brick_case
from test_gpu_sums import swapped

V_WRITERS = {   # name -> the tolerance of the xb_vacuum_assign before it
    'scatter_zero_into_vacuum_bricks': 'tol', 'planes_with_vacuum_bricks_zeroed': 'tol', 'scatter_vacuum_above_tolerance': 'tol',
    'scatter_vacuum_without_tolerance': None, 'planes_with_vacuum_without_tolerance': None}
V_FOLLOWERS = ('neargrid', 'ongrid', 'neargrid_refine')
V_REFINE = ('all', -1)

S_SHAPE = (16, 16, 128)
S_WRITERS = ('scatter_foreign_label', 'planes_of_another_map', 'volume_assign_swap', 'import_labels', 'vacuum_assign_tol')
S_REFINES = (('all', -1), ('changed', 2))
S_VOXEL = (4, 4, 28)      # the centre of brick (0, 0, 3): deep inside a certified brick of the basin of the maximum (4, 4, 32)
S_SWAP = np.array([1, 0, 2], np.int64)
S_TOL = 0.05


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


# ---- grid V ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_v():
    """(rho, dist_mat, T_grad, tol)"""
    rho, dm, tg, tol = vacuum_brick_case()
    return _frozen(rho), dm, tg, tol


@functools.lru_cache(maxsize=None)
def v_vacuum_map(with_tol):
    """what xb_vacuum_assign leaves: -1 where rho <= tol, 0 elsewhere (all 0 without a tolerance)"""
    rho, _, _, tol = grid_v()
    vol0, _, _ = oracle.vacuum_assign(rho, np.zeros(rho.shape, np.int32), tol if with_tol else float('nan'), rho, 1.0)
    return _frozen(vol0)


@functools.lru_cache(maxsize=None)
def v_vacuum_bricks():
    """bool[4, 4, 4]: the 8^3 bricks whose every voxel lies at or below the tolerance"""
    rho, _, _, tol = grid_v()
    return _frozen(rho.reshape(4, 8, 4, 8, 4, 8).max(axis=(1, 3, 5)) <= tol)


def _brick_voxels(bricks, offsets):
    shape = grid_v()[0].shape
    return np.array([np.ravel_multi_index(tuple(8 * b + o for b, o in zip(brick, off)), shape) for brick in bricks for off in offsets], np.int64)


@functools.lru_cache(maxsize=None)
def v_write(writer):
    """the write as data: {'kind': 'scatter', 'idx', 'labels'} or {'kind': 'planes', 'xa', 'xb', 'planes'}, and 'bricks': the whole-
    vacuum bricks it writes into (a list of brick indices; empty where it writes elsewhere)"""
    rho, dm, tg, tol = grid_v()
    vac = v_vacuum_bricks()
    wb = [tuple(int(x) for x in b) for b in np.argwhere(vac)]
    if writer == 'scatter_zero_into_vacuum_bricks':     # first, middle and last whole-vacuum brick: a corner, the centre, the far corner
        bricks = [wb[0], wb[len(wb) // 2], wb[-1]]
        idx = _brick_voxels(bricks, [(0, 0, 0), (4, 4, 4), (7, 7, 7)])
        return {'kind': 'scatter', 'idx': idx, 'labels': np.zeros(idx.size, np.int32), 'bricks': bricks}
    if writer == 'planes_with_vacuum_bricks_zeroed':    # the planes of brick row 2, two of its whole-vacuum bricks zeroed
        bricks = [b for b in wb if b[0] == 2][:2]
        planes = v_vacuum_map(True)[16:24].copy()
        for b in bricks:
            planes[:, 8 * b[1]:8 * b[1] + 8, 8 * b[2]:8 * b[2] + 8] = 0
        return {'kind': 'planes', 'xa': 16, 'xb': 24, 'planes': _frozen(planes), 'bricks': bricks}
    if writer in ('scatter_vacuum_above_tolerance', 'scatter_vacuum_without_tolerance'):
        # the maximum of the second basin (its whole basin turns to vacuum) and three other voxels above the tolerance
        base = v_expect(None, 'neargrid')
        above = np.flatnonzero(rho.reshape(-1) > tol)
        idx = np.array([base['maxima'][1]] + [int(above[k]) for k in (above.size // 7, above.size // 2, above.size - 5)], np.int64)
        assert len(set(idx.tolist())) == idx.size and (rho.reshape(-1)[idx] > tol).all()
        return {'kind': 'scatter', 'idx': idx, 'labels': np.full(idx.size, -1, np.int32), 'bricks': []}
    if writer == 'planes_with_vacuum_without_tolerance':    # four planes of the tolerance's vacuum map over the all-zero one
        planes = v_vacuum_map(True)[12:16].copy()
        assert (planes == -1).any() and (planes == 0).any()
        return {'kind': 'planes', 'xa': 12, 'xb': 16, 'planes': _frozen(planes), 'bricks': []}
    raise KeyError(writer)


def apply_write(labels, w):
    """the host-side image of a write"""
    out = np.array(labels, dtype=np.int32, copy=True)
    if w['kind'] == 'scatter':
        out.reshape(-1)[w['idx']] = w['labels']
    else:
        out[w['xa']:w['xb']] = w['planes']
    return out


def v_patched(writer):
    if writer is None:
        return v_vacuum_map(True)
    return _frozen(apply_write(v_vacuum_map(V_WRITERS[writer] == 'tol'), v_write(writer)))


@functools.lru_cache(maxsize=None)
def v_expect(writer, follower, with_tol=True):
    """the oracle's result of `follower` on the vacuum map patched by `writer` (None: unpatched, with or without the tolerance):
    {'maxima': linear indices in basin order, 'map', and for neargrid_refine 'log'}"""
    rho, dm, tg, tol = grid_v()
    vol0 = v_patched(writer) if writer is not None else v_vacuum_map(with_tol)
    if follower == 'ongrid':
        bmax, lab = oracle.bader_calc('ongrid', rho, vol0.copy(), dm, tg, 1)
        maxima = np.ravel_multi_index(tuple(np.asarray(bmax).T), rho.shape) if len(bmax) else np.zeros(0, np.int64)
        return {'maxima': maxima, 'map': _frozen(lab.astype(np.int64))}
    lab, maxima = rank_labels(own_map(rho, vol0, dm, tg, main_ties=True))
    if follower == 'neargrid':
        return {'maxima': maxima, 'map': _frozen(lab)}
    v = lab.astype(np.int32).copy()
    log = []
    oracle.refine('neargrid', V_REFINE, rho, v, dm, tg, 1, log=log)
    return {'maxima': maxima, 'map': _frozen(v.astype(np.int64)), 'log': [tuple(x) for x in log]}


def same(a, b):
    return (np.array_equal(a['maxima'], b['maxima']) and np.array_equal(a['map'], b['map']) and a.get('log') == b.get('log'))


# ---- grid S ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_s():
    """(rho, dist_mat, T_grad)"""
    atoms = ATOMS_A.copy()
    atoms[:, 3] *= 1.5
    rho = synth.synth_density(S_SHAPE, synth.CUBIC6, atoms)
    vl = np.divide(synth.CUBIC6, S_SHAPE)
    return _frozen(rho), distance_matrix(vl), gradient_transform(vl)


@functools.lru_cache(maxsize=None)
def s_assignment():
    """the oracle's neargrid assignment: (labels int32, maxima)"""
    rho, dm, tg = grid_s()
    lab, maxima = rank_labels(own_map(rho, np.zeros(S_SHAPE, np.int32), dm, tg, main_ties=True))
    return _frozen(lab.astype(np.int32)), maxima


@functools.lru_cache(maxsize=None)
def s_write(writer):
    """the write as data: kind 'scatter' / 'planes' as v_write, or {'kind': 'volume_assign', 'swap'}, {'kind': 'import', 'labels'},
    {'kind': 'vacuum_assign', 'tol'}; 'start': the map the refinement starts from"""
    rho, dm, tg = grid_s()
    lab, maxima = s_assignment()
    n = len(maxima)
    if writer == 'scatter_foreign_label':
        v = int(np.ravel_multi_index(S_VOXEL, S_SHAPE))
        w = {'kind': 'scatter', 'idx': np.array([v], np.int64), 'labels': np.array([(int(lab.reshape(-1)[v]) + 1) % n], np.int32)}
    elif writer == 'planes_of_another_map':     # four planes across a brick boundary from the map with its labels rotated by one
        w = {'kind': 'planes', 'xa': 6, 'xb': 10, 'planes': _frozen(((lab + 1) % n)[6:10].astype(np.int32))}
    elif writer == 'volume_assign_swap':
        return {'kind': 'volume_assign', 'swap': S_SWAP, 'start': _frozen(swapped(lab, S_SWAP).astype(np.int32))}
    elif writer == 'import_labels':             # the map with its labels rotated by two, from a device array
        other = _frozen(((lab + 2) % n).astype(np.int32))
        return {'kind': 'import', 'labels': other, 'start': other}
    elif writer == 'vacuum_assign_tol':
        vol0, _, _ = oracle.vacuum_assign(rho, np.zeros(S_SHAPE, np.int32), S_TOL, rho, 1.0)
        assert 0 < (vol0 == -1).mean() < 1
        return {'kind': 'vacuum_assign', 'tol': S_TOL, 'start': _frozen(vol0)}
    else:
        raise KeyError(writer)
    w['start'] = _frozen(apply_write(lab, w))
    return w


@functools.lru_cache(maxsize=None)
def s_expect(writer, mode):
    """the oracle's refinement `mode` of the map `writer` leaves (None: the assignment itself): {'log', 'map'}"""
    rho, dm, tg = grid_s()
    v = (s_assignment()[0] if writer is None else s_write(writer)['start']).copy()
    log = []
    oracle.refine('neargrid', mode, rho, v, dm, tg, 1, log=log)
    return {'log': [tuple(x) for x in log], 'map': _frozen(v)}

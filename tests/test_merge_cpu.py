"""The host side of the persistence merge (pybader_amd/merge.py, xb_merge_basins) and the plain numpy restatement of the
definition in include/bader_hip.h / DESIGN.md section 15 that tests/test_gpu_merge.py compares the kernels with.

`reference_merge` goes round by round: it relabels the map through the current roots, asks
test_adjacency_cpu.reference_adjacency for the pairs and their saddles, and decides per root.  Everything in it is an integer, a
comparison of keys, an index or one float64 subtraction, so it is compared with `==`: no tolerance anywhere.

The cases of tests/test_gpu_merge.py are built here (`cases`, `expected`) and run through the restatement without a GPU, so
that what the GPU test compares is known not to be vacuous."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, adjacency
from test_adjacency_cpu import ORTHO_DIRS, key, reference_adjacency, unkey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


# ---- the definition, restated -------------------------------------------------------------------------------------------------
def reference_merge(rho, labels, n, dirs, max_idx, tol, max_rounds):
    """-> dict(root int32[n], merge_round int32[n], merge_persistence f64[n], rounds, n_survivors, converged, parent int64[n])"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    peak = rho.reshape(-1)[np.asarray(max_idx, dtype=np.int64)]
    pk = key(peak).tolist()
    inside = (lab >= 0) & (lab < n)

    def above(b, a):
        return pk[b] > pk[a] or (pk[b] == pk[a] and b < a)

    cur = np.arange(n, dtype=np.int64)
    parent = np.arange(n, dtype=np.int64)
    mround = np.full(n, -1, np.int32)
    mpers = np.full(n, INF)
    rounds, converged = 0, False
    while rounds < max_rounds:
        relabelled = np.where(inside, cur[np.where(inside, lab, 0)], -1)
        pairs, _, saddle, _ = reference_adjacency(rho, relabelled, n, dirs)
        best = {}                                                      # lower -> [saddle key, saddle, target]
        for (a, b), s, sk in zip(pairs.tolist(), saddle, key(saddle).tolist()):
            lower, upper = (a, b) if above(b, a) else (b, a)
            e = best.get(lower)
            if e is None or sk > e[0]:
                best[lower] = [sk, s, upper]
            elif sk == e[0] and upper < e[2]:
                e[2] = upper
        merged = 0
        for m in np.flatnonzero(cur == np.arange(n)).tolist():         # the roots
            pers = INF
            if m in best:
                with np.errstate(invalid='ignore'):
                    pers = peak[m] - best[m][1]
            mpers[m] = pers
            if pers < tol:
                parent[m], mround[m] = best[m][2], rounds
                merged += 1
        rounds += 1
        if not merged:
            converged = True
            break
        for m in range(n):
            r = cur[m]
            while parent[r] != r:
                r = parent[r]
            cur[m] = r
    return {'root': cur.astype(np.int32), 'merge_round': mround, 'merge_persistence': mpers, 'rounds': rounds,
            'n_survivors': int((mround < 0).sum()), 'converged': converged, 'parent': parent}


def chain_depth(parent):
    """the most links from a label to its root"""
    deepest = 0
    for m in range(len(parent)):
        d = 0
        while parent[m] != m:
            m, d = parent[m], d + 1
        deepest = max(deepest, d)
    return deepest


def maxima_of(rho, labels, n):
    """max_idx[m]: the voxel of label m with the largest key(rho), the smallest index on ties; voxel 0 for an absent label"""
    lab, kv = np.asarray(labels).reshape(-1), key(rho).reshape(-1)
    out = np.zeros(n, np.int64)
    order = np.lexsort((-np.arange(lab.size), kv))                   # ascending key, descending index: the last per label wins
    ok = (lab[order] >= 0) & (lab[order] < n)
    out[lab[order][ok]] = order[ok]
    return out


# ---- the cases of tests/test_gpu_merge.py -----------------------------------------------------------------------------------------
TOLS = ('zero', 'mid', 'inf')


def cases(shape):
    """(density name, map name, lattice name) of a shape, in the order both test files walk them"""
    import test_gpu_adjacency as tga
    return [(d, m, l) for d in tga.densities(shape) for m in tga.label_maps(shape) for l in tga.LATTICES]


@functools.lru_cache(maxsize=None)
def expected(shape, dname, mname, lname):
    """-> (rho, lab, n, dirs, max_idx, {tol name: (tol, reference_merge's result)}); computed once, shared, never changed"""
    import test_gpu_adjacency as tga
    rho = tga.densities(shape)[dname]
    lab, ns = tga.label_maps(shape)[mname]
    n = ns[0]
    dirs, _ = tga.directions(shape, lname)
    max_idx = maxima_of(rho, lab, n)
    zero = reference_merge(rho, lab, n, dirs, max_idx, 0.0, 64)
    finite = zero['merge_persistence'][np.isfinite(zero['merge_persistence'])]
    # a mid quantile of the round-0 persistences; the next double above it, so that the median label itself merges
    mid = float(np.nextafter(np.quantile(finite, 0.5, method='lower'), INF)) if finite.size else 1.0
    out = {'zero': (0.0, zero)}
    for name, tol in (('mid', mid), ('inf', INF)):
        out[name] = (tol, reference_merge(rho, lab, n, dirs, max_idx, tol, 64))
    max_idx.flags.writeable = False
    return rho, lab, n, dirs, max_idx, out


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_three_entries():
    hdr = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    want = {
        'xb_merge_basins': ['xb_ctx *c', 'const int32_t *dirs', 'int n_dirs', 'int64_t n', 'const int64_t *max_idx', 'double tol',
                            'int64_t max_rounds', 'int64_t *rounds', 'int64_t *n_survivors', 'int *converged'],
        'xb_merge_fetch': ['xb_ctx *c', 'int32_t *root', 'int32_t *merge_round', 'double *merge_persistence', 'int64_t capacity'],
        'xb_merge_release': ['xb_ctx *c'],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, f'include/bader_hip.h does not declare {name}'
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args)
    assert callable(_lib.Context.merge_basins) and callable(_lib.Context.merge_release)


def test_bader_has_the_threshold_and_it_is_off():
    from pybader_amd.interface import Bader
    from pybader_amd import merge
    assert Bader.persistence_tol is None and callable(Bader.merge_volumes)
    assert callable(merge.merge_basins) and callable(merge.Merge.apply)


def test_merge_object():
    from pybader_amd.merge import Merge
    m = Merge(np.array([0, 0, 2, 2, 4], np.int32), np.array([-1, 0, -1, 1, -1], np.int32), np.zeros(5), 3, True)
    assert m.survivors.tolist() == [0, 2, 4] and m.survivors.dtype == np.int64 and len(m) == 3
    assert m.swap.tolist() == [0, 0, 1, 1, 2] and m.swap.dtype == np.int64


# ---- hand-checked cases -------------------------------------------------------------------------------------------------------------
def line(z, labels):
    """a profile along z laid out in (3, 3, len(z)), labels per z; -> (rho, lab, n, max_idx)"""
    shape = (3, 3, len(z))
    rho = np.ascontiguousarray(np.broadcast_to(np.array(z, dtype=np.float64), shape))
    lab = np.ascontiguousarray(np.broadcast_to(np.array(labels, dtype=np.int32), shape))
    n = int(max(labels)) + 1
    return rho, lab, n, maxima_of(rho, lab, n)


def test_the_double_well():
    """the profile of test_adjacency_cpu.test_persistence_of_a_double_well: maxima 5 (label 0) and 3 (label 1), the pass between
    them at 2: label 1 has persistence 1"""
    z = [1.5, 3.0, 5.0, 3.0, 2.0, 2.5, 3.0, 2.0, 1.0, 0.5, 0.75, 1.0]
    rho, lab, n, max_idx = line(z, [0] * 5 + [1] * 5 + [0] * 2)
    assert rho.reshape(-1)[max_idx].tolist() == [5.0, 3.0]
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 1.5, 64)
    assert r['root'].tolist() == [0, 0] and r['merge_round'].tolist() == [-1, 0] and r['merge_persistence'].tolist() == [INF, 1.0]
    assert (r['rounds'], r['n_survivors'], r['converged']) == (2, 1, True)
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 1.0, 64)            # the comparison is strict
    assert r['root'].tolist() == [0, 1] and r['merge_round'].tolist() == [-1, -1] and r['merge_persistence'].tolist() == [INF, 1.0]
    assert (r['rounds'], r['n_survivors'], r['converged']) == (1, 2, True)


def test_equal_peaks_merge_into_the_smaller_label():
    """a plateau of height 3 split into two labels: equal bits, so label 0 is above label 1, and the saddle is the plateau itself"""
    rho, lab, n, max_idx = line([3.0, 3.0, 3.0, 3.0, 1.0, 1.0], [0, 0, 1, 1, 1, 0])
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 1e-300, 64)
    assert r['root'].tolist() == [0, 0] and r['merge_round'].tolist() == [-1, 0] and r['merge_persistence'].tolist() == [INF, 0.0]
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 0.0, 64)
    assert r['root'].tolist() == [0, 1] and r['merge_persistence'].tolist() == [INF, 0.0]
    # adjacency.persistence puts neither above the other
    pairs, _, saddle, _ = reference_adjacency(rho, lab, n, ORTHO_DIRS)
    assert adjacency.persistence(pairs, saddle, np.array([3.0, 3.0])).tolist() == [INF, INF]


def test_a_chain_collapses_in_one_round():
    """a staircase, a label per step: each step's highest saddle towards the step above is its own height; the lowest step meets
    the highest through the wrap at the same saddle as its other neighbour, and that tie goes to the smaller label"""
    rho, lab, n, max_idx = line([5.0, 4.0, 3.0, 2.0, 1.0, 0.5], [0, 1, 2, 3, 4, 5])
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 0.25, 64)
    assert r['parent'].tolist() == [0, 0, 1, 2, 3, 0] and chain_depth(r['parent']) == 4
    assert r['root'].tolist() == [0] * 6 and r['merge_round'].tolist() == [-1, 0, 0, 0, 0, 0]
    assert r['merge_persistence'].tolist() == [INF, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert (r['rounds'], r['n_survivors'], r['converged']) == (2, 1, True)
    one = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 0.25, 1)          # max_rounds stops it: not converged
    assert (one['rounds'], one['n_survivors'], one['converged']) == (1, 1, False)
    assert one['root'].tolist() == [0] * 6 and one['merge_round'].tolist() == r['merge_round'].tolist()


def test_a_second_round_is_needed():
    """high | low | middle | vacuum: the middle label's only neighbour is the low one, which is below it; once the low one
    has been absorbed by the high one, the middle label has a neighbour above it"""
    rho, lab, n, max_idx = line([10.0, 1.0, 5.0, 0.0], [0, 1, 2, -1])
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 4.5, 64)
    assert r['merge_round'].tolist() == [-1, 0, 1] and r['root'].tolist() == [0, 0, 0]
    assert r['merge_persistence'].tolist() == [INF, 0.0, 4.0]
    assert (r['rounds'], r['n_survivors'], r['converged']) == (3, 1, True)
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 4.0, 64)
    assert r['merge_round'].tolist() == [-1, 0, -1] and r['root'].tolist() == [0, 0, 2] and r['rounds'] == 2
    assert r['merge_persistence'].tolist() == [INF, 0.0, 4.0], 'a survivor reports the last round run'


def test_a_target_tie_goes_to_the_smallest_label():
    """label 1 lies between label 2 (peak 10) and label 0 (peak 5), with the saddle 1 on both sides"""
    rho, lab, n, max_idx = line([10.0, 1.0, 5.0, 0.0], [2, 1, 0, -1])
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, 0.5, 64)
    assert r['parent'].tolist() == [0, 0, 2] and r['merge_round'].tolist() == [-1, 0, -1]


def test_a_nan_saddle_merges_nothing():
    """label 1 touches label 0 through a voxel that holds a negative NaN, below every number in key order: its saddle is that
    NaN, its persistence a NaN, and no tolerance merges it"""
    nan = -np.abs(np.float64('nan'))
    rho, lab, n, max_idx = line([10.0, nan, 1.0, 0.0], [0, 1, 1, -1])
    assert rho.reshape(-1)[max_idx].tolist() == [10.0, 1.0]
    r = reference_merge(rho, lab, n, ORTHO_DIRS, max_idx, INF, 64)
    assert r['root'].tolist() == [0, 1] and r['merge_round'].tolist() == [-1, -1] and r['rounds'] == 1
    assert r['merge_persistence'][0] == INF and np.isnan(r['merge_persistence'][1])


def test_round_zero_is_adjacency_persistence_when_the_peaks_differ():
    rng = np.random.default_rng(23)
    shape, n = (5, 7, 11), 9
    rho = rng.random(shape)
    lab = rng.integers(0, n, shape).astype(np.int32)
    max_idx = maxima_of(rho, lab, n)
    peak = rho.reshape(-1)[max_idx]
    assert len(np.unique(key(peak))) == n
    dirs, _ = adjacency.active_directions(np.diag([4.0, 5.5, 7.25]) / np.array(shape, float)[:, None])
    pairs, _, saddle, _ = reference_adjacency(rho, lab, n, dirs)
    r = reference_merge(rho, lab, n, dirs, max_idx, 0.0, 1)
    assert np.array_equal(r['merge_persistence'], adjacency.persistence(pairs, saddle, peak))
    assert np.isfinite(r['merge_persistence']).sum() == n - 1
    # maxima_of: ties go to the smallest index, an absent label to voxel 0
    assert maxima_of(np.ones((2, 2, 2)), np.array([1, 1, 0, 0, 3, 3, 1, 0]).reshape(2, 2, 2), 4).tolist() == [2, 0, 0, 4]
    assert unkey(key(peak)).tolist() == peak.tolist()


# ---- the inputs of the GPU test are not vacuous ------------------------------------------------------------------------------------------
def _shapes_and_densities():
    import test_gpu_adjacency as tga
    return [(s, d) for s in tga.SHAPES for d in ('smooth', 'three values', 'signed')]


@pytest.mark.parametrize('shape,dname', _shapes_and_densities())
def test_the_gpu_cases_merge_chain_and_take_rounds(shape, dname):
    full = []
    for d, mname, lname in cases(shape):
        if d != dname:
            continue
        rho, lab, n, dirs, max_idx, per_tol = expected(shape, dname, mname, lname)
        assert set(per_tol) == set(TOLS)
        zero = per_tol['zero'][1]
        assert zero['n_survivors'] == n and zero['rounds'] == 1 and zero['converged'], 'a threshold of 0 merges nothing'
        for tname, (tol, r) in per_tol.items():
            merges, depth = n - r['n_survivors'], chain_depth(r['parent'])
            print(f'{shape} {dname} / {mname} / {lname} / {tname}: n {n} merges {merges} survivors {r["n_survivors"]} '
                  f'depth {depth} rounds {r["rounds"]}')
            assert r['converged'] and np.array_equal(r['root'][r['root']], r['root'])
            if merges > 0 and r['n_survivors'] > 1 and depth >= 3 and r['rounds'] >= 2:
                full.append((mname, lname, tname))
    assert full, 'no case of this shape and density merges, keeps two survivors, chains three deep and takes two rounds'

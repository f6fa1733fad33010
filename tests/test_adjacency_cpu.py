"""The host side of the basin adjacency (pybader_amd/adjacency.py, weight.voronoi_areas, xb_adjacency) and the plain numpy
restatement of the definition in include/bader_hip.h / DESIGN.md section 14 that tests/test_gpu_adjacency.py compares the
kernels with.

`reference_adjacency` rolls the label map and the density once per direction and keeps a dictionary per pair.  Everything in
it is an integer, a comparison of keys or an index, so it is compared with `==`: no tolerance anywhere."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, adjacency, synth, weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIC = np.array([[5.0, 0.3, -0.2], [1.4, 6.1, 0.5], [-0.8, 1.2, 6.9]])      # the triclinic cell of tests/test_multipole_cpu.py
CUBIC = synth.CUBIC6
ORTHO = np.diag([4.0, 5.5, 7.25])
ORTHO_DIRS = [(0, 0, 1), (0, 1, 0), (1, 0, 0)]

try:
    with open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_adjacency.h')) as _f:
        AJ_DENSE = int(re.search(r'^#define AJ_DENSE (\d+)', _f.read(), re.M).group(1))
except OSError:          # (the tests below then fail one by one instead of the module failing to import)
    AJ_DENSE = 0


# ---- the definition, restated -------------------------------------------------------------------------------------------------
def key(x):
    """key(x) = bits(x) ^ (bits(x) >> 63 ? ~0 : 1 << 63), as uint64"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ np.uint64(1 << 63))


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k ^ np.uint64(1 << 63), ~k).view(np.float64)


def reference_adjacency(rho, labels, n, dirs):
    """-> (pairs int32[P, 2] ascending, facets int64[P, K], saddle f64[P], saddle_facet int64[P])"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    assert lab.shape == rho.shape
    dirs = [tuple(int(x) for x in d) for d in np.asarray(dirs).reshape(-1, 3)]
    kv = key(rho)
    table = {}
    for k, d in enumerate(dirs):
        back = tuple(-x for x in d)
        lab_u = np.roll(lab, back, axis=(0, 1, 2))            # lab_u[v] = lab[v + d], wrapped on every axis
        s = np.minimum(kv, np.roll(kv, back, axis=(0, 1, 2)))    # the smaller of the two, in key order
        counts = (lab >= 0) & (lab < n) & (lab_u >= 0) & (lab_u < n) & (lab != lab_u)
        a, b, s = lab.reshape(-1), lab_u.reshape(-1), s.reshape(-1)
        for v in np.flatnonzero(counts.reshape(-1)).tolist():
            pair = (min(a[v], b[v]), max(a[v], b[v]))
            e = table.setdefault(pair, {'facets': [0] * len(dirs), 'key': None, 'facet': None})
            e['facets'][k] += 1
            f, sk = v * 8 + k, int(s[v])
            if e['key'] is None or sk > e['key'] or (sk == e['key'] and f < e['facet']):
                e['key'], e['facet'] = sk, f
    order = sorted(table)
    pairs = np.array(order, dtype=np.int32).reshape(-1, 2)
    facets = np.array([table[p]['facets'] for p in order], dtype=np.int64).reshape(-1, len(dirs))
    saddle = unkey(np.array([table[p]['key'] for p in order], dtype=np.uint64))
    sfacet = np.array([table[p]['facet'] for p in order], dtype=np.int64)
    return pairs, facets, saddle, sfacet


def same(got, want):
    """pairs and their order, facet counts, saddle bits, saddle facet"""
    assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype
    assert np.array_equal(got[1], want[1]) and got[1].shape == want[1].shape
    assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
    assert np.array_equal(got[3], want[3])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_three_entries():
    hdr = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    want = {
        'xb_adjacency': ['xb_ctx *c', 'const int32_t *dirs', 'int n_dirs', 'int64_t n', 'int64_t *n_pairs'],
        'xb_adjacency_fetch': ['xb_ctx *c', 'int32_t *a', 'int32_t *b', 'int64_t *facets', 'double *saddle',
                               'int64_t *saddle_facet', 'int64_t capacity'],
        'xb_adjacency_release': ['xb_ctx *c'],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, f'include/bader_hip.h does not declare {name}'
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args)
    assert callable(_lib.Context.adjacency) and callable(_lib.Context.adjacency_release)
    assert 2 <= AJ_DENSE and AJ_DENSE * (AJ_DENSE - 1) // 2 * 15 * 8 <= 4 << 20, 'the largest dense table fits the L2 of an XCD'
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'bader_hip.hip')).read()
    assert re.search(r'which < 0 \|\| which >= XB_TIMER_COUNT\b', src) and 'TimedKernel tk[XB_TIMER_COUNT]' in src
    assert 0 <= _lib.XB_TIMER_ADJACENCY < _lib.XB_TIMER_COUNT, "xb_adjacency's timer is one of the slots the bounds check admits"


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.adjacency_flag is False and callable(Bader.bond_surfaces)


# ---- two half spaces ------------------------------------------------------------------------------------------------------------
def test_two_half_spaces():
    shape = (6, 5, 4)
    lab = np.zeros(shape, np.int32)
    lab[3:] = 1
    rho = synth.synth_density(shape, CUBIC)
    dirs, areas = adjacency.active_directions(CUBIC / np.array(shape, float)[:, None])
    assert [tuple(d) for d in dirs] == ORTHO_DIRS
    pairs, facets, saddle, sfacet = reference_adjacency(rho, lab, 2, dirs)
    assert pairs.tolist() == [[0, 1]]
    assert facets.tolist() == [[0, 0, 2 * 5 * 4]]                      # the planes x = 2|3 and x = 5|0
    b, c = CUBIC[1], CUBIC[2]
    assert adjacency.facet_area(facets, areas)[0] == 40 * (np.linalg.norm(np.cross(b, c)) / (5 * 4))
    # the saddle: the largest min(rho[v], rho[v + x]) over the two boundary planes, by hand
    cand = np.concatenate([np.minimum(rho[2], rho[3]).reshape(-1), np.minimum(rho[5], rho[0]).reshape(-1)])
    assert saddle[0] == cand.max()
    v, k = divmod(int(sfacet[0]), 8)
    p = np.unravel_index(v, shape)
    assert k == 2 and p[0] in (2, 5) and min(rho[p], rho[(p[0] + 1) % 6, p[1], p[2]]) == saddle[0]
    voxels, pos = adjacency.saddle_geometry(sfacet, dirs, shape, CUBIC)
    assert voxels[0, 0].tolist() == list(p) and voxels[0, 1].tolist() == [(p[0] + 1) % 6, p[1], p[2]]
    assert pos[0].tolist() == [p[0] + 0.5, 6.0 * p[1] / 5.0, 6.0 * p[2] / 4.0]      # voxel spacing 1 along x: the midpoint is exact
    # labels outside [0, n) bound nothing: with n = 1 there is no pair, and a vacuum plane between the halves separates them
    assert reference_adjacency(rho, lab, 1, dirs)[0].shape == (0, 2)
    lab2 = lab.copy()
    lab2[2] = -1
    lab2[5] = 7
    assert reference_adjacency(rho, lab2, 2, dirs)[0].shape == (0, 2)


# ---- voronoi_areas ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,lat,shape', [('cubic', CUBIC, (6, 6, 6)), ('ortho', ORTHO, (5, 7, 11)), ('tric', TRIC, (5, 7, 11)),
                                            ('synth tric', synth.TRICLINIC, (40, 36, 44))])
def test_voronoi_areas(name, lat, shape):
    vl = lat / np.array(shape, float)[:, None]
    areas, alpha = weight.voronoi_areas(vl), weight.voronoi_weights(vl)
    assert areas.shape == (3, 3, 3) and areas[0, 0, 0] == 0.0
    for d in itertools.product((-1, 0, 1), repeat=3):
        i, j = tuple(x % 3 for x in d), tuple(-x % 3 for x in d)
        assert areas[i] == areas[j]
        if d == (0, 0, 0):
            continue
        r = np.array(d, dtype=np.float64) @ vl
        want = areas[i] / float(np.sqrt(r @ r)) if areas[i] else 0.0
        assert np.float64(want).tobytes() == alpha[i].tobytes(), (name, d)
    dirs, a = adjacency.active_directions(vl)
    assert dirs.dtype == np.int32 and a.dtype == np.float64 and len(dirs) == len(a) <= 7
    listed = [tuple(d) for d in dirs.tolist()]
    assert listed == sorted(listed) and all(d > tuple(-x for x in d) for d in listed)
    assert np.array_equal(a, [areas[tuple(x % 3 for x in d)] for d in listed]) and np.all(a > 0)
    if name.endswith('tric'):
        assert len(listed) > 3
    else:
        assert listed == ORTHO_DIRS
        assert np.allclose(a, [np.prod(np.diag(vl)) / np.diag(vl)[ax] for ax in (2, 1, 0)], rtol=1e-12)
    # the cell's volume from its facets: sum over all 26 of area * |r| / 6 (pyramids from the centre)
    vol = sum(areas[tuple(x % 3 for x in d)] * np.linalg.norm(np.array(d, float) @ vl) / 6.0
              for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0))
    assert abs(vol - abs(np.linalg.det(vl))) <= 1e-9 * abs(np.linalg.det(vl))


def test_a_skewed_lattice_raises_as_voronoi_weights_does():
    vl = np.array([[1.0, 0.0, 0.0], [2.6, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError):
        weight.voronoi_weights(vl)
    with pytest.raises(ValueError):
        weight.voronoi_areas(vl)
    with pytest.raises(ValueError):
        adjacency.active_directions(vl)
    with pytest.raises(ValueError):
        weight.voronoi_areas(np.zeros((3, 3)))


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_facet_id_and_follow_the_tie():
    shape = (4, 5, 6)
    lab = np.zeros(shape, np.int32)
    lab[:, :, 3:] = 1                                                 # split along z: the facets z = 2|3 and z = 5|0
    rho = np.full(shape, 1.0)
    rho[:, :, 2] = 2.0
    rho[:, :, 3] = 2.0                                                # every facet of the plane z = 2|3 has s = 2: a tie of 20
    rho[0, 0, 0] = 3.0                                                # three distinct values; (0,0,0) borders (0,0,5) where rho = 1
    assert len(np.unique(rho)) == 3
    pairs, facets, saddle, sfacet = reference_adjacency(rho, lab, 2, ORTHO_DIRS)
    assert pairs.tolist() == [[0, 1]] and facets.tolist() == [[2 * 4 * 5, 0, 0]] and saddle[0] == 2.0
    assert sfacet[0] == np.ravel_multi_index((0, 0, 2), shape) * 8 + 0
    rho2 = rho.copy()
    rho2[:2, :, 2] = 1.5                                              # the tie now starts at x = 2
    assert reference_adjacency(rho2, lab, 2, ORTHO_DIRS)[3][0] == np.ravel_multi_index((2, 0, 2), shape) * 8 + 0
    rho3 = np.full(shape, 1.0)
    rho3[3, 4, 5] = rho3[3, 4, 0] = 2.0                               # one facet through the wrap alone reaches 2
    got = reference_adjacency(rho3, lab, 2, ORTHO_DIRS)
    assert got[2][0] == 2.0 and got[3][0] == np.ravel_multi_index((3, 4, 5), shape) * 8 + 0
    # all equal: the very first counting facet
    assert reference_adjacency(np.ones(shape), lab, 2, ORTHO_DIRS)[3][0] == np.ravel_multi_index((0, 0, 2), shape) * 8


# ---- the key order --------------------------------------------------------------------------------------------------------------------
def test_key_order():
    x = np.array([-np.inf, -3.5, -1e-300, -0.0, 0.0, 1e-300, 2.0, np.inf])
    k = key(x)
    assert np.all(k[:-1] < k[1:]), '-0.0 < +0.0, negative values order as <'
    assert np.array_equal(unkey(k).view(np.uint64), x.view(np.uint64))
    assert np.array_equal(adjacency.key(x), k)
    nan = np.array([np.nan, -np.nan])
    assert key(np.abs(nan))[0] > k[-1] and key(-np.abs(nan))[0] < k[0]
    # a surface whose two sides are -0.0 and +0.0: the smaller is -0.0; among facets with s = -0.0 and s = -1 the saddle is -0.0
    shape = (3, 3, 4)
    lab = np.zeros(shape, np.int32)
    lab[:, :, 2:] = 1
    rho = np.full(shape, -1.0)
    rho[1, 1, 1], rho[1, 1, 2] = 0.0, -0.0
    pairs, facets, saddle, sfacet = reference_adjacency(rho, lab, 2, ORTHO_DIRS)
    assert saddle.view(np.uint64)[0] == np.float64(-0.0).view(np.uint64)
    assert sfacet[0] == np.ravel_multi_index((1, 1, 1), shape) * 8
    # negative values (a spin density): s is the more negative side, the saddle the least negative s
    rho = -np.arange(1.0, 37.0).reshape(shape)
    _, _, saddle, sfacet = reference_adjacency(rho, lab, 2, ORTHO_DIRS)
    assert saddle[0] == max(np.minimum(rho[:, :, 1], rho[:, :, 2]).max(), np.minimum(rho[:, :, 3], rho[:, :, 0]).max())


# ---- thin axes ------------------------------------------------------------------------------------------------------------------------
def test_axes_of_length_one_and_two():
    rng = np.random.default_rng(3)
    shape = (1, 4, 5)
    lab = rng.integers(0, 3, shape).astype(np.int32)
    rho = rng.random(shape)
    with_x = reference_adjacency(rho, lab, 3, ORTHO_DIRS)
    assert not with_x[1][:, 2].any(), 'an axis of length 1 gives no facets along it'
    same([with_x[0], with_x[1][:, :2], with_x[2], with_x[3]], reference_adjacency(rho, lab, 3, ORTHO_DIRS[:2]))
    shape = (2, 1, 1)
    lab = np.array([0, 1], np.int32).reshape(shape)
    rho = np.array([0.25, 0.75]).reshape(shape)
    pairs, facets, saddle, sfacet = reference_adjacency(rho, lab, 2, ORTHO_DIRS)
    assert pairs.tolist() == [[0, 1]] and facets.tolist() == [[0, 0, 2]], 'two facets between the same two voxels, both count'
    assert saddle[0] == 0.25 and sfacet[0] == 0 * 8 + 2


# ---- persistence ----------------------------------------------------------------------------------------------------------------------
def test_persistence_of_a_double_well():
    """a 1-D profile along z laid out in (3, 3, 12): maxima 5 (label 0) and 3 (label 1), between them a pass of height 2
    on one side and, through the wrap, of height 1 on the other"""
    z = np.array([1.5, 3.0, 5.0, 3.0, 2.0, 2.5, 3.0, 2.0, 1.0, 0.5, 0.75, 1.0])
    shape = (3, 3, 12)
    rho = np.ascontiguousarray(np.broadcast_to(z, shape))
    lab = np.zeros(shape, np.int32)
    lab[:, :, 5:10] = 1                                               # label 1: z = 5 .. 9; the facets 4|5 (s = 2) and 9|10 (s = 0.5)
    pairs, facets, saddle, sfacet = reference_adjacency(rho, lab, 2, ORTHO_DIRS)
    assert pairs.tolist() == [[0, 1]] and saddle[0] == 2.0
    p = adjacency.persistence(pairs, saddle, np.array([5.0, 3.0]))
    assert p[0] == np.inf and p[1] == 3.0 - 2.0
    # a third, isolated label and two labels of equal height: neither is above the other
    assert adjacency.persistence(pairs, saddle, np.array([5.0, 3.0, 9.0])).tolist() == [np.inf, 1.0, np.inf]
    assert adjacency.persistence(pairs, saddle, np.array([3.0, 3.0])).tolist() == [np.inf, np.inf]
    # the highest saddle with a HIGHER neighbour counts, in key order
    pairs3 = np.array([[0, 1], [0, 2], [1, 2]], np.int32)
    got = adjacency.persistence(pairs3, np.array([0.5, 1.5, 2.5]), np.array([4.0, 3.0, 6.0]))
    assert got.tolist() == [4.0 - 1.5, 3.0 - 2.5, np.inf]

"""Tests of what k_edge_sweep_bits carries from one tile to the next.  A workgroup strides over the listed tiles; it keeps the edge
masks and the list offsets of up to four tiles (EB_BATCH) in LDS and takes their list space with one atomic when the batch is
full or its tiles are done.  tests/test_gpu_edge_sweep_bits.py guards the algebra on grids of a few dozen tiles, where every
workgroup sweeps exactly one; with min(tiles, 2048) workgroups and an eighth of the list per XCD a workgroup takes a second tile
only above 2 048 listed tiles and a fifth only above 8 192.  The shapes:

  128 x 192 x 192    2 304 tiles: with all of them listed 256 workgroups sweep two tiles and the rest one
  160 x 256 x 256    5 120 tiles: two or three per workgroup
  320 x 256 x 256   10 240 tiles: five per workgroup -- a full batch written out inside the loop, then a batch of one (the block
                    maps only: 21 M voxels)

Every case runs edge_find() under the default form and under CROSS_CHECK_VOXEL_SWEEP (the per-voxel kernels), compares `known`
byte for byte, the edge count and the sorted edge list (xb_edge_list), proves through sweep_stats() which form ran, and asserts
from the tile list's counter that more than 2 048 tiles were listed.  Every comparison is exact.

On uploaded labels without a table every edge is a candidate for the maximum exception (two more barriers per tile); after an
assignment the context keeps its brick bytes and the tiles take the short way.  Both run."""
import numpy as np
import pytest

from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform

SHAPES = {'128x192x192': (128, 192, 192), '160x256x256': (160, 256, 256), '320x256x256': (320, 256, 256)}
SMALL, LARGE = '128x192x192', '320x256x256'
CASES = [(n, k) for n in SHAPES if n != LARGE for k in ('random', 'blocks', 'slabs_x', 'slabs_y', 'slabs_z')] + [(LARGE, 'blocks')]
# label 2, 3, ... on [start, start + length) along the axis, 1 elsewhere.  The first face lies on a tile boundary (x: 3|4, tiles
# of 4; y: 7|8, tiles of 8; z: 63|64, tiles of 64).  A face lists the tiles of the bricks next to it only, so three slabs do not
# reach 2 048 listed tiles along every axis of both shapes; the table holds as many parallel slabs as it takes (at least three).
SLABS = {
    ('128x192x192', 0): [(4, 16), (44, 20), (84, 24)],
    ('128x192x192', 1): [(8, 16), (40, 16), (72, 16), (104, 16), (136, 16), (168, 16)],
    ('128x192x192', 2): [(64, 16), (100, 20), (140, 24)],
    ('160x256x256', 0): [(4, 16), (36, 20), (76, 16), (108, 20), (132, 12)],
    ('160x256x256', 1): [(8, 16), (40, 16), (72, 16), (104, 16), (136, 16), (168, 16), (200, 16), (232, 16)],
    ('160x256x256', 2): [(64, 16), (100, 20), (140, 24)],
}


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    c.close()


def matrices(shape):
    vl = np.divide(synth.CUBIC6, shape)
    return distance_matrix(vl), gradient_transform(vl)


def ramp(shape):
    """a density that grows with the C-order voxel index: with the periodic wrap its only 27-point maximum is the last voxel"""
    return np.arange(1, int(np.prod(shape)) + 1, dtype=np.float64).reshape(shape)


def labels_of(kind, name):
    shape = SHAPES[name]
    rng = np.random.default_rng(9)
    if kind == 'random':      # every tile listed, every row has edges
        return rng.integers(1, 5, shape).astype(np.int32)
    if kind == 'blocks':      # 16^3 blocks
        small = rng.integers(1, 5, tuple(s // 16 for s in shape)).astype(np.int32)
        return np.repeat(np.repeat(np.repeat(small, 16, 0), 16, 1), 16, 2)
    axis = {'slabs_x': 0, 'slabs_y': 1, 'slabs_z': 2}[kind]
    lab = np.ones(shape, np.int32)
    for k, (start, length) in enumerate(SLABS[name, axis]):
        idx = [slice(None)] * 3
        idx[axis] = slice(start, start + length)
        lab[tuple(idx)] = 2 + k
    return lab


def both_forms(ctx, lab):
    """edge_find() on `lab` under the bit form and under the per-voxel kernels -> (known, edge count, tiles listed), after
    comparing the two runs"""
    res = []
    for bits in (0, _lib.CROSS_CHECK_VOXEL_SWEEP):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
        s0 = ctx.sweep_stats()
        ctx.upload_labels(lab)
        n = ctx.edge_find()
        edges, tiles = ctx.edge_list()
        s1 = ctx.sweep_stats()
        res.append((n, ctx.download_known(), np.sort(edges), tiles, (s1[0] - s0[0], s1[1] - s0[1])))
    ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    (n0, known0, edges0, tiles0, took0), (n1, known1, edges1, tiles1, took1) = res
    assert took0 == (1, 0) and took1 == (0, 1), (took0, took1)
    print(f'edges {n0} / {n1}, tiles listed {tiles0}')
    assert tiles0 > 2048, 'no workgroup reaches a second tile'
    assert tiles0 > 8192 or lab.shape != SHAPES[LARGE], 'no workgroup fills a batch'
    assert n0 == n1 and edges0.size == n0 and edges1.size == n1
    assert np.array_equal(known0, known1)
    assert np.array_equal(edges0, edges1)
    assert np.array_equal(edges0, np.flatnonzero(known0.ravel() == -2))
    return known0, n0, tiles0


def brute_known(lab):
    """refinement.py:357-404 without vacuum, on the ramp density: the 26-neighbour inequality and its dilation"""
    e = np.zeros(lab.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if dx or dy or dz:
                    e |= np.roll(lab, (dx, dy, dz), (0, 1, 2)) != lab
    e[-1, -1, -1] = False   # the ramp's maximum is no edge (refinement.py:374-383)
    near = np.zeros(lab.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                near |= np.roll(e, (dx, dy, dz), (0, 1, 2))
    return np.where(e, -2, np.where(near, -1, 2)).astype(np.int8)


@pytest.mark.gpu
@pytest.mark.parametrize('name,kind', CASES)
def test_label_maps_on_the_ramp(ctx, name, kind):
    """uploaded labels, no table: every edge goes through the maximum exception.  The small shape against numpy as well."""
    shape = SHAPES[name]
    ctx.set_grid(shape, *matrices(shape))
    ctx.upload_density(ramp(shape))
    ctx.vacuum_assign(None, 1.0)
    lab = labels_of(kind, name)
    known, n, tiles = both_forms(ctx, lab)
    ntiles = lab.size // (4 * 8 * 64)
    if kind == 'random':
        assert tiles == ntiles and n > 0.99 * lab.size
    else:
        assert 0 < n < lab.size
    if name == SMALL:
        assert np.array_equal(known, brute_known(lab))


@pytest.mark.gpu
@pytest.mark.parametrize('name,kind', [c for c in CASES if c[1] in ('random', 'blocks')])
def test_label_maps_after_an_assignment(ctx, name, kind):
    """the same maps behind a neargrid assignment of the 8-atom density: the context keeps the table's brick bytes, only the
    tiles next to a brick with a maximum take the exception, the others finish behind three barriers"""
    shape = SHAPES[name]
    ctx.set_grid(shape, *matrices(shape))
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx.vacuum_assign(None, 1.0)
    ctx.assign('neargrid')
    both_forms(ctx, labels_of(kind, name))


@pytest.mark.gpu
def test_assign_and_refine_under_both_forms(ctx):
    """the real path on the small shape: assign('neargrid') and refine('changed', 2) -- labels, maxima and logs"""
    shape = SHAPES[SMALL]
    out = []
    for bits in (0, _lib.CROSS_CHECK_VOXEL_SWEEP):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, bits)
        ctx.set_grid(shape, *matrices(shape))
        ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
        ctx.vacuum_assign(None, 1.0)
        s0 = ctx.sweep_stats()
        n = ctx.assign('neargrid')
        maxima = ctx.maxima().copy()
        assigned = ctx.download_labels(np.int32)
        log = ctx.refine('changed', 2)
        s1 = ctx.sweep_stats()
        out.append((n, maxima, assigned, log, ctx.download_labels(np.int32), (s1[0] - s0[0], s1[1] - s0[1])))
    ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    a, b = out
    assert a[5][0] > 0 and a[5][1] == 0 and b[5][0] == 0 and b[5][1] == a[5][0], (a[5], b[5])
    assert a[0] == b[0] > 1 and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3] and len(a[3]) > 0 and a[3][0][0] > 0, (a[3], b[3])
    assert np.array_equal(a[4], b[4])

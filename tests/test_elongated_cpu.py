"""The constructions of tests/elongated_common.py against the CPU oracle alone, and the arithmetic that puts every shape of
tests/test_gpu_elongated.py on its side of a threshold, with the thresholds read back from the sources.  The GPU file trusts the
tile predictor at sizes no oracle is run for; this file is why it may.  If PW_SPAN, the 2^27 of the lean kernels, use24 or a tile
edge moves, the test that fails here names the shape that no longer crosses it."""
import itertools
import os
import re

import numpy as np
import pytest

import elongated_common as ec

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pybader_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def define(text, name):
    m = re.search(r'^#define\s+' + name + r'\s+(\d+)\b', text, re.M)
    assert m, f'{name} is no longer a plain #define'
    return int(m.group(1))


# ---- the thresholds and the shapes ---------------------------------------------------------------------------------------

def test_the_thresholds_are_what_the_shapes_were_chosen_for():
    assert f'constexpr int PW_SPAN = {ec.PW_SPAN};' in source('bader_kernels.h')
    stages = source('host_stages.h')
    assert ec.LEAN_VOXELS == 1 << 27
    assert 'light(g).use24 && c->N <= (1LL << 27);' in stages                      # lean_retrace_ok
    assert '(long long)g.wlen * g.nyz <= (1LL << 27) ? 4 : 3' in stages            # the lean walkers' offset form
    assert 'if (lean == 3) c->stat_wide_traces++;' in stages                       # ... which xb_trace_stats reports
    assert ec.U24 == 1 << 24
    assert 'l.use24 = ((long long)g.nx * g.ny < (1 << 24)) && g.nz < (1 << 24);' in source('bader_hip.hip')
    assert define(source('k_trace.h'), 'XB_MORTON_BITS') == ec.MORTON_BITS
    assert 'const bool linear = bits > XB_MORTON_BITS;' in stages and 'x &= 0x09249249u;' in source('k_trace.h')   # compact3: ten bits per axis
    masks, edges, ctx = source('k_masks.h'), source('k_edges.h'), source('host_context.h')
    assert (define(masks, 'GT_X'), define(masks, 'GT_Y'), define(masks, 'BRK')) == (ec.GT_X, ec.GT_Y, ec.BRK)
    assert (define(edges, 'ET_X'), define(edges, 'ET_Y')) == (ec.ET_X, ec.ET_Y)
    assert define(ctx, 'RELABEL_X') == ec.RELABEL_X
    # the relabel launches groups of RELABEL_X planes and its kernel strides by as many
    assert '(g.x1 - g.x0 + RELABEL_X - 1) / RELABEL_X)' in stages
    assert f'x = g.x0 + blockIdx.z * {ec.RELABEL_X} + (threadIdx.x >> 6)' in source('k_trace.h')
    # the limit: the smallest tile edge on the axis times the device's bound, before anything is allocated
    assert 'std::min(std::min(GT_X, ET_X), RELABEL_X) : std::min(std::min(GT_Y, ET_Y), BRK)' in ctx
    assert ctx.index('exceeds the launch limit') < ctx.index('HIPCHK(hipMalloc(&c->rho')


def test_axis_limits_arithmetic():
    """with the 65 536 a gfx950 device reports for gridDim.y and gridDim.z; the GPU file derives the shapes from what the context
    reads"""
    nx_max, ny_max = ec.axis_limits(65536, 65536)
    assert (nx_max, ny_max) == (262144, 524288)
    # the largest tile counts the accepted axes ask for, launch by launch
    assert -(-nx_max // ec.GT_X) <= 65536 and -(-nx_max // ec.ET_X) == 65536 and -(-nx_max // ec.RELABEL_X) == 65536
    assert -(-ny_max // ec.GT_Y) == 65536 and -(-ny_max // ec.ET_Y) == 65536 and -(-ny_max // ec.BRK) == 65536
    assert -(-(nx_max + 1) // ec.ET_X) > 65536 and -(-(ny_max + 1) // ec.BRK) > 65536
    lx, ly = ec.longest_shapes(nx_max, ny_max)
    assert lx == (262144, 16, 16) and ly == (16, 524288, 16)
    assert ec.forms(lx) == (True, True, True) and ec.forms(ly) == (True, True, True)
    # a bound of 65 535 (the inclusive reading of other runtimes): whole tiles below it
    assert ec.longest_shapes(*ec.axis_limits(65535, 65535)) == ((262128, 16, 16), (16, 524272, 16))


def test_the_shapes_straddle_the_thresholds():
    shapes = list(ec.THRESHOLD_SHAPES)
    assert all(s % t == 0 and s >= 16 for shape in shapes + [ec.SEAM_TILE_SHAPE] for s, t in zip(shape, ec.TILE))
    for shape, want in ec.THRESHOLD_SHAPES.items():
        assert ec.forms(shape) == want, shape
    z_long, above, top24, off24 = shapes
    # 2^27 voxels exactly, non-cubic: the last record's byte offset is 2^32 - 32; window origins on z up to nz - PW_SPAN
    assert ec.n_voxels(z_long) == ec.LEAN_VOXELS and (ec.n_voxels(z_long) - 1) * 32 == 2 ** 32 - 32
    assert z_long[2] - ec.PW_SPAN == 523776
    # just above: one 16-plane step of a 512 x 512 cross-section
    assert ec.n_voxels(above) == ec.LEAN_VOXELS + (1 << 22) and above[2] > ec.PW_SPAN
    # the top of the 24-bit operand: x * ny + y reaches 16 711 679 < 2^24, one row of tiles below nx * ny == 2^24
    assert (top24[0] - 1) * top24[1] + top24[1] - 1 == 16711679 < ec.U24 and top24[0] * (top24[1] + ec.TILE[1]) == ec.U24
    assert off24[0] * off24[1] == ec.U24 and not ec.use24(off24)
    # pw_lin: a window-relative (511, 511) on a grid with windows on x (nx >= PW_SPAN) stays below 2^24 for every ny that keeps use24
    ny_top = (ec.U24 - 1) // ec.PW_SPAN
    assert ec.PW_SPAN * ny_top < ec.U24 and (ec.PW_SPAN - 1) * ny_top + ec.PW_SPAN - 1 < ec.U24
    assert (ec.PW_SPAN - 1) * top24[1] + ec.PW_SPAN - 1 < ec.U24
    # nz >= 2^24 is out of reach below the int32 limit with 16-voxel axes: 16 * 16 * 2^24 == 2^32
    assert 16 * 16 * ec.U24 > 2 ** 31 - 1
    assert max(ec.n_voxels(s) for s in shapes) == 1 << 28
    # the walk list: 1024 bricks on an axis are the last a Morton code holds; every longer axis here takes the linear order
    at, above_z, above_x = ec.MORTON_SHAPES
    assert at[2] // ec.BRK == 1 << ec.MORTON_BITS and not ec.walk_list_linear(at)
    assert above_z[2] // ec.BRK == (1 << ec.MORTON_BITS) + 1 and ec.walk_list_linear(above_z)
    assert above_x[0] // ec.BRK == (1 << ec.MORTON_BITS) + 2 and ec.walk_list_linear(above_x)
    assert all(s % t == 0 for shape in ec.MORTON_SHAPES for s, t in zip(shape, ec.TILE)) and all(ec.forms(s) == (True, True, True) for s in ec.MORTON_SHAPES)
    assert [ec.walk_list_linear(s) for s in shapes] == [True, False, False, False]
    assert all(ec.walk_list_linear(s) for s in ec.longest_shapes(*ec.axis_limits(65536, 65536)))
    # the seams: lengths below, at and above one window, between one and two, and above two
    assert ec.SEAM_LENGTHS == (ec.PW_SPAN - 8, ec.PW_SPAN, ec.PW_SPAN + 8, 640) and (0, 2 * ec.PW_SPAN + 8) in ec.SEAM_CASES
    assert len(ec.SEAM_CASES) == 13 and all(ec.forms(tuple(L if a == k else 16 for k in range(3))) == (True, True, True) for a, L in ec.SEAM_CASES)
    assert ec.SEAM_TILE_SHAPE[0] > ec.PW_SPAN and ec.SEAM_TILE_SHAPE[1] > ec.PW_SPAN and ec.forms(ec.SEAM_TILE_SHAPE) == (True, True, True)


# ---- the tile density ------------------------------------------------------------------------------------------------------

def test_tile_density_is_what_the_module_states():
    rho = ec.tile_density()
    assert rho.shape == ec.TILE and rho.dtype == np.float64 and rho.min() > ec.BACKGROUND
    x, y, z = 5, 11, 2
    want = ec.BACKGROUND
    for (fx, fy, fz), amp, sigma in ec.GAUSSIANS:
        for sx, sy, sz in itertools.product((-1, 0, 1), repeat=3):
            r2 = (x - (fx + sx) * 16) ** 2 + (y - (fy + sy) * 16) ** 2 + (z - (fz + sz) * 8) ** 2
            want += amp * np.exp(-r2 / (2 * sigma * sigma))
    assert abs(rho[x, y, z] - want) <= 1e-14 * want
    big = ec.tiled_density((32, 48, 16))
    assert np.array_equal(big[16:, 32:, 8:], rho) and big.flags.c_contiguous


def test_displacement_is_periodic_below_the_tile_and_leaves_the_brick():
    d = ec.displacement()            # (asserts periodicity over the 2 x 2 x 2 tiling and |d| < TILE itself)
    assert d.shape == ec.TILE + (3,)
    far = np.abs(d).reshape(-1, 3).max(0)
    print('max |d| per axis', far)
    assert np.all(far < np.array(ec.TILE))
    assert far[0] >= 9 and far[1] >= 9, 'walkers must leave their 8^3 brick on x and y'
    assert np.array_equal(ec.tile_maxima(), [ec.TILE_MAXIMUM])


TILINGS = [(3, 2, 2), (2, 3, 5), (4, 3, 2), (1, 4, 3), (5, 1, 2), (1, 1, 7)]   # no multiples of each other; one tile wide on x, on y, on both


@pytest.mark.parametrize('mult', TILINGS, ids=ec.ids)
def test_prediction_equals_the_oracle_and_is_a_fixed_point(mult):
    shape = tuple(m * t for m, t in zip(mult, ec.TILE))
    rho = ec.tiled_density(shape)
    F = ec.oracle_own_map(rho)
    assert np.array_equal(F, ec.predicted_maxima(shape, 0, shape[0]))
    half = shape[0] // 2
    assert np.array_equal(F[half - 3:half + 5], ec.predicted_maxima(shape, half - 3, half + 5)), 'a slab of planes off the tile seams'
    mx, lab = ec.oracle_labels(F)
    assert mx.shape[0] == ec.n_tiles(shape) and np.array_equal(ec.sort_rows(mx), ec.lifted_maxima(shape))
    for mode, want_log in ec.tile_logs(shape).items():
        v, log = ec.oracle_refine(rho, lab, mode)
        assert np.array_equal(v, lab), mode
        assert log == want_log, (mode, log, want_log)


@pytest.mark.parametrize('single', list(itertools.product((False, True), repeat=3)), ids=lambda s: ''.join('1' if b else 'n' for b in s))
def test_edges_per_tile_by_the_axes_one_tile_wide(single):
    shape = tuple(t if s else 3 * t for s, t in zip(single, ec.TILE))
    rho = ec.tiled_density(shape)
    _, lab = ec.oracle_labels(ec.oracle_own_map(rho))
    _, log = ec.oracle_refine(rho, lab, ('changed', 2))
    assert log == ec.tile_logs(shape)[('changed', 2)]
    assert (log[0][0] if log else 0) == ec.EDGES_PER_TILE[single] * ec.n_tiles(shape)


# ---- the long walk ---------------------------------------------------------------------------------------------------------

def test_long_walk_on_z_is_the_packed_walker_tests_case():
    """tests/test_gpu_packed_walker.py keeps its 16 x 16 x 640 case, built here: the values its docstring states"""
    rho, dm, tg = ec.long_walk(2, 640)
    z = np.arange(640, dtype=np.float64)
    up = (z - 30.0) % 640.0
    prof = np.where(up <= 600.0, up / 600.0, (640.0 - up) / 40.0)
    ridge = 1.0 + 0.02 * np.cos(2.0 * np.pi * np.arange(16.0) / 8.0)[None, :, None] + 0.001 * np.cos(2.0 * np.pi * np.arange(16.0) / 16.0)[:, None, None]
    assert np.array_equal(rho, (1.0 + 40.0 * prof)[None, None, :] * ridge)
    from pybader_amd.interface import distance_matrix, gradient_transform
    vl = np.divide(np.diag([1.6, 1.6, 64.0]), (16, 16, 640))
    assert np.array_equal(dm, distance_matrix(vl)) and np.array_equal(tg, gradient_transform(vl))


@pytest.mark.parametrize('axis,length', ec.SEAM_CASES, ids=lambda p: str(p))
def test_long_walk_maxima_and_path_lengths(axis, length):
    """two maxima, both at L - 10 on the ridges; the walker that starts on a ridge one above the minimum makes L - 41 steps up the
    long axis, through every window on the way; the one on the minimum goes down through the periodic face in 40"""
    import oracle
    rho, dm, tg = ec.long_walk(axis, length)
    shape = rho.shape
    assert shape[axis] == length and sorted(shape)[:2] == [16, 16]
    crest = [0, 0, 0]
    crest[axis] = length - 10
    other = list(crest)
    other[(axis + 2) % 3] = 8
    ridge_values = rho.max()
    assert rho[tuple(crest)] == ridge_values and rho[tuple(other)] == ridge_values
    for mx in (crest, other):      # strict local maxima: every one of the 26 neighbours is lower
        nb = [rho[tuple((np.array(mx) + o) % shape)] for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
        assert max(nb) < rho[tuple(mx)]
    start = ec.long_walk_start(axis, length)
    path = oracle.trajectory_path(rho, dm, tg, start)
    assert len(path) - 1 == length - 41 and path[-1] == np.ravel_multi_index(tuple(crest), shape)
    assert np.array_equal(np.unravel_index(path, shape)[axis], np.arange(31, length - 9)), 'one voxel up the long axis per step'
    at_min = list(np.unravel_index(start, shape))
    at_min[axis] = 30
    down = oracle.trajectory_path(rho, dm, tg, int(np.ravel_multi_index(tuple(at_min), shape)))
    assert len(down) - 1 == 40 and down[-1] == path[-1]
    assert np.array_equal(np.unravel_index(down, shape)[axis], (30 - np.arange(41)) % length), 'down through the face at 0'


def test_long_walk_map_has_two_basins_and_is_a_fixed_point():
    """one case in full (the GPU file runs the oracle on all thirteen): two basins, no brick of one label, log [(64 L, 0), (0, 0)]"""
    axis, length = 1, 520
    rho, _, _ = ec.long_walk(axis, length)
    mx, lab = ec.oracle_labels(ec.oracle_own_map(rho, 0.1))
    assert mx.shape == (2, 3) and np.all(mx[:, axis] == length - 10) and sorted(mx[:, (axis + 2) % 3]) == [0, 8]
    bricks = lab.reshape(tuple(k for s in rho.shape for k in (s // 8, 8))).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 512)
    assert np.all(bricks.min(1) != bricks.max(1)), 'every brick holds both labels'
    v, log = ec.oracle_refine(rho, lab, ('changed', 2), 0.1)
    assert np.array_equal(v, lab) and log == [(64 * length, 0), (0, 0)]

"""Shared by tests/test_elongated_cpu.py and tests/test_gpu_elongated.py: the constructions for grids that are long on one axis
(surface slabs, wires), where the kernel forms chosen from a grid's SHAPE meet -- the 512-voxel windows of the packed walker
(bader_kernels.h, PW_SPAN, pw_rebase), the 24-bit index products (use24), the 32-bit record offsets of the lean kernels (2^27
voxels) and the tile counts that become gridDim.y / gridDim.z (xb_set_grid's per-axis limits).

The tile density -- an expectation that needs no oracle at 2^28 voxels.  Three Gaussians inside a tile of TILE = 16 x 16 x 8 voxels
(their 27 periodic images summed, cubic voxels of edge 0.025), repeated: np.tile of ONE array, so the density is periodic bit
for bit.  A trajectory reads only the 27 neighbours of the voxel it stands on, so the displacement from a voxel to the maximum its
own trajectory ends on, d(v) = maximum(v) - v by nearest image, is periodic with the tile on every tiling.  displacement() takes d
from the oracle on the 2 x 2 x 2 tiling (where |d| < TILE per axis makes the nearest image unambiguous) and checks its
periodicity; predicted_maxima() then states the maximum of every voxel of ANY tiling: (v + d(v mod TILE)) mod shape.
tests/test_elongated_cpu.py pins that to the oracle on tilings that are no multiples of each other, one tile wide among them.

The long walk -- tests/test_gpu_packed_walker.py's 16 x 16 x 640 with the long axis and its length free: the density rises along
the long axis from its minimum at 30 to its crest at L - 10 and falls through the periodic face; two ridges across one short axis.

All lattices are diagonal with cubic voxels; every shape is a multiple of the tile (and so of the 8^3 bricks)."""
import numpy as np

TILE = (16, 16, 8)
VOXEL = 0.025
GAUSSIANS = (((0.30, 0.35, 0.40), 1.0, 3.6), ((0.70, 0.60, 0.55), 0.7, 3.2), ((0.45, 0.80, 0.20), 0.5, 4.4))   # fractional centre, amplitude, sigma (voxels)
BACKGROUND = 0.01
# One maximum per tile, at TILE_MAXIMUM: every basin is the tile's, shifted.  Edge voxels of the own-trajectory map per tile (a
# neighbour among the 26 carries another label), by which axes are ONE tile wide -- across such an axis a basin meets itself
# through the wrap and has no edge there (the oracle: tests/test_elongated_cpu.py)
TILE_MAXIMUM = (6, 7, 3)
EDGES_PER_TILE = {(False, False, False): 968, (False, False, True): 611, (False, True, False): 783, (False, True, True): 362,
                  (True, False, False): 780, (True, False, True): 359, (True, True, False): 512, (True, True, True): 0}

# the thresholds the shapes straddle, as the sources state them (tests/test_elongated_cpu.py reads them back)
PW_SPAN = 512                 # bader_kernels.h: voxels per axis of a packed walker's window
LEAN_VOXELS = 1 << 27         # host_stages.h: lean_retrace_ok (N) and the 32-bit offset form of the lean walkers (wlen * nyz)
U24 = 1 << 24                 # bader_hip.hip, light(): use24 = nx * ny < 2^24 && nz < 2^24
GT_X, GT_Y, ET_X, ET_Y, BRK, RELABEL_X = 8, 8, 4, 8, 8, 4   # tile edges along x and y of pass A, the edge sweep, the bricks, the relabel
MORTON_BITS = 10              # k_trace.h: bits per axis of the walk list's Morton codes -- 1024 bricks, 8192 voxels; beyond: linear order

# window seams: the long axis on x, y and z at lengths around one window, and two windows and a bit on x
SEAM_LENGTHS = (504, 512, 520, 640)
SEAM_CASES = [(axis, L) for axis in (0, 1, 2) for L in SEAM_LENGTHS] + [(0, 1032)]
SEAM_TILE_SHAPE = (528, 528, 16)    # the tile density with window origins that are non-zero in x and y at once

# the thresholds, crossed with the tile density: shape -> (packed walker, 32-bit offsets, lean retrace) that must run
THRESHOLD_SHAPES = {
    (16, 16, 524288): (True, True, True),      # N = 2^27: the last record's offset is 2^32 - 32; window origins up to 523 776 on z
    (512, 512, 528): (True, False, False),     # N = 2^27 + 2^22: just above lean_retrace_ok and the 32-bit offsets
    (4096, 4080, 16): (True, False, False),    # x * ny + y up to 16 711 679, the top of the 24-bit operand
    (4096, 4096, 16): (False, False, False),   # nx * ny == 2^24: use24 off, the generic walker
}


# the walk list's order: at the last axis length a Morton code holds, and the first beyond it on z and on x
MORTON_SHAPES = [(16, 16, 8192), (16, 16, 8200), (8208, 16, 16)]


def ids(shape):
    return 'x'.join(str(s) for s in shape)


def n_voxels(shape):
    return int(shape[0]) * int(shape[1]) * int(shape[2])


def n_tiles(shape):
    assert all(s % t == 0 for s, t in zip(shape, TILE)), shape
    return (shape[0] // TILE[0]) * (shape[1] // TILE[1]) * (shape[2] // TILE[2])


def matrices(shape, voxel=VOXEL):
    from pybader_amd.interface import distance_matrix, gradient_transform
    vl = np.eye(3) * voxel
    return distance_matrix(vl), gradient_transform(vl)


# ---- what the shape selects (restated from host_stages.h / bader_hip.hip; the CPU file checks the restatement's constants) -------

def use24(shape):
    return shape[0] * shape[1] < U24 and shape[2] < U24


def forms(shape):
    """(packed walker, 32-bit table offsets, lean retrace) on one GPU for a whole-brick grid of at least 16 voxels per axis"""
    packed = use24(shape)
    return packed, packed and n_voxels(shape) <= LEAN_VOXELS, packed and n_voxels(shape) <= LEAN_VOXELS


def walk_list_linear(shape):
    """the walk list is made in linear brick order: an axis of more bricks than a Morton code holds"""
    return max(-(-s // BRK) for s in shape) > 1 << MORTON_BITS


def axis_limits(max_grid_y, max_grid_z):
    """(longest nx, longest ny) xb_set_grid accepts: the smallest tile edge on the axis times the device's gridDim bound"""
    return min(GT_X, ET_X, RELABEL_X) * max_grid_z, min(GT_Y, ET_Y, BRK) * max_grid_y


def longest_shapes(nx_max, ny_max, cap=1 << 27):
    """the longest accepted x- and y-elongated grids of whole tiles with a 16 x 16 cross-section (at most `cap` voxels each)"""
    lx = min(nx_max, cap // 256) // TILE[0] * TILE[0]
    ly = min(ny_max, cap // 256) // TILE[1] * TILE[1]
    return (lx, 16, 16), (16, ly, 16)


# ---- the tile density and its predictor ----------------------------------------------------------------------------------

def tile_density(tile=TILE):
    ax = [np.arange(t, dtype=np.float64) for t in tile]
    rho = np.full(tile, BACKGROUND)
    for frac, amp, sigma in GAUSSIANS:
        g = []
        for k in range(3):      # separable: the sum over the 27 images is the product of three sums over 3 images
            c = frac[k] * tile[k]
            g.append(sum(np.exp(-((ax[k] - c - s * tile[k]) ** 2) / (2.0 * sigma * sigma)) for s in (-1, 0, 1)))
        rho = rho + amp * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    return np.ascontiguousarray(rho)


def tiled_density(shape, tile=TILE):
    assert all(s % t == 0 for s, t in zip(shape, tile)), (shape, tile)
    return np.ascontiguousarray(np.tile(tile_density(tile), tuple(s // t for s, t in zip(shape, tile))))


def oracle_own_map(rho, voxel=VOXEL):
    """linear index of the maximum every voxel's own trajectory ends on (the assignment's tie rule)"""
    from rough_common import own_map
    dm, tg = matrices(rho.shape, voxel)
    return own_map(rho, np.zeros(rho.shape, np.int32), dm, tg, main_ties=True)


def oracle_labels(F):
    """what xb_assign(neargrid) returns for the own-trajectory map F: (maxima [n, 3] in label order, labels int32)"""
    from rough_common import rank_labels
    lab, maxima = rank_labels(F)
    return np.array(np.unravel_index(maxima, F.shape), np.int64).T.reshape(-1, 3), np.ascontiguousarray(lab.astype(np.int32))


def oracle_refine(rho, labels, mode, voxel=VOXEL):
    import oracle
    dm, tg = matrices(rho.shape, voxel)
    v = np.ascontiguousarray(labels.astype(np.int32))
    log = []
    oracle.refine('neargrid', mode, rho, v, dm, tg, 1, log=log)
    return v, [(int(a), int(b)) for a, b in log]


_displacement = {}


def displacement(tile=TILE):
    """d[x, y, z] = maximum(v) - v (three ints) for the voxels of one tile, from the oracle on the 2 x 2 x 2 tiling; asserts that
    it is the same in all eight tiles and below the tile on every axis, which is what makes it the displacement on every tiling"""
    if tile not in _displacement:
        shape2 = tuple(2 * t for t in tile)
        F = oracle_own_map(tiled_density(shape2, tile))
        m = np.stack(np.unravel_index(F, shape2), -1).astype(np.int64)
        v = np.stack(np.meshgrid(*(np.arange(s) for s in shape2), indexing='ij'), -1)
        s = np.array(shape2)
        d = (m - v + s // 2) % s - s // 2          # nearest image on the doubled tile: [-tile, tile)
        assert np.all(np.abs(d) < np.array(tile)), 'a trajectory as long as the tile: the nearest image is ambiguous'
        d0 = d[:tile[0], :tile[1], :tile[2]]
        assert np.array_equal(d, np.tile(d0, (2, 2, 2, 1))), 'the displacement field is not periodic with the tile'
        d0 = np.ascontiguousarray(d0.astype(np.int32))
        d0.setflags(write=False)
        _displacement[tile] = d0
    return _displacement[tile]


def predicted_maxima(shape, xa, xb, tile=TILE):
    """linear index (int32 [xb - xa, ny, nz]) of the maximum of every voxel of the planes xa .. xb of the tiling `shape`:
    (v + d(v mod tile)) mod shape.  Each wrapped coordinate depends on its own axis in full and on the other two through the
    tile only, so it is formed on an array one tile wide on those and broadcast."""
    nx, ny, nz = shape
    t0, t1, t2 = tile
    assert nx % t0 == 0 and ny % t1 == 0 and nz % t2 == 0 and n_voxels(shape) < 2 ** 31
    d = displacement(tile)
    xs, ys, zs = np.arange(xa, xb, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nz, dtype=np.int64)
    dx = d[xs % t0][..., 0]                          # [p, t1, t2]
    mx = (xs[:, None, None] + dx) % nx
    dy = d[xs % t0][:, ys % t1][..., 1]              # [p, ny, t2]
    my = (ys[None, :, None] + dy) % ny
    dz = d[xs % t0][:, :, zs % t2][..., 2]           # [p, t1, nz]
    mz = (zs[None, None, :] + dz) % nz
    p = xb - xa
    a = (mx * (ny * nz)).astype(np.int32).reshape(p, 1, t1, 1, t2)
    b = (my * nz).astype(np.int32).reshape(p, ny // t1, t1, 1, t2)
    c = mz.astype(np.int32).reshape(p, 1, t1, nz // t2, t2)
    return (a + b + c).reshape(p, ny, nz)


def tile_maxima(tile=TILE):
    """the maxima inside one tile, rows sorted"""
    d = displacement(tile)
    v = np.stack(np.meshgrid(*(np.arange(t) for t in tile), indexing='ij'), -1)
    return sort_rows(np.unique(((v + d) % np.array(tile)).reshape(-1, 3), axis=0))


def lifted_maxima(shape, tile=TILE):
    """the maxima of the tiling: every tile maximum in every tile, rows sorted"""
    tm = tile_maxima(tile)
    origins = np.stack(np.meshgrid(*(np.arange(0, s, t) for s, t in zip(shape, tile)), indexing='ij'), -1).reshape(-1, 1, 3)
    return sort_rows((origins + tm[None]).reshape(-1, 3))


def sort_rows(a):
    a = np.asarray(a, np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def tile_logs(shape):
    """the refinement logs of the tiling's own-trajectory map, a fixed point: ('changed', 2) and ('all', -1)"""
    e = EDGES_PER_TILE[tuple(s == t for s, t in zip(shape, TILE))] * n_tiles(shape)
    return {('changed', 2): [(e, 0), (0, 0)], ('all', -1): [(e, 0), (e, 0)]} if e else {('changed', 2): [], ('all', -1): []}


# ---- the long walk ---------------------------------------------------------------------------------------------------------

def long_walk(axis, length):
    """(rho, dist_mat, T_grad) of a 16 x 16 x L grid with the long axis on `axis`: the density rises along it from its minimum at
    30 to its crest at L - 10 over L - 40 voxels and falls from there through the periodic face back to 30; a modulation across
    the short axis before it (cyclically: y for a long z) puts two ridges (0 and 8) and the surfaces between them (4 and 12) inside
    every brick, so no brick is certified.  Walkers from 31 travel L - 40 voxels up, through every window of the axis; walkers from
    below 30 travel down through the face at 0 into the window at the grid's other end."""
    shape = [16, 16, 16]
    shape[axis] = length
    ridge_axis, other = (axis + 2) % 3, (axis + 1) % 3
    t = np.arange(length, dtype=np.float64)
    rise = float(length - 40)
    up = (t - 30.0) % float(length)
    prof = np.where(up <= rise, up / rise, (float(length) - up) / 40.0)
    s = np.arange(16, dtype=np.float64)

    def along(a, values):
        sh = [1, 1, 1]
        sh[a] = values.shape[0]
        return values.reshape(sh)
    ridge = 1.0 + along(ridge_axis, 0.02 * np.cos(2.0 * np.pi * s / 8.0)) + along(other, 0.001 * np.cos(2.0 * np.pi * s / 16.0))
    rho = np.ascontiguousarray(along(axis, 1.0 + 40.0 * prof) * ridge)
    assert rho.shape == tuple(shape)
    dm, tg = matrices(tuple(shape), 0.1)
    return rho, dm, tg


def long_walk_start(axis, length):
    """the voxel with the longest trajectory: on a ridge, one above the minimum"""
    v = [0, 0, 0]
    v[axis] = 31
    shape = [16, 16, 16]
    shape[axis] = length
    return int(np.ravel_multi_index(tuple(v), tuple(shape)))

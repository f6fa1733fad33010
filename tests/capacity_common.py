"""Shared by tests/test_capacity_cpu.py and tests/test_gpu_capacity.py: two synthetic densities whose number of maxima is exact
by construction, so a grid's shape alone decides on which side of a fixed capacity of the assignment pipeline a case lands
(k_fused.h: XB_BOXES_MAX, XB_SORT_MAX, XB_REGIONS_MAX, the 1024 block sums per round of k_rank_blocks; host_context.h: max_cap).

Density A -- one maximum per 8^3 brick, every basin is its brick, for ongrid and for neargrid's own-trajectory map alike:
    rho[x, y, z] = 2 + F8[x % 8] + 1.25 * F8[y % 8] + 1.5 * F8[z % 8]
F8 rises to its one maximum at 3 and falls to the brick's faces, so the density is separable, every brick repeats the same
512 values, the maxima are the voxels (8i + 3, 8j + 3, 8k + 3), the label of a voxel is the C-order index of its brick (basins are
numbered by their first voxel, a brick's corner) and maxima() lists those voxels in the same order.

Density B -- a maximum on every voxel whose three indices are even, N / 8 of them:
    rho = e(x) e(y) e(z) + 0.5 * default_rng(1).random(shape),   e(t) = 1 for even t, else 0
An all-even voxel holds at least 1, each of its 26 neighbours has an odd index and so less than 0.5; no other voxel is a maximum
since one of its neighbours is all-even.  No closed-form map: the basins follow the noise, each method needs its oracle.

All axes are multiples of 8 and the lattice is diag(shape) / 40: cubic voxels of edge 1 / 40, which the closed form of A relies on
(the 26 neighbour distances are those of a cube)."""
import numpy as np

F8 = np.array([0.1, 0.4, 0.8, 1.0, 0.7, 0.5, 0.3, 0.2])

# the capacities the cases straddle, as the kernels define them (tests/test_capacity_cpu.py reads them back from the sources)
XB_BOXES_MAX = 1024          # k_fused.h: regions whose rank / first brick sits in an LDS table
XB_SORT_MAX = 2048           # k_fused.h: maxima k_number_maxima sorts in LDS
XB_REGIONS_MAX = 65535       # k_fused.h: trapping regions seeded by bricks
RANK_BLOCKS_PER_ROUND = 1024   # k_fused.h, k_rank_blocks: block sums scanned per round, then a carry
MAX_CAP = 1 << 22            # host_context.h: max_cap = min(N, 2^22) entries of the maxima table

# shapes by the count they are chosen for (bricks of 8^3 voxels == maxima of density A)
REGION_SHAPES = {1008: (64, 72, 112), 1024: (64, 64, 128), 1056: (64, 96, 88)}     # nz >= 80: the full-size brick kernels
REGION_SHAPE_SMALL = (64, 128, 64)                                                    # 1024 bricks, nz < 80: the small_grid form
SORT_SHAPES = {2040: (136, 64, 120), 2048: (128, 64, 128), 2057: (136, 88, 88)}
SEED_SHAPES = {64512: (256, 504, 256), 65536: (256, 512, 256), 67584: (264, 512, 256)}
CARRY_SHAPE = SEED_SHAPES[67584]        # n_blocks = 1056: one full round of k_rank_blocks, then 32 sums behind the carry
EXACT_ROUND_SHAPE = SEED_SHAPES[65536]  # n_blocks = 1024: the round that fits exactly, no carry
B_FITS_SHAPE = SEED_SHAPES[65536]       # density B: 2^22 maxima == max_cap
B_OVER_SHAPE = SEED_SHAPES[67584]       # density B: 4 325 376 maxima
B_NEARGRID_SHAPE = (64, 64, 128)        # density B under neargrid: ovf_cap == N here, the slow path's list cannot overflow


def lattice(shape):
    return np.diag(np.asarray(shape, np.float64)) / 40.0


def matrices(shape):
    from pybader_amd.interface import distance_matrix, gradient_transform
    vl = np.divide(lattice(shape), shape)
    return distance_matrix(vl), gradient_transform(vl)


def n_voxels(shape):
    return int(shape[0]) * int(shape[1]) * int(shape[2])


def n_bricks(shape):
    assert all(s % 8 == 0 for s in shape), shape
    return (shape[0] // 8) * (shape[1] // 8) * (shape[2] // 8)


def n_rank_blocks(shape):
    """number_maxima_big (host_assign.h): one bit per voxel, 32 per word, 1024 words per workgroup of k_rank_scan"""
    n_words = (n_voxels(shape) + 31) // 32
    return (n_words + 1023) // 1024


def density_a(shape):
    fx, fy, fz = (F8[np.arange(s) % 8] for s in shape)
    return np.ascontiguousarray(2.0 + fx[:, None, None] + 1.25 * fy[None, :, None] + 1.5 * fz[None, None, :])


def labels_a(shape):
    """the closed-form map of density A: the C-order index of the voxel's brick"""
    nb1, nb2 = shape[1] // 8, shape[2] // 8
    bx, by, bz = (np.arange(s, dtype=np.int32) // 8 for s in shape)
    return np.ascontiguousarray((bx[:, None, None] * nb1 + by[None, :, None]) * nb2 + bz[None, None, :])


def maxima_a(shape):
    """the maxima of density A in label order: (8i + 3, 8j + 3, 8k + 3), bricks in C order"""
    g = np.meshgrid(*(np.arange(s // 8, dtype=np.int64) * 8 + 3 for s in shape), indexing='ij')
    return np.stack(g, -1).reshape(-1, 3)


def edges_a(shape):
    """edge voxels of A's map (a neighbour among the 26 carries another label): the 8^3 - 6^3 voxels of every brick's shell"""
    return (512 - 216) * n_bricks(shape)


def density_b(shape):
    ex, ey, ez = ((np.arange(s) % 2 == 0).astype(np.float64) for s in shape)
    noise = np.random.default_rng(1).random(shape)
    return np.ascontiguousarray(ex[:, None, None] * ey[None, :, None] * ez[None, None, :] + 0.5 * noise)


def maxima_b_sorted(shape):
    """the all-even voxels, rows in lexicographic order (the ORDER of maxima() follows the basins' first voxels: compare as sets)"""
    g = np.meshgrid(*(np.arange(0, s, 2, dtype=np.int64) for s in shape), indexing='ij')
    return np.stack(g, -1).reshape(-1, 3)


def sort_rows(a):
    a = np.asarray(a, np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def oracle_ongrid(rho, shape):
    import oracle
    dm, tg = matrices(shape)
    bmax, lab = oracle.bader_calc('ongrid', rho, np.zeros(shape, np.int32), dm, tg, 1)
    return np.asarray(bmax, np.int64), np.ascontiguousarray(lab.astype(np.int32))


def oracle_neargrid(rho, shape):
    """what xb_assign(neargrid) returns: the own-trajectory map, basins numbered by their first voxel"""
    from rough_common import own_map, rank_labels
    dm, tg = matrices(shape)
    lab, maxima = rank_labels(own_map(rho, np.zeros(shape, np.int32), dm, tg, main_ties=True))
    return np.array(np.unravel_index(maxima, shape), np.int64).T.reshape(-1, 3), np.ascontiguousarray(lab.astype(np.int32))


def oracle_refine(rho, labels, shape, mode):
    import oracle
    dm, tg = matrices(shape)
    v = np.ascontiguousarray(labels.astype(np.int32))
    log = []
    oracle.refine('neargrid', mode, rho, v, dm, tg, 1, log=log)
    return v, [(int(a), int(b)) for a, b in log]

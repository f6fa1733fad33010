"""Critical points of the density and the bond graph they define -- the core of a QTAIM analysis, no counterpart in the
reference.  Nuclear, bond, ring and cage points are the maxima, 2-saddles, 1-saddles and minima of rho; the bond graph says
which basins a bond path joins and what rho is at the bond point.  adjacency.adjacency lists every pair of basins that touch;
this tells a bonded pair from one that merely shares a few facets.

The points are the piecewise-linear critical points of rho on the Freudenthal triangulation of the periodic voxel lattice
(14 neighbours per voxel, ties broken by voxel index): integers throughout, and minima - rings + bonds - maxima == 0 on any
field once every axis has four voxels.  The pass runs in libbader_hip.so (xb_critical_points / xb_critical_bonds,
csrc/k_critical.h); the definition is in include/bader_hip.h and DESIGN.md section 17, and tests/test_critical_cpu.py restates
it in numpy.

    critical_points(density, vacuum_tol=None, flood=False)    a CriticalPoints
    bond_graph(density, volumes, n)                           a BondGraph
    positions(voxels, shape, lattice)                         Cartesian positions of voxels"""
import numpy as np

from . import _lib
from .utils import ensure_density, ensure_labels

NUCLEAR, BOND, RING, CAGE = 1, 2, 4, 8   # the bits of CriticalPoints.kinds
OFFSETS = np.array([(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1),
                    (0, 0, -1), (0, -1, 0), (0, -1, -1), (-1, 0, 0), (-1, 0, -1), (-1, -1, 0), (-1, -1, -1)], dtype=np.int64)


def positions(voxels, shape, lattice):
    """Cartesian positions f64[P, 3] of `voxels` (int[P, 3], or linear C-order indices int[P]) on a grid of `shape` in the cell
    `lattice` (a row per axis), as utils.surface_dist forms them: lat[0] p0 / nx, += lat[1] p1 / ny, += lat[2] p2 / nz"""
    shape = tuple(int(s) for s in shape)
    v = np.asarray(voxels, dtype=np.int64)
    if v.ndim == 1:
        v = np.stack(np.unravel_index(v, shape), axis=1).astype(np.int64).reshape(-1, 3)
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    p = v.astype(np.float64)
    pos = np.empty((v.shape[0], 3), np.float64)
    for j in range(3):
        c = lat[0, j] * p[:, 0] / np.float64(shape[0])
        c = c + lat[1, j] * p[:, 1] / np.float64(shape[1])
        c = c + lat[2, j] * p[:, 2] / np.float64(shape[2])
        pos[:, j] = c
    return pos


class CriticalPoints:
    """The non-regular voxels of a density, ascending in their linear index:

    shape          the grid
    counts         int64[6]: maxima, bond voxels, sum of bond, ring voxels, sum of ring, minima (_lib.XB_CRITICAL_*)
    lin            int64[P]     linear C-order index
    voxels         int64[P, 3]
    masks          uint16[P]    the lower mask L: bit k set iff the neighbour at OFFSETS[k] lies below the voxel
    ring, bond     uint8[P]     multiplicity as a 1-saddle / 2-saddle
    kinds          uint8[P]     NUCLEAR | BOND | RING | CAGE bits (a voxel on noise may be BOND and RING at once)"""

    def __init__(self, shape, counts, lin, masks, ring, bond):
        self.shape = tuple(int(s) for s in shape)
        self.counts, self.lin, self.masks, self.ring, self.bond = counts, lin, masks, ring, bond
        self.voxels = np.stack(np.unravel_index(lin, self.shape), axis=1).astype(np.int64).reshape(-1, 3)
        self.kinds = (np.where(masks == _lib.XB_CRITICAL_FULL, NUCLEAR, 0) | np.where(bond > 0, BOND, 0) |
                      np.where(ring > 0, RING, 0) | np.where(masks == 0, CAGE, 0)).astype(np.uint8)

    def __len__(self):
        return self.lin.shape[0]

    @property
    def euler(self):
        """minima - sum of ring + sum of bond - maxima: 0 on a grid with every axis >= 4 (without a vacuum tolerance)"""
        c = self.counts
        return int(c[_lib.XB_CRITICAL_MINIMA] - c[_lib.XB_CRITICAL_RING_SUM] + c[_lib.XB_CRITICAL_BOND_SUM] - c[_lib.XB_CRITICAL_MAXIMA])


class BondGraph:
    """The pairs of basins a bond path joins, ascending in (a, b) with a < b:

    pairs          int32[P, 2]
    saddles        int64[P]     bond voxels between the two (one per periodic image the path goes through, more on noise)
    rho_b          f64[P]       the density at the highest of them
    voxel          int64[P]     its linear index (the smallest among equals);  voxels int64[P, 3]
    same_basin     bond voxels whose paths all end in one basin"""

    def __init__(self, shape, n, pairs, saddles, rho_b, voxel, same_basin):
        self.shape, self.n = tuple(int(s) for s in shape), int(n)
        self.pairs, self.saddles, self.rho_b, self.voxel, self.same_basin = pairs, saddles, rho_b, voxel, int(same_basin)
        self.voxels = np.stack(np.unravel_index(voxel, self.shape), axis=1).astype(np.int64).reshape(-1, 3)

    def __len__(self):
        return self.pairs.shape[0]

    def neighbours(self, a):
        """the basins bonded to basin `a`"""
        p = self.pairs
        return np.concatenate([p[p[:, 0] == a, 1], p[p[:, 1] == a, 0]])


def _resident(density):
    ctx = _lib.default_context()
    shape = tuple(int(s) for s in density.shape)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    return ctx, shape


def critical_points(density, vacuum_tol=None, flood=False):
    """The critical points of `density` (host array, or a float32 / float64 device array).

    vacuum_tol   None, or the density at or below which a voxel is neither counted nor listed
    flood        count the components of the masks by flood fill instead of the table: the second implementation

    -> CriticalPoints; inside utils.resident() nothing is uploaded again."""
    ctx, shape = _resident(density)
    return CriticalPoints(shape, *ctx.critical_points(vacuum_tol, flood))


def bond_graph(density, volumes, n, vacuum_tol=None):
    """The bond graph of the labels 0 .. n - 1 of `volumes` (host or device array) on `density`, the field they were made
    from: the basins that the bond points of critical_points(density, vacuum_tol) join.  Labels < 0 and >= n join nothing.
    -> BondGraph"""
    ctx, shape = _resident(density)
    if tuple(int(s) for s in volumes.shape) != shape:
        raise ValueError(f'bond_graph: the label map has shape {tuple(volumes.shape)}, the density {shape}')
    ensure_labels(ctx, volumes)
    if int(n) < 1:
        return BondGraph(shape, n, np.zeros((0, 2), np.int32), np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64), 0)
    ctx.critical_points(vacuum_tol, False)
    return BondGraph(shape, n, *ctx.critical_bonds(n))

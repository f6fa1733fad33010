"""Merge Bader volumes whose persistence lies below a threshold: the filter of spurious maxima that the saddles of
pybader_amd.adjacency are for -- no counterpart in the reference.  A noisy density has a maximum in every ripple of its vacuum;
a spurious one is separated from a higher neighbour by a saddle barely below its own value.  The result is a simplified label
map and a shorter list of maxima, on which charge sums, atom assignment, moments, weights and bond surfaces run unchanged.

The rounds run in libbader_hip.so (xb_merge_basins, csrc/k_merge.h); the definition is in include/bader_hip.h and DESIGN.md
section 15, and tests/test_merge_cpu.py restates it in numpy.  Every number is exact: saddles are maxima of existing doubles,
the persistence is one float64 subtraction, ties go to the smallest label.

A volume b is ABOVE a when its maximum is higher in key order, or has the same bits and b < a.  adjacency.persistence puts two
maxima of the same bits above neither; here one is above the other, so that a plateau split into two maxima can merge and the
parent pointers form a forest.  The merge is round-synchronous and looks at direct neighbours only: in a round every volume
sees its highest saddle towards a volume above it, merges into that one when its maximum minus the saddle is < tol, and the
next round starts from the merged partition.  It is not the persistence simplification of a merge tree, which cancels pairs
in ascending persistence one at a time.

    merge_basins(density, volumes, lattice, maxima_voxels, tol, max_rounds=64)   a Merge"""
import numpy as np

from . import _lib
from .adjacency import active_directions
from .utils import ensure_density, ensure_labels, volume_assign


class Merge:
    """What became of the labels 0 .. n - 1:

    root               int32[n]  the label each one ended up in (its own: it survives)
    merge_round        int32[n]  the round, from 0, in which it merged; -1 for a survivor
    merge_persistence  f64[n]    its maximum minus its highest saddle towards a volume above it, in the round it merged; for a
                                 survivor in the last round run (+inf without such a neighbour)
    rounds, converged  the rounds run, and whether the last one merged nothing (False: max_rounds stopped it)
    survivors          int64[S]  the surviving labels, ascending
    swap               int64[n]  label -> index of its root in `survivors`: the new label"""

    def __init__(self, root, merge_round, merge_persistence, rounds, converged):
        self.root, self.merge_round, self.merge_persistence = root, merge_round, merge_persistence
        self.rounds, self.converged = int(rounds), bool(converged)
        self.survivors = np.flatnonzero(merge_round < 0).astype(np.int64)
        self.swap = np.searchsorted(self.survivors, root).astype(np.int64)

    def __len__(self):
        return self.survivors.shape[0]

    def apply(self, volumes):
        """volumes[v] = swap[volumes[v]] in place (utils.volume_assign: host or device map; labels < 0 stay) -> volumes"""
        volume_assign(volumes, self.swap)
        return volumes


def merge_basins(density, volumes, lattice, maxima_voxels, tol, max_rounds=64):
    """Merge the labels 0 .. n - 1 of `volumes` below the persistence `tol`.

    density        the field the labels were made from: host array, or a float32 / float64 device array
    volumes        the label map, host or device array (not written); labels < 0 and >= n bound no surface
    lattice        the CELL's lattice, one row per axis
    maxima_voxels  int [n, 3]: the voxel of each label's maximum
    tol            >= 0, in the density's unit; +inf merges everything that has a neighbour above it

    -> Merge; inside utils.resident() nothing is uploaded again."""
    ctx = _lib.default_context()
    shape = tuple(int(s) for s in volumes.shape)
    lattice = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    dirs, _ = active_directions(lattice / np.array(shape, dtype=np.float64)[:, None])
    vox = np.asarray(maxima_voxels, dtype=np.int64).reshape(-1, 3)
    if vox.shape[0] < 1:
        return Merge(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64), 0, True)
    if np.any(vox < 0) or np.any(vox >= np.array(shape, dtype=np.int64)):
        raise ValueError('merge_basins: a maximum lies outside the grid')
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    ensure_labels(ctx, volumes)
    root, rnd, pers, rounds, _, converged = ctx.merge_basins(dirs, np.ravel_multi_index(tuple(vox.T), shape), tol, max_rounds)
    return Merge(root, rnd, pers, rounds, converged)

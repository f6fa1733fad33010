"""The Voronoi partition: every voxel belongs to its nearest atom (`bader -c voronoi` in the Henkelman group's code) -- no
counterpart in the reference.  It is the geometric baseline printed next to the Bader charges: the difference between the two
says how far the zero-flux surfaces bend away from the bisector planes.  The map is an atom map like
thread_handlers.assign_to_atoms' `atoms_volumes`: multipole.moment_sum, adjacency.adjacency, utils.volume_mask and
utils.charge_sum take it unchanged.

    voronoi_assign(density, lattice, atoms, vacuum_tol=None, full_search=False)   -> (volumes, stats)
    voronoi_charges(density, lattice, atoms, voxel_volume, vacuum_tol=None)       -> (charge, volume, volumes)

The search runs in libbader_hip.so (xb_voronoi_assign, csrc/k_voronoi.h); the definition -- voxel position, the 27 images, ties
to the smaller atom index, the vacuum -- is in include/bader_hip.h and DESIGN.md section 16, and tests/test_voronoi_cpu.py
restates it in numpy."""
import numpy as np

from . import _lib, device
from .utils import charge_sum, dtype_calc, ensure_density, fetch_labels


def voronoi_assign(density, lattice, atoms, vacuum_tol=None, full_search=False):
    """The nearest-atom map of the grid of `density`.

    density      host array, or a float32 / float64 device array: it gives the grid's shape and the kind of the result, and
                 with a `vacuum_tol` the vacuum (it is not read, nor uploaded, without one)
    lattice      the CELL's lattice, one row per axis
    atoms        [n, 3] Cartesian, already `atoms - voxel_offset`; searched as given over their 27 periodic images
    vacuum_tol   None, or the density at or below which a voxel gets -1 (as utils.vacuum_assign decides it)
    full_search  every tile of voxels searches all 27 n images instead of its candidate list: the second implementation

    -> (volumes, stats): the map, of dtype_calc(-n) and on the host or the device as assign_to_atoms returns `atoms_volumes` for
    this density, tracked inside utils.resident() like any fetched label map; stats = {'candidate_tiles', 'full_tiles',
    'max_candidates'} of the search."""
    ctx = _lib.default_context()
    shape = tuple(int(n) for n in density.shape)
    atoms = np.ascontiguousarray(atoms, dtype=np.float64).reshape(-1, 3)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    if vacuum_tol is not None:
        ensure_density(ctx, density)
    stats = ctx.voronoi_assign(lattice, atoms, vacuum_tol, full_search)
    dtype = np.dtype(dtype_calc(-atoms.shape[0]))
    return fetch_labels(ctx, dtype=dtype, on_device=device.is_device_array(density)), stats


def voronoi_charges(density, lattice, atoms, voxel_volume, vacuum_tol=None):
    """Charge and volume of every atom's Voronoi cell: voronoi_assign, then utils.charge_sum on that map.
    -> (charge f64[n], volume f64[n], volumes)"""
    volumes, _ = voronoi_assign(density, lattice, atoms, vacuum_tol)
    n = np.asarray(atoms).reshape(-1, 3).shape[0]
    charge, volume = np.zeros(n), np.zeros(n)
    charge_sum(charge, volume, voxel_volume, density, volumes)
    return charge, volume, volumes

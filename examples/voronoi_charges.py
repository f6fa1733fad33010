#!/usr/bin/env python3
"""Bader and Voronoi charge of every atom, side by side:

    python examples/voronoi_charges.py CHGCAR [vacuum_tol]           (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with voronoi_flag=True adds the
Voronoi partition (pybader_amd.voronoi: every voxel belongs to its nearest atom over the periodic images) and sums the same
density over it.  The Voronoi charge is the geometric baseline: the difference between the two columns is the charge that the
bending of the zero-flux surfaces away from the bisector planes moves between neighbours.  The last column is the share of the
atom's Voronoi cell that its Bader atom covers as well."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp        # noqa: E402
from pybader_amd.interface import Bader         # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    path = sys.argv[1]
    tol = float(sys.argv[2]) if len(sys.argv) == 3 else None
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    b = Bader(density, lattice, atoms, info, voronoi_flag=True, vacuum_tol=tol)
    b()
    print(f'{path}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} maxima, {b.atoms.shape[0]} atoms; search: {b.voronoi_stats}')
    print(f'{"atom":>5} {"Bader charge":>14} {"Voronoi charge":>15} {"difference":>12} {"Bader volume":>13} {"Voronoi volume":>15} {"overlap":>8}')
    both, vor = np.asarray(b.atoms_volumes), np.asarray(b.voronoi_volumes)
    for k in range(b.atoms.shape[0]):
        cell = vor == k
        share = float((both[cell] == k).mean()) if cell.any() else float('nan')
        print(f'{k:5d} {b.atoms_charge[k]:14.6f} {b.voronoi_charge[k]:15.6f} {b.atoms_charge[k] - b.voronoi_charge[k]:12.6f} '
              f'{b.atoms_volume[k]:13.6f} {b.voronoi_volume[k]:15.6f} {share:8.4f}')
    print(f'{"sum":>5} {b.atoms_charge.sum():14.6f} {b.voronoi_charge.sum():15.6f}')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Which Bader atoms share an interatomic surface, how large it is and where the density on it is highest:

    python examples/bond_surfaces.py CHGCAR            (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with adjacency_flag=True adds,
per pair of atoms whose volumes touch, the area of their shared surface (in the squared length unit of the file), the density
at its highest point -- the grid estimate of rho at the bond critical point -- and that point's Cartesian position
(pybader_amd.adjacency).  Then the least persistent Bader maxima: those a noisy density is most likely to have invented."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp        # noqa: E402
from pybader_amd.interface import Bader         # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = sys.argv[1]
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    b = Bader(density, lattice, atoms, info, adjacency_flag=True)
    b()
    a = b.atoms_adjacency
    print(f'{path}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} maxima, {b.atoms.shape[0]} atoms, {len(a)} atom pairs in contact')
    print(f'{"atom":>5} {"atom":>5} {"area":>12} {"rho at saddle":>14}   position of the saddle')
    for (i, j), area, rho, pos in zip(a.pairs, b.atoms_bond_area, b.atoms_bond_density, b.atoms_bond_position):
        print(f'{i:5d} {j:5d} {area:12.6f} {rho:14.6e}   {pos[0]:10.5f} {pos[1]:10.5f} {pos[2]:10.5f}')
    order = np.argsort(b.bader_persistence, kind='stable')[:5]
    print('least persistent maxima (volume: maximum minus its highest saddle towards a higher one):',
          ', '.join(f'{m}: {b.bader_persistence[m]:.3e}' for m in order))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Grid charges and weight-method charges per atom, side by side:

    python examples/weight_charges.py CHGCAR            (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube), the default neargrid run gives the grid charges
(atoms_charge) and weight_flag=True adds the weight-method ones (atoms_weight_charge, Yu & Trinkle 2011): on a coarse grid the two
differ by the charge of the staircase surface the grid methods give wholly to one atom."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp        # noqa: E402
from pybader_amd.interface import Bader         # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = sys.argv[1]
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    b = Bader(density, lattice, atoms, info, weight_flag=True)
    b()
    print(f'{path}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} grid maxima, {b.weight_maxima.shape[0]} weight-method maxima')
    print(f'{"atom":>5} {"grid charge":>14} {"weight charge":>14} {"difference":>12} {"grid volume":>13} {"weight volume":>14}')
    for k in range(b.atoms.shape[0]):
        print(f'{k:5d} {b.atoms_charge[k]:14.6f} {b.atoms_weight_charge[k]:14.6f} '
              f'{b.atoms_weight_charge[k] - b.atoms_charge[k]:12.6f} {b.atoms_volume[k]:13.5f} {b.atoms_weight_volume[k]:14.5f}')
    print(f'{"sum":>5} {b.atoms_charge.sum():14.6f} {b.atoms_weight_charge.sum():14.6f}')


if __name__ == '__main__':
    main()

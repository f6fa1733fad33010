#!/usr/bin/env python3
"""Charge, dipole and quadrupole of every Bader atom:

    python examples/multipole_moments.py CHGCAR            (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with multipole_flag=True adds the
moments of each atom's density about its nucleus (pybader_amd.multipole: electrons count positive in the density, so the
electronic dipole is -m1 and the traceless quadrupole -(3 m2 - tr(m2) I), in e * length and e * length^2 of the file's length
unit).  The last column is the trace of the quadrupole, which is zero up to rounding; m0 is the atom's charge again."""
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
    b = Bader(density, lattice, atoms, info, multipole_flag=True)
    b()
    print(f'{path}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} maxima, {b.atoms.shape[0]} atoms')
    print(f'{"atom":>5} {"charge":>14} {"m0 - charge":>12} {"|dipole|":>12} {"largest |Q_ij|":>15} {"tr Q":>10}')
    for k in range(b.atoms.shape[0]):
        q = b.atoms_quadrupole[k]
        print(f'{k:5d} {b.atoms_charge[k]:14.6f} {b.atoms_moments[k, 0] - b.atoms_charge[k]:12.2e} '
              f'{np.linalg.norm(b.atoms_dipole[k]):12.6f} {np.abs(q).max():15.6f} {np.trace(q):10.2e}')
    print(f'{"sum":>5} {b.atoms_charge.sum():14.6f}   total electronic dipole about the nuclei {b.atoms_dipole.sum(axis=0)}')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The Laplacian of a charge density per atom and at the bond points:

    python examples/laplacian.py CHGCAR [vacuum_tol]           (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with laplacian_flag=True and
critical_flag=True adds, per atom, L = the integral of the Laplacian over the atom's basin -- zero for an exact zero-flux basin,
so |L| over the integral of |Laplacian| says how good the integration is -- and, per bonded pair of atoms, rho, the Laplacian
and the ellipticity at the bond point (pybader_amd.laplacian): a negative Laplacian there marks a shared-shell (covalent)
interaction, a positive one a closed-shell interaction, and eigenvalues near zero a shallow saddle of the tails."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp, laplacian     # noqa: E402
from pybader_amd.interface import Bader                 # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    path = sys.argv[1]
    tol = float(sys.argv[2]) if len(sys.argv) == 3 else None
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    b = Bader(density, lattice, atoms, info, laplacian_flag=True, critical_flag=True, vacuum_tol=tol)
    b()
    print(f'{path}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} Bader maxima, {b.atoms.shape[0]} atoms')
    print(f'{"atom":>4} {"charge":>12} {"volume":>12} {"L":>12} {"|L| / L_abs":>12}')
    for i, (q, v, L, La) in enumerate(zip(b.atoms_charge, b.atoms_volume, b.atoms_laplacian, b.atoms_laplacian_abs)):
        print(f'{i:4d} {q:12.6f} {v:12.6f} {L:12.4e} {(abs(L) / La if La else 0.0):12.4e}')
    g = b.atoms_bond_graph
    p = laplacian.point_properties(b.reference, b.lattice, g.voxels)      # (the eigenvalues too; the flag keeps two columns of it)
    print(f'bond graph: {len(g)} bonded pairs of atoms')
    print(f'{"a":>4} {"b":>4} {"rho_b":>12} {"laplacian":>12} {"ellipticity":>12} {"l1":>10} {"l2":>10} {"l3":>10}')
    for (i, j), r, lap, e, ev in zip(b.atoms_bonds.tolist(), b.atoms_bond_density.tolist(), b.atoms_bond_laplacian.tolist(),
                                     b.atoms_bond_ellipticity.tolist(), p.eigenvalues):
        print(f'{i:4d} {j:4d} {r:12.6f} {lap:12.6f} {e:12.6f} {ev[0]:10.4f} {ev[1]:10.4f} {ev[2]:10.4f}')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The molecular envelope of a charge density -- its area, its volume and the volume each atom has inside it -- as a PLY mesh:

    python examples/isosurface.py CHGCAR [level]           (or a .cube file)
    python examples/isosurface.py --nci CHGCAR [s_cut rho_cut]

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with isosurface_level set adds the
surface density == level (pybader_amd.isosurface: marching tetrahedra on the lattice of the critical points, closed and
consistently oriented), its area and the volume inside it, in total and per atom next to the atom's Bader volume (AIMAll's
Vol(0.001)).  The level defaults to 0.001 e / bohr^3; both readers return e / Angstrom^3, so it is converted with nci.E_PER_A3
unless it is given.  With --nci the surface s = s_cut of the reduced density gradient, coloured by sign(lambda2) rho, is written
instead (nci.nci_isosurface; the thresholds default to 0.5 and 0.05 e / bohr^3).  The mesh goes next to the input as a binary
PLY, vertices in the lattice's length unit, with the colour as a vertex property."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp, nci     # noqa: E402
from pybader_amd.interface import Bader          # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a != '--nci']
    want_nci = len(args) != len(sys.argv) - 1
    if not args or len(args) > (3 if want_nci else 2):
        sys.exit(__doc__)
    path = args[0]
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    if want_nci:
        s_cut = float(args[1]) if len(args) > 1 else nci.S_CUT
        rho_cut = float(args[2]) if len(args) > 2 else nci.RHO_CUT * nci.E_PER_A3
        m = nci.nci_isosurface(density['charge'], lattice, s_cut, rho_cut)
        out = info['prefix'] + 'NCI-isosurface.ply'
        m.write_ply(out)
        print(f'{path}: s = {s_cut:g} where rho < {rho_cut:g}: {m.vertices.shape[0]} vertices, {len(m)} triangles, area {m.area:.6f}')
        if len(m):
            print(f'sign(lambda2) rho on the surface: {m.colour.min():.6f} .. {m.colour.max():.6f}')
        print('wrote', out)
        return
    level = float(args[1]) if len(args) > 1 else 0.001 * nci.E_PER_A3
    b = Bader(density, lattice, atoms, info, isosurface_level=level)
    b()
    m = b.isosurface
    print(f'{path}: grid {b.grid_shape}, {b.atoms.shape[0]} atoms; envelope rho = {level:g}')
    print(f'{m.vertices.shape[0]} vertices, {len(m)} triangles, Euler characteristic {m.euler}')
    print(f'area {b.isosurface_area:.6f}   volume {b.isosurface_volume:.6f}   (cell {abs(b.voxel_volume) * density["charge"].size:.6f})')
    print(f'{"atom":>4} {"Bader volume":>16} {"inside envelope":>16}')
    for i, (vol, inside) in enumerate(zip(b.atoms_volume, b.atoms_isosurface_volume)):
        print(f'{i:4d} {vol:16.6f} {inside:16.6f}')
    out = info['prefix'] + 'isosurface.ply'
    m.write_ply(out)
    print('wrote', out)


if __name__ == '__main__':
    main()

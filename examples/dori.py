#!/usr/bin/env python3
"""Where the densities of atoms overlap -- covalent bonds and non-covalent contacts in one picture: DORI, the density overlap
regions indicator.

    python examples/dori.py CHGCAR [d_cut rho_min rho_split]           (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with dori_flag=True and
dori_domains_flag=True (pybader_amd.dori) prints

  - one line per atom: the volume and the electrons of the region gamma >= d_cut inside the atom's basin, split by
    sign(lambda2) rho into attractive, van der Waals and repulsive parts;
  - one line per connected domain of that region -- one per bond or contact: the two atoms it lies between, its class, its
    voxels, its volume, the electrons in it, gamma at its densest voxel and where that voxel lies;

writes the surface gamma = d_cut coloured by sign(lambda2) rho next to the input as DORI-surface.ply, and shows the populations
of the DORI basins: gamma handed to a second Bader run as the reference field, the density as the charge that is summed.  The
thresholds default to 0.9 and, in atomic units, 0.001 and 0.01, converted with dori.E_PER_A3 for the e / Angstrom^3 both readers
return."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import _lib, dori, io_cube, io_vasp     # noqa: E402
from pybader_amd.interface import Bader                   # noqa: E402


def main():
    if len(sys.argv) not in (2, 5):
        sys.exit(__doc__)
    path = sys.argv[1]
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    if len(sys.argv) == 5:
        d_cut, rho_min, rho_split = (float(a) for a in sys.argv[2:])
    else:
        d_cut, rho_min, rho_split = dori.D_CUT, dori.RHO_MIN * dori.E_PER_A3, dori.RHO_SPLIT * dori.E_PER_A3
    b = Bader(density, lattice, atoms, info, dori_flag=True, dori_domains_flag=True, dori_cut=d_cut, dori_rho_min=rho_min,
              dori_rho_split=rho_split)
    b()
    print(f'{path}: grid {b.grid_shape}, {b.atoms.shape[0]} atoms; region gamma >= {d_cut:g} where rho > {rho_min:g}, split at {rho_split:g}')
    print(f'{"atom":>4} ' + ' '.join(f'{"V " + c:>16} {"q " + c:>16}' for c in dori.CLASSES))
    for i, (vol, q) in enumerate(zip(b.atoms_dori_volume, b.atoms_dori_charge)):
        print(f'{i:4d} ' + ' '.join(f'{vol[k]:16.6f} {q[k]:16.6f}' for k in range(3)))
    d = b.dori_domains
    print(f'{d.m} domains')
    print(f'{"domain":>6} {"atoms":>9} {"class":>14} {"voxels":>9} {"volume":>14} {"electrons":>14} {"gamma":>9}   position of the top voxel')
    for i in range(d.m):
        a0, a1 = b.dori_domain_atoms[i]
        pos = b.dori_domain_position[i]
        print(f'{i:6d} {a0:4d} {a1:4d} {dori.CLASSES[b.dori_domain_kind[i]]:>14} {b.dori_domain_count[i]:9d} {b.dori_domain_volume[i]:14.6f} '
              f'{b.dori_domain_charge[i]:14.6f} {b.dori_domain_value[i]:9.5f}   {pos[0]:10.5f} {pos[1]:10.5f} {pos[2]:10.5f}')
    mesh = dori.dori_isosurface(b.reference, b.lattice, d_cut, rho_min)
    ply = info.get('prefix', '') + 'DORI-surface.ply'
    mesh.write_ply(ply)
    print(f'wrote {ply}: {len(mesh)} triangles, area {mesh.area:.6f}')
    # DORI basins: gamma is the field that is partitioned, rho the charge that is summed (the existing reference path)
    gamma, _ = dori.dori_fields(b.reference, b.lattice, rho_min, colour=False)
    try:
        basins = Bader({'charge': b.charge}, lattice, atoms, info, reference=gamma)
        basins()
    except _lib.BaderHipError:      # (a device field the path refuses: the host copy of gamma)
        basins = Bader({'charge': np.asarray(b.charge)}, lattice, atoms, info, reference=np.ascontiguousarray(gamma.to_host()))
        basins()
    order = np.argsort(-basins.bader_charge)[:12]
    print(f'{basins.bader_charge.shape[0]} DORI basins; the most populated:')
    for k in order:
        print(f'  basin {k:6d}  nearest atom {basins.bader_atoms[k]:4d}  electrons {basins.bader_charge[k]:12.6f}  volume {basins.bader_volume[k]:12.6f}')


if __name__ == '__main__':
    main()

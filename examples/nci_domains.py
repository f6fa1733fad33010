#!/usr/bin/env python3
"""The single contacts of a charge density: the NCI region split into its connected domains.

    python examples/nci_domains.py CHGCAR [s_cut rho_cut rho_split]           (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with nci_flag=True and
nci_domains_flag=True splits the low-s, low-rho region into its connected pieces (pybader_amd.nci.nci_domains) and prints one line
per domain: the two atoms that hold most of it, its class (that of its densest voxel: attractive, van der Waals or repulsive), its
voxels, its volume, the integral of the density over it and where its densest voxel lies.  The thresholds default to the usual 0.5,
0.05 and 0.01 in atomic units, converted with nci.E_PER_A3 for the e / Angstrom^3 both readers return.  The islands of the 0.001
envelope (pybader_amd.regions.connected_regions) are counted as well: how many molecules the cell holds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp, nci, regions     # noqa: E402
from pybader_amd.interface import Bader                     # noqa: E402


def main():
    if len(sys.argv) not in (2, 5):
        sys.exit(__doc__)
    path = sys.argv[1]
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    if len(sys.argv) == 5:
        s_cut, rho_cut, rho_split = (float(a) for a in sys.argv[2:])
    else:
        s_cut, rho_cut, rho_split = nci.S_CUT, nci.RHO_CUT * nci.E_PER_A3, nci.RHO_SPLIT * nci.E_PER_A3
    b = Bader(density, lattice, atoms, info, nci_flag=True, nci_domains_flag=True, nci_s_cut=s_cut, nci_rho_cut=rho_cut,
              nci_rho_split=rho_split)
    b()
    d = b.nci_domains
    print(f'{path}: grid {b.grid_shape}, {b.atoms.shape[0]} atoms; region s < {s_cut:g}, rho < {rho_cut:g}, split at {rho_split:g}: '
          f'{d.m} domains')
    print(f'{"domain":>6} {"atoms":>9} {"class":>14} {"voxels":>9} {"volume":>14} {"charge":>14}   position of the top voxel')
    for i in range(d.m):
        a0, a1 = b.nci_domain_atoms[i]
        pos = b.nci_domain_position[i]
        print(f'{i:6d} {a0:4d} {a1:4d} {nci.CLASSES[b.nci_domain_kind[i]]:>14} {d.size[i]:9d} {b.nci_domain_volume[i].sum():14.6f} '
              f'{d.total[i]:14.6f}   {pos[0]:10.5f} {pos[1]:10.5f} {pos[2]:10.5f}')
    level = 0.001 * nci.E_PER_A3
    r = regions.connected_regions(b.reference, level, voxel_volume=b.voxel_volume, volumes=b.atoms_volumes, n=b.atoms.shape[0])
    print(f'the envelope rho >= {level:g}: {r.m} piece(s); volumes {[round(float(v), 4) for v in r.volume[:8]]}'
          + (' ...' if r.m > 8 else ''))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""WHOSE interaction is it?  The independent gradient model (IGM / IGMH): delta-g_inter between user-named fragments.

    python examples/igm.py CHGCAR FRAGMENTS [cut [r_cut [mode]]]          (or a .cube file)

FRAGMENTS names the fragment of every atom, in the file's order, as digits 0 .. 3, '-' for an atom in none: 00001111 puts the
first four atoms into fragment 0 and the next four into fragment 1.  The file is read by this package's own readers (io_vasp /
io_cube).  No free-atom data is shipped, so the example makes its atomic densities from the file itself: it runs the iterative
stockholder analysis (isa_flag), takes each atom's converged shells as the knots of a table that is linear in r^2
(hirshfeld.ProAtoms; the ISA tables themselves are piecewise constant and have no gradient), and runs igm.igm_domains and
igm.igm_isosurface with them.  A user with free-atom densities passes them as `proatoms` and `species` instead.  It prints

  - one line per atom: the volume, the electrons and the integral of delta-g_inter of the region delta-g_inter >= cut inside the
    atom's basin, split by sign(lambda2) rho into attractive, van der Waals and repulsive parts;
  - one line per connected domain of that region -- one per contact between fragments: the two atoms it lies between, its class,
    its voxels, its volume, the integral of delta-g_inter over it, its value at the domain's densest voxel;

and writes the surface delta-g_inter = cut coloured by sign(lambda2) rho next to the input as IGM-surface.ply.  cut defaults to
igm.DG_CUT (in the units of the file's density gradient), r_cut to 3.0 (the ISA atoms' cutoff), mode to 'stockholder' (IGMH)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import igm, io_cube, io_vasp             # noqa: E402
from pybader_amd.hirshfeld import ProAtoms                 # noqa: E402
from pybader_amd.interface import Bader                    # noqa: E402
from pybader_amd.isa import isa_charges                    # noqa: E402


def main():
    if not 3 <= len(sys.argv) <= 6:
        sys.exit(__doc__)
    path, word = sys.argv[1], sys.argv[2]
    cut = float(sys.argv[3]) if len(sys.argv) > 3 else igm.DG_CUT
    r_cut = float(sys.argv[4]) if len(sys.argv) > 4 else 3.0
    mode = sys.argv[5] if len(sys.argv) > 5 else 'stockholder'
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    density, lattice, atoms, info = reader.read(path)
    fragments = np.array([-1 if ch == '-' else int(ch) for ch in word], np.int32)
    if fragments.shape[0] != len(atoms):
        sys.exit(f'{path} has {len(atoms)} atoms, FRAGMENTS names {fragments.shape[0]}')
    b = Bader(density, lattice, atoms, info)
    b()
    n, sites = b.atoms.shape[0], b.atoms - b.voxel_offset
    r = isa_charges(b.density, b.lattice, sites, b.voxel_volume, r_cut=r_cut)
    print(f'{path}: grid {b.grid_shape}, {n} atoms; ISA {"converged" if r.converged else "stopped"} after {r.iterations} iterations')
    pro = ProAtoms(np.concatenate([r.tables, np.zeros((n, 1))], axis=1), r.r_cut)      # the shells as knots, linear in r^2 between
    kw = dict(species=np.arange(n, dtype=np.int32), proatoms=pro, mode=mode)
    rho_split = igm.RHO_SPLIT * igm.E_PER_A3
    reg = igm.igm_regions(b.density, b.atoms_volumes, b.lattice, sites, fragments, n, b.voxel_volume, cut, rho_split, **kw)
    print(f'region delta-g_inter >= {cut:g} ({mode}), split at |sign(lambda2) rho| = {rho_split:g}')
    print(f'{"atom":>4} {"frag":>4} ' + ' '.join(f'{"V " + c:>16} {"q " + c:>16} {"I " + c:>16}' for c in igm.CLASSES))
    for i in range(n):
        print(f'{i:4d} {fragments[i]:4d} ' + ' '.join(f'{reg.volume[i, k]:16.6f} {reg.charge[i, k]:16.6f} {reg.integral[i, k]:16.6f}' for k in range(3)))
    d = igm.igm_domains(b.density, b.lattice, sites, fragments, b.atoms_volumes, n, b.voxel_volume, cut, rho_split, **kw)
    print(f'{d.m} domains')
    print(f'{"domain":>6} {"atoms":>9} {"class":>14} {"voxels":>9} {"volume":>14} {"integral":>14} {"delta-g_inter":>14}')
    for i in range(d.m):
        print(f'{i:6d} {d.atoms[i, 0]:4d} {d.atoms[i, 1]:4d} {igm.CLASSES[d.kind[i]]:>14} {d.count[i]:9d} {d.volume[i]:14.6f} '
              f'{d.integral[i]:14.6f} {d.value[i]:14.6f}')
    mesh = igm.igm_isosurface(b.density, b.lattice, sites, fragments, cut, **kw)
    ply = info.get('prefix', '') + 'IGM-surface.ply'
    mesh.write_ply(ply)
    print(f'wrote {ply}: {len(mesh)} triangles, area {mesh.area:.6f}')


if __name__ == '__main__':
    main()

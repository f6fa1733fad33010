#!/usr/bin/env python3
"""The non-covalent interaction (NCI) regions of a charge density per atom:

    python examples/nci.py CHGCAR [s_cut rho_cut rho_split]           (or a .cube file)

The file is read by this package's own readers (io_vasp / io_cube); the default neargrid run with nci_flag=True adds, per atom,
the volume and the charge of the low-s, low-rho region of the atom's basin, split by sign(lambda2) rho into attractive (hydrogen
bonds), van der Waals and repulsive (steric) parts (pybader_amd.nci).  The thresholds default to the usual 0.5, 0.05 and 0.01 in
atomic units; a CHGCAR read by io_vasp is in e / Angstrom^3, so the two density thresholds are converted with nci.E_PER_A3
unless they are given.  The two fields -- the reduced gradient s and sign(lambda2) rho -- are written next to the input with the
file type's own writer, as NCI-s and NCI-sign_lambda2_rho (s is +inf where the density is not positive; the file holds 100 there,
as NCIPLOT's cube files do)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp, nci     # noqa: E402
from pybader_amd.interface import Bader          # noqa: E402


def main():
    if len(sys.argv) not in (2, 5):
        sys.exit(__doc__)
    path = sys.argv[1]
    cube = path.lower().endswith(('.cube', '.cub'))
    reader = io_cube if cube else io_vasp
    density, lattice, atoms, info = reader.read(path)
    if len(sys.argv) == 5:
        s_cut, rho_cut, rho_split = (float(a) for a in sys.argv[2:])
    else:
        # (both readers return Angstrom and e / Angstrom^3: pybader's convention)
        s_cut, rho_cut, rho_split = nci.S_CUT, nci.RHO_CUT * nci.E_PER_A3, nci.RHO_SPLIT * nci.E_PER_A3
    b = Bader(density, lattice, atoms, info, nci_flag=True, nci_s_cut=s_cut, nci_rho_cut=rho_cut, nci_rho_split=rho_split)
    b()
    print(f'{path}: grid {b.grid_shape}, {b.atoms.shape[0]} atoms; region s < {s_cut:g}, rho < {rho_cut:g}, split at {rho_split:g}')
    print(f'{"atom":>4} ' + ' '.join(f'{"V " + c:>16} {"q " + c:>16}' for c in nci.CLASSES))
    for i, (vol, q) in enumerate(zip(b.atoms_nci_volume, b.atoms_nci_charge)):
        print(f'{i:4d} ' + ' '.join(f'{vol[k]:16.6f} {q[k]:16.6f}' for k in range(3)))
    total = b.atoms_nci_volume.sum(axis=0)
    print('all  ' + ' '.join(f'{total[k]:16.6f} {b.atoms_nci_charge[:, k].sum():16.6f}' for k in range(3)))
    s, x = nci.nci_fields(b.reference, b.lattice)
    out = dict(info)
    out['charge_flag'], out['spin_flag'], out['fortran_format'] = True, False, 0
    for name, field in (('NCI-s', np.where(np.isfinite(s), s, 100.0)), ('NCI-sign_lambda2_rho', x)):
        out['comment'] = name + '\n'
        info['write_function'](name, b.atoms, b.lattice, {'charge': np.ascontiguousarray(field)}, out, prefix=info['prefix'])
        print('wrote', info['prefix'] + name + ('.cube' if cube else '-CHGCAR'))


if __name__ == '__main__':
    main()

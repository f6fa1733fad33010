"""Gaussian / CP2K cube writer with the density block formatted on the GPU.

Same call signature and file as the reference's `pybader.io.cube.write` (io/cube.py:186-240): the charge density in
Bohr units (times bohr_to_ang**3), the lattice and atoms converted to Bohr, the voxel vectors on the grid lines, and
every (x, y) record of nz values in lines of six, the remainder of the record on a line of its own; the numbers as
the reference's python_format / fortran_format (`file_info['fortran_format']` 0, 1 or 2), byte for byte.
Deliberate difference: `atoms`, `lattice` and `density` are left as they are (the reference converts them in place,
so a second export from the same object would be written in the wrong units).  A cube reader is not part of this
module.
"""
import numpy as np

from . import _lib, textfmt
from .io_vasp import header_number, header_precision

__extensions__ = ['.cube']

bohr_to_ang = .52917721067
ang_to_bohr = 1 / bohr_to_ang


def write(fn, atoms, lattice, density, file_info, prefix=None, suffix='.cube', ctx=None):
    """Write `density['charge']` ([x][y][z]) as a cube file named `prefix + fn + suffix` (no prefix when None)."""
    ctx = ctx or _lib.default_context()
    if prefix is not None:
        fn = prefix + fn
    fn += suffix
    style = textfmt.style_of(file_info.get('fortran_format', 0))
    charge = density['charge']
    shape = np.asarray(charge).shape
    atoms = np.asarray(atoms, dtype=np.float64) * ang_to_bohr
    lattice = np.asarray(lattice, dtype=np.float64) * ang_to_bohr
    lattice = lattice / np.asarray(shape)
    lattice_prec = header_precision(lattice[lattice != 0])
    atoms_prec = header_precision(atoms[atoms != 0])
    head = ["Cube File writen in pybader\n", file_info['comment'], f"{atoms.shape[0]:>5}{'  0.0000000' * 3}\n"]
    for i, row in enumerate(lattice):
        head.append(f"{shape[i]:>5}" + ''.join(header_number(v, lattice_prec) for v in row) + '\n')
    for i, row in enumerate(atoms):
        head.append(f"{file_info['elements'][i]:>5}" + '  0.0000000'
                    + ''.join(header_number(v, atoms_prec) for v in row) + '\n')
    with open(fn, 'wb') as f:
        f.write(''.join(head).encode())
        textfmt.write_block(f, ctx, charge, bohr_to_ang ** 3, style, 5, 'cube')

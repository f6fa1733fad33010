"""Gaussian / CP2K cube reader and writer with the density block parsed / formatted on the GPU.

`read` has the call signature and return value of the reference's `pybader.io.cube.read` (io/cube.py:18-137):
`(density, lattice, atoms, file_info)`, the lattice and atoms in Angstrom (atoms wrapped into the cell), the density
times ang_to_bohr**3.  The header is read with the reference's numpy operations in its order, so `lattice` and `atoms`
are its arrays bit for bit.  The density block is handed to `xb_parse_cube_text` as raw bytes (memory mapped) and
converted on the device, bit-identical to numpy's string -> float64 times ang_to_bohr**3; the charge density stays
resident for the following `bader_calc`.  `file_info['write_function']` is `write`, so `Bader.write_volume` exports
without pybader installed.
Deliberate differences, all where the reference cannot read the file (nval > 1 values per voxel) or cuts it:
* nval comes from the fifth number of line 3 (Gaussian; the reference reads a sixth and raises IndexError) or, with a
  negative atom count, from the list of orbital ids after the atoms, which may wrap over several lines (the reference
  swallows the first data line after it and raises ValueError);
* `orbitals` does what the reference's docstring says: 0 sums every value of a voxel when the atom count is negative
  and takes the first one otherwise, an id > 0 takes that orbital, an iterable of ids sums them in the order listed,
  a negative number returns every orbital as an array [nval][x][y][z] (the reference would return [nval][y][z][x]).
  Ids are the listed ones, 1..nval without a list; an unknown id raises ValueError;
* the block is read as whitespace separated numbers, whatever the width of its lines (the reference reads whole
  records by byte counts taken from the first line, which cuts a number in two when the lines differ in width).

`write` has the call signature and file as the reference's `pybader.io.cube.write` (io/cube.py:186-240): the charge density in
Bohr units (times bohr_to_ang**3), the lattice and atoms converted to Bohr, the voxel vectors on the grid lines, and
every (x, y) record of nz values in lines of six, the remainder of the record on a line of its own; the numbers as
the reference's python_format / fortran_format (`file_info['fortran_format']` 0, 1 or 2), byte for byte.
Deliberate difference: `atoms`, `lattice` and `density` are left as they are (the reference converts them in place,
so a second export from the same object would be written in the wrong units).
"""
import collections
import mmap
import os

import numpy as np

from . import _lib, textfmt, utils
from .interface import distance_matrix, gradient_transform
from .io_vasp import _line, header_number, header_precision

__extensions__ = ['.cube']
__args__ = ['orbitals']

bohr_to_ang = .52917721067
ang_to_bohr = 1 / bohr_to_ang

CubeHeader = collections.namedtuple('CubeHeader', 'lattice atoms elements shape nval ids atom_count data_offset')


def read_header(buf):
    """The header of a cube file held in `buf` (bytes, mmap): lattice and atoms in Angstrom as the reference computes
    them (io/cube.py:49-81, 131-132), the element numbers (int64), the grid, the number of values per voxel and their
    ids, the atom count as written (negative: an id list follows the atoms) and the byte offset of the density block."""
    _, pos = _line(buf, 0)                                     # two comment lines
    _, pos = _line(buf, pos)
    text, pos = _line(buf, pos)
    line = text.split()
    atom_count = int(line[0])                                  # (the origin is ignored, as in the reference)
    nval = int(line[4]) if len(line) > 4 else 1
    shape = np.zeros(3, dtype=np.int64)
    lattice = np.zeros((3, 3), dtype=np.float64)
    for i in range(3):
        text, pos = _line(buf, pos)
        line = text.split()
        shape[i] = line[0]
        lattice[i] = line[1:]
        lattice[i] *= shape[i]
    elements = np.zeros(abs(atom_count), dtype=np.int64)
    atoms = np.zeros((abs(atom_count), 3), dtype=np.float64)
    for i in range(abs(atom_count)):
        text, pos = _line(buf, pos)
        line = text.split()
        elements[i] = line[0]
        atoms[i] = line[-3:]
    atoms = np.dot(atoms, np.linalg.inv(lattice))              # wrapped into the cell in fractional coordinates
    atoms %= 1
    atoms = np.dot(atoms, lattice)
    ids = np.arange(1, nval + 1, dtype=np.int64)
    if atom_count < 0:                                         # id count, then the ids, over one or more lines
        text, pos = _line(buf, pos)
        line = text.split()
        ids = np.zeros(int(line.pop(0)), dtype=np.int64)
        nval, count = ids.shape[0], 0
        while True:
            for m in line[:nval - count]:
                ids[count] = m
                count += 1
            if count >= nval:
                break
            if pos >= len(buf):
                raise ValueError(f'cube header: {count} of {nval} orbital ids before the end of the file')
            text, pos = _line(buf, pos)
            line = text.split()
    if nval < 1:
        raise ValueError(f'cube header: {nval} values per voxel')
    lattice *= bohr_to_ang
    atoms *= bohr_to_ang
    return CubeHeader(lattice, atoms, elements, tuple(int(g) for g in shape), nval, ids, atom_count, pos)


def _orbital_picks(head, orbitals):
    """the value indices to sum for `orbitals` (None: every orbital on its own)"""
    ids = [int(i) for i in head.ids]

    def pick(m):
        if int(m) not in ids:
            raise ValueError(f'orbital {m} is not in the file (ids {ids})')
        return ids.index(int(m))

    if head.nval == 1:
        return [0]                                             # the reference ignores `orbitals` here
    if hasattr(orbitals, '__iter__'):
        picks = [pick(m) for m in orbitals]
        if not picks:
            raise ValueError('orbitals: an empty selection')
        return picks
    if orbitals < 0:
        return None
    if orbitals > 0:
        return [pick(orbitals)]
    return list(range(head.nval)) if head.atom_count < 0 else [0]


def read(fn, orbitals=0, ctx=None):
    """Read the density of a cube file; `orbitals` selects among nval > 1 values per voxel (module docstring)."""
    ctx = ctx or _lib.default_context()
    prefix, _ = os.path.split(fn)
    prefix = os.path.join(prefix, '')
    scale = ang_to_bohr ** 3
    density = {}
    with open(fn, 'rb') as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        block = None
        try:
            head = read_header(mm)
            picks = _orbital_picks(head, orbitals)
            vl = head.lattice / np.array(head.shape, dtype=np.float64)[:, None]
            ctx.set_grid(head.shape, distance_matrix(vl), gradient_transform(vl))
            block = np.frombuffer(mm, dtype=np.uint8)[head.data_offset:]   # to the end of the file
            if picks is None:                                  # every orbital: [nval][x][y][z], not resident
                charge = np.empty((head.nval,) + head.shape, dtype=np.float64)
                for k in range(head.nval):
                    ctx.parse_cube_text(block, scale, head.nval, k)
                    charge[k] = ctx.download_density()
                density['charge'] = charge
            else:                                              # ((a + b) + c) * scale, left to right as np.sum
                for n, k in enumerate(picks):
                    last = n == len(picks) - 1
                    ctx.parse_cube_text(block, scale if last else 1.0, head.nval, k, accumulate=n > 0)
                density['charge'] = ctx.download_density()
                utils.remember_density(ctx, density['charge'])
        finally:
            block = None
            try:
                mm.close()
            except BufferError:                                # a failed parse's traceback still holds the view:
                pass                                           # the map closes when that is collected
    file_info = {
        'filename': fn,
        'prefix': prefix,
        'file_type': 'cube',
        'write_function': write,
        'elements': head.elements,
        'voxel_offset': np.array([.5, .5, .5]),
    }
    return density, head.lattice, head.atoms, file_info


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

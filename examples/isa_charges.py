#!/usr/bin/env python3
"""Bader, Voronoi and ISA charge of every atom, side by side -- and the Hirshfeld charge when pro-atoms are given:

    python examples/isa_charges.py                                   the synthetic 8-atom cell at 64^3
    python examples/isa_charges.py CHGCAR [--r-cut 3.0] [--shells K] [--tol 1e-6] [--free-atoms ATOM1 ATOM2 ...]

The iterative stockholder atoms (ISA, pybader_amd.isa) are Hirshfeld's weights WITHOUT pro-atoms: each atom's weight function is
the spherical average of that atom's own share of the density, iterated to self-consistency.  Nothing but the density file is
needed, so this runs on any CHGCAR / CHG / .cube.  With --free-atoms (one free-atom density file per atom of the cell, in the
cell's order, as examples/hirshfeld_charges.py takes them) the plain Hirshfeld charge is printed beside it.

Without arguments the density is pybader_amd.synth's 8-atom cell, whose atoms have known integrals, and the pro-atoms are sampled
from synth's own atom profile."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp, synth        # noqa: E402
from pybader_amd.hirshfeld import ProAtoms             # noqa: E402
from pybader_amd.interface import Bader                # noqa: E402


def read(path):
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    return reader.read(path)


def synthetic(n=64, r_cut=3.0, knots=4096):
    lat, a5 = synth.CUBIC6, synth.ATOMS8
    rho = synth.synth_density((n, n, n), lat, a5) - synth.BACKGROUND
    x = np.arange(knots + 1, dtype=np.float64) * (r_cut * r_cut) / knots
    tab = np.stack([a[4] * np.maximum(1.0 - x / (2048.0 * a[3] * a[3]), 0.0) ** 1024 for a in a5])
    tab[:, -1] = 0.0
    return {'charge': rho}, lat, synth.atoms_cartesian(a5, lat), None, ProAtoms(tab, np.full(len(a5), r_cut)), np.arange(len(a5))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('density', nargs='?')
    ap.add_argument('--free-atoms', nargs='*', default=[])
    ap.add_argument('--r-cut', type=float, default=3.0)
    ap.add_argument('--shells', type=int, default=None)
    ap.add_argument('--tol', type=float, default=1e-6)
    ap.add_argument('--knots', type=int, default=4096)
    a = ap.parse_args()
    pro, species = None, None
    if a.density is None:
        density, lattice, atoms, info, pro, species = synthetic(r_cut=a.r_cut)
        what = 'the synthetic 8-atom cell'
    else:
        density, lattice, atoms, info = read(a.density)
        what = a.density
        if a.free_atoms:
            if len(a.free_atoms) != len(atoms):
                sys.exit(f'{a.density} holds {len(atoms)} atoms: one free-atom file per atom is wanted, {len(a.free_atoms)} were given')
            made, species = {}, []
            for path in a.free_atoms:
                if path not in made:
                    d, lat1, _, _ = read(path)
                    rho1 = np.asarray(d['charge'], dtype=np.float64)
                    centre = (np.array(np.unravel_index(int(rho1.argmax()), rho1.shape)) / rho1.shape) @ np.asarray(lat1)
                    made[path] = (len(made), ProAtoms.from_density(rho1, lat1, centre, a.r_cut, a.knots))
                species.append(made[path][0])
            for _, p in sorted(made.values(), key=lambda t: t[0]):
                pro = p if pro is None else pro.joined(p)
    extra = {} if pro is None else {'hirshfeld_flag': True, 'proatoms': pro, 'species': np.asarray(species)}
    b = Bader(density, lattice, atoms, info, voronoi_flag=True, isa_flag=True, isa_r_cut=a.r_cut, isa_shells=a.shells, isa_tol=a.tol,
              **extra)
    b()
    state = 'converged' if b.isa_converged else 'NOT converged'
    print(f'{what}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} maxima, {b.atoms.shape[0]} atoms; ISA {state} to {a.tol:g} after '
          f'{b.isa_iterations} iterations')
    hirsh = pro is not None
    print(f'{"atom":>5} {"Bader":>12} {"Voronoi":>12} {"ISA":>12}' + (f' {"Hirshfeld":>12}' if hirsh else '') + f' {"ISA vol":>11}')
    for k in range(b.atoms.shape[0]):
        print(f'{k:5d} {b.atoms_charge[k]:12.6f} {b.voronoi_charge[k]:12.6f} {b.isa_charge[k]:12.6f}'
              + (f' {b.hirshfeld_charge[k]:12.6f}' if hirsh else '') + f' {b.isa_volume[k]:11.5f}')
    print(f'{"sum":>5} {b.atoms_charge.sum():12.6f} {b.voronoi_charge.sum():12.6f} {b.isa_charge.sum():12.6f}'
          + (f' {b.hirshfeld_charge.sum():12.6f}' if hirsh else '')
          + f'   (beyond every atom\'s r_cut: charge {b.isa_rest[0]:.3e} in a volume of {b.isa_rest[1]:.3f})')


if __name__ == '__main__':
    main()

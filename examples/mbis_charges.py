#!/usr/bin/env python3
"""Bader, Voronoi, ISA and MBIS charge of every atom, side by side:

    python examples/mbis_charges.py                                  the synthetic 8-atom cell at 64^3
    python examples/mbis_charges.py CHGCAR [--shells 1] [--r-cut 5.0] [--tol 1e-6] [--isa-r-cut 3.0]

The minimal-basis iterative stockholder atoms (MBIS, pybader_amd.mbis) are iterative Hirshfeld weights whose pro-atoms are sums of
a few Slater shells N / (8 pi sigma^3) exp(-r / sigma), fitted to each atom's own share of the density.  Like ISA (pybader_amd.isa)
they need nothing but the density file, so this runs on any CHGCAR / CHG / .cube; unlike ISA an atom has a handful of numbers of
state, and the iteration converges in tens of steps.  The populations and widths of the fitted shells are printed below the charges,
with the share of each atom's model that the cutoff truncates.

Without arguments the density is pybader_amd.synth's 8-atom cell, whose atoms have known integrals."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import io_cube, io_vasp, mbis, synth        # noqa: E402
from pybader_amd.interface import Bader                      # noqa: E402


def read(path):
    reader = io_cube if path.lower().endswith(('.cube', '.cub')) else io_vasp
    return reader.read(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('density', nargs='?')
    ap.add_argument('--shells', type=int, default=1)
    ap.add_argument('--r-cut', type=float, default=5.0)
    ap.add_argument('--isa-r-cut', type=float, default=3.0)
    ap.add_argument('--tol', type=float, default=1e-6)
    a = ap.parse_args()
    if a.density is None:
        lattice, a5 = synth.CUBIC6, synth.ATOMS8
        density = {'charge': synth.synth_density((64, 64, 64), lattice, a5) - synth.BACKGROUND}
        atoms, info, what = synth.atoms_cartesian(a5, lattice), None, 'the synthetic 8-atom cell'
    else:
        density, lattice, atoms, info = read(a.density)
        what = a.density
    b = Bader(density, lattice, atoms, info, voronoi_flag=True, isa_flag=True, isa_r_cut=a.isa_r_cut, isa_tol=a.tol,
              mbis_flag=True, mbis_shells=a.shells, mbis_r_cut=a.r_cut, mbis_tol=a.tol)
    b()
    said = lambda ok: 'converged' if ok else 'NOT converged'
    print(f'{what}: grid {b.grid_shape}, {b.bader_maxima.shape[0]} maxima, {b.atoms.shape[0]} atoms; ISA {said(b.isa_converged)} after '
          f'{b.isa_iterations} iterations, MBIS {said(b.mbis_converged)} after {b.mbis_iterations}')
    print(f'{"atom":>5} {"Bader":>12} {"Voronoi":>12} {"ISA":>12} {"MBIS":>12} {"MBIS vol":>11}')
    for k in range(b.atoms.shape[0]):
        print(f'{k:5d} {b.atoms_charge[k]:12.6f} {b.voronoi_charge[k]:12.6f} {b.isa_charge[k]:12.6f} {b.mbis_charge[k]:12.6f} {b.mbis_volume[k]:11.5f}')
    print(f'{"sum":>5} {b.atoms_charge.sum():12.6f} {b.voronoi_charge.sum():12.6f} {b.isa_charge.sum():12.6f} {b.mbis_charge.sum():12.6f}'
          f'   (beyond every atom\'s r_cut: charge {b.mbis_rest[0]:.3e} in a volume of {b.mbis_rest[1]:.3f})')
    lost = mbis.tail(b.mbis_populations, b.mbis_widths, np.broadcast_to(a.r_cut, (b.atoms.shape[0],)))
    print('the fitted shells (population, width in the lattice\'s length unit) and the share of the model beyond r_cut:')
    for k in range(b.atoms.shape[0]):
        shells = ', '.join(f'({n:.5f}, {s:.5f})' for n, s in zip(b.mbis_populations[k], b.mbis_widths[k]) if n > 0)
        print(f'{k:5d} {shells}   tail {lost[k]:.2e}')


if __name__ == '__main__':
    main()

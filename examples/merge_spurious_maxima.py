#!/usr/bin/env python3
"""Merging the spurious maxima of a noisy density:

    python examples/merge_spurious_maxima.py [--size 48] [--noise 2e-3] [--tol 4e-3]

A synthetic 8-atom cell (pybader_amd.synth) gets seeded uniform noise of amplitude --noise in its vacuum, where the density is
flat enough for every ripple to be a maximum of its own.  The default neargrid run is made twice, without and with
Bader(persistence_tol=--tol): the second merges every Bader volume whose maximum stands less than --tol above its highest
saddle towards a higher volume (pybader_amd.merge) before anything is summed.  Printed: the maxima before and after, the
rounds the merge took, and the charge per atom of both runs."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import synth                   # noqa: E402
from pybader_amd.interface import Bader         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=48)
    ap.add_argument('--noise', type=float, default=2e-3)
    ap.add_argument('--tol', type=float, default=4e-3)
    a = ap.parse_args()
    shape, lat = (a.size,) * 3, synth.CUBIC6
    rho = synth.synth_density(shape, lat)
    rho = rho + np.where(rho < 0.2, a.noise * np.random.default_rng(11).random(shape), 0.0)
    atoms = synth.atoms_cartesian(synth.ATOMS8, lat)
    before = Bader({'charge': rho.copy()}, lat, atoms)
    before()
    after = Bader({'charge': rho.copy()}, lat, atoms, persistence_tol=a.tol)
    after()
    m = after.bader_merge
    print(f'grid {shape}, noise {a.noise:g} in the vacuum, persistence_tol {a.tol:g}')
    print(f'maxima: {before.bader_maxima.shape[0]} before, {after.bader_maxima.shape[0]} after '
          f'({m.rounds} rounds, {"converged" if m.converged else "stopped by max_rounds"})')
    merged = m.merge_round >= 0
    if merged.any():
        print(f'largest persistence merged: {m.merge_persistence[merged].max():.3e}; '
              f'smallest kept: {m.merge_persistence[~merged].min():.3e}')
    print(f'{"atom":>5} {"charge before":>16} {"charge after":>16} {"difference":>12}')
    for i, (x, y) in enumerate(zip(before.atoms_charge, after.atoms_charge)):
        print(f'{i:5d} {x:16.8f} {y:16.8f} {y - x:12.3e}')
    print(f'{"sum":>5} {before.atoms_charge.sum():16.8f} {after.atoms_charge.sum():16.8f}')


if __name__ == '__main__':
    main()

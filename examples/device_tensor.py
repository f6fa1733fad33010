#!/usr/bin/env python3
"""A density that lives on the GPU as a torch tensor -> per-atom Bader charges and a label tensor, without a trip
through host memory.

    python examples/device_tensor.py [--size 128] [--float32] [--permuted]

The tensor here is a synthetic density built by torch on its own stream (a sum of Gaussians on a cubic cell) -- in
real use it is whatever a model or a PyTorch / CuPy pipeline left on the card.  It goes into
pybader_amd.interface.Bader as it is (float32 or float64, any strides); the atom map comes back as a device array
that torch wraps without a copy.  No synchronize() is needed on either side: the library orders its work against the
stream named with device.on_stream."""
import argparse
import os
import sys
import time

import numpy as np
import torch          # before pybader_amd loads its library: both then share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gaussians(n, lattice, atoms_frac, dtype, dev):
    """sum of periodic Gaussians on an n^3 grid, computed by torch on the current stream"""
    axis = torch.arange(n, device=dev, dtype=torch.float64) / n
    rho = torch.full((n, n, n), 1e-3, device=dev, dtype=torch.float64)
    cell = float(lattice[0, 0])
    for a in atoms_frac:
        d = [((axis - float(c) + 0.5) % 1.0 - 0.5) * cell for c in a]
        r2 = d[0][:, None, None] ** 2 + d[1][None, :, None] ** 2 + d[2][None, None, :] ** 2
        rho += torch.exp(-r2 / 0.5)
    return rho.to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--float32', action='store_true')
    ap.add_argument('--permuted', action='store_true', help='hand the tensor in with its axes permuted (z slowest)')
    args = ap.parse_args()
    from pybader_amd import device, thread_handlers
    from pybader_amd.interface import Bader
    thread_handlers.VERBOSE = False
    dev = 'cuda:0'
    lattice = np.eye(3) * 6.0
    atoms_frac = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.25], [0.75, 0.25, 0.75], [0.25, 0.75, 0.75]])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), device.on_stream(stream.cuda_stream):
        rho = gaussians(args.size, lattice, atoms_frac, torch.float32 if args.float32 else torch.float64, dev)
        if args.permuted:
            rho = rho.permute(2, 1, 0).contiguous().permute(2, 1, 0)      # same values, z is now the slowest axis in memory
        t0 = time.perf_counter()
        b = Bader({'charge': rho}, lattice, atoms_frac @ lattice)
        b()                                                               # no synchronize: ordered behind the producer
        atom_map = torch.as_tensor(b.atoms_volumes, device=dev)           # zero-copy view of the library's result
        voxels_per_atom = torch.bincount(atom_map.flatten().to(torch.int64), minlength=len(atoms_frac))
        counts = voxels_per_atom.cpu().numpy()
        ms = 1e3 * (time.perf_counter() - t0)
    print(f'{tuple(rho.shape)} {rho.dtype} strides {rho.stride()}: {b.bader_maxima.shape[0]} Bader maxima, {ms:.1f} ms')
    print(f'atom map: {type(b.atoms_volumes).__name__} {b.atoms_volumes.dtype} at 0x{b.atoms_volumes.ptr:x}, '
          f'torch view shares it: {atom_map.data_ptr() == b.atoms_volumes.ptr}')
    for i, (q, v, c) in enumerate(zip(b.atoms_charge, b.atoms_volume, counts)):
        print(f'  atom {i}: charge {q:10.6f}  volume {v:9.4f} = {v / b.voxel_volume:.0f} voxels (torch counts {int(c)} on the map)')


if __name__ == '__main__':
    main()

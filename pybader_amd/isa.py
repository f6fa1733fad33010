"""Iterative stockholder atoms (ISA; Lillestolen & Wheatley 2008): Hirshfeld charges WITHOUT pro-atoms -- no counterpart in the
reference.  Each atom's weight function is the spherical average of that atom's own share of the density, iterated to
self-consistency; nothing but the density file is needed, and the arbitrariness of the promolecule is gone.

    isa_charges(density, lattice, atoms, voxel_volume, r_cut=3.0, shells=None, tol=1e-6, ...)   -> IsaResult
    isa_promolecule(density, lattice, atoms, result)      -> the field sum_a w_a of the converged atoms
    isa_residual(density, lattice, atoms, result)         -> rho - sum_a w_a, the non-spherical residual

The iteration runs in libbader_hip.so (xb_isa_setup, xb_isa_iterate, csrc/k_isa.h) on the Hirshfeld setup of the context
(pybader_amd.hirshfeld): the tables are piecewise constant on K shells uniform in r^2, the shell sums are 64-bit integers, so every
iterate is bit-defined (include/bader_hip.h; tests/test_isa_cpu.py restates it in numpy).  The final charges
are one xb_hirshfeld_sum on the converged tables."""
import math

import numpy as np

from . import _lib, device
from .utils import ensure_density


class IsaResult:
    """charge, volume f64[n]; rest f64[2] (charge and volume of the voxels no atom reaches); stats (of the final sum, and 'e',
    'cmax', 'pairs', 'empty_shells' of the setup); iterations; converged; history f64[iterations, n] (every iteration's
    fixed-point charges, in the density's charge units); tables f64[n, K]; counts i64[n, K]; r_cut f64[n]"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def default_shells(lattice, shape, r_cut):
    """clamp(floor((min r_cut / (2 h_max))^2), 8, 4096), h_max the longest voxel edge: the innermost shell is about two voxels in
    radius"""
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    h_max = max(float(np.linalg.norm(lat[i])) / int(shape[i]) for i in range(3))
    return int(min(max(math.floor((float(np.min(r_cut)) / (2.0 * h_max)) ** 2), 8), 4096))


def _context(density):
    ctx = _lib.default_context()
    shape = tuple(int(s) for s in density.shape)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    return ctx


def _rho_bound(ctx, density):
    """max |rho|: numpy for a host density, the library's reduction for one on the device (already resident)"""
    if device.is_device_array(density):
        return ctx.density_absmax()
    return float(np.max(np.abs(density)))


def isa_charges(density, lattice, atoms, voxel_volume, r_cut=3.0, shells=None, tol=1e-6, max_iter=2000, check_every=16, initial=None,
                direct=False, full_search=False):
    """ISA charge and volume of every atom.

    density      host array, or a float32 / float64 device array
    lattice      the CELL's lattice, one row per axis
    atoms        [n, 3] Cartesian, already `atoms - voxel_offset`; taken as given, not wrapped
    r_cut        a number or one per atom: where an atom's weight ends
    shells       K; None: default_shells()
    tol          the caller's convergence threshold on max_a |charge_a(i) - charge_a(i - 1)| between consecutive iterations, in the
                 density's charge units -- a setting, not a measured number
    max_iter     the most iterations; check_every: how many run per library call (one host wait each)
    initial      None (all ones) or f64[n, K], the starting tables
    direct, full_search   the second implementations of the shell pass and of the tile search: the same bits

    -> IsaResult.  The iteration stops AT the first iteration whose change is below tol: when the library's last call ran on past
    it, the tables from before that call are loaded again and exactly the iterations up to it are repeated (the tables are the
    whole state, so these are the same bits)."""
    ctx = _context(density)
    at = np.ascontiguousarray(atoms, dtype=np.float64).reshape(-1, 3)
    n = at.shape[0]
    rc = np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (n,)).copy()
    K = default_shells(lattice, density.shape, rc) if shells is None else int(shells)
    every = max(1, min(int(check_every), _lib.XB_ISA_ITERS_MAX))
    ensure_density(ctx, density)
    bound = _rho_bound(ctx, density)
    if not bound > 0:
        raise ValueError('isa_charges: the density is zero everywhere (or not finite)')
    info = ctx.isa_setup(lattice, at, rc, K, bound, initial)
    scale = math.ldexp(1.0, -info['e']) * float(voxel_volume)
    rows, last, converged = [], None, False
    while len(rows) < int(max_iter) and not converged:
        m = min(every, int(max_iter) - len(rows))
        before = ctx.isa_tables()[0] if m > 1 else None
        q, _ = ctx.isa_iterate(m, direct, full_search)
        for j, row in enumerate(q.astype(np.float64) * scale):
            rows.append(row)
            if last is not None and np.max(np.abs(row - last)) < tol:
                converged = True
                if j + 1 < m:
                    ctx.isa_load(before)
                    ctx.isa_iterate(j + 1, direct, full_search)
                break
            last = row
    charge, volume, rest, stats = ctx.hirshfeld_sum(voxel_volume, full_search)
    tables, counts = ctx.isa_tables()
    stats = dict(stats, **info)
    return IsaResult(charge=charge, volume=volume, rest=rest, stats=stats, iterations=len(rows), converged=bool(converged),
                     history=np.array(rows).reshape(len(rows), n), tables=tables, counts=counts, r_cut=rc, shells=K, rho_bound=bound)


def _field(density, lattice, atoms, result, mode, full_search):
    ctx = _context(density)
    ctx.isa_setup(lattice, atoms, result.r_cut, result.shells, result.rho_bound, result.tables)
    if mode == _lib.XB_HIRSHFELD_DEFORMATION:
        ensure_density(ctx, density)
    return ctx.hirshfeld_field(mode, full_search, on_device=device.is_device_array(density))


def isa_promolecule(density, lattice, atoms, result, full_search=False):
    """sum_a w_a of the converged atoms of `result` (an IsaResult) on the grid of `density`, which gives the shape and the kind of
    the result only: a host array for a host density, a device.DeviceArray for a device one (xb_hirshfeld_field)."""
    return _field(density, lattice, atoms, result, _lib.XB_HIRSHFELD_PROMOLECULE, full_search)


def isa_residual(density, lattice, atoms, result, full_search=False):
    """rho - sum_a w_a: what the spherical atoms of `result` cannot hold, ISA's own quality figure (xb_hirshfeld_field)."""
    return _field(density, lattice, atoms, result, _lib.XB_HIRSHFELD_DEFORMATION, full_search)

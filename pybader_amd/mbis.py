"""Minimal-basis iterative stockholder atoms (MBIS; Verstraelen, Vandenbrande, Heidar-Zadeh, Vanduyfhuys, Van Speybroeck, Waroquier
and Ayers, JCTC 2016): iterative Hirshfeld charges whose pro-atoms are sums of a few Slater shells
N_ai / (8 pi sigma_ai^3) exp(-r / sigma_ai) -- no counterpart in the reference.  An atom has 2 to 16 numbers of state instead of
ISA's table of shell averages (pybader_amd.isa), and the fit converges in tens of iterations where ISA needs hundreds.

    mbis_charges(density, lattice, atoms, voxel_volume, shells=1, r_cut=5.0, tol=1e-6, ...)   -> MbisResult
    initial_from_numbers(Z)                                -> (shells, N, sigma): the paper's hydrogenic start for all-electron densities
    mbis_promolecule(density, lattice, atoms, result)      -> the field sum_a rho0_a of the converged atoms
    mbis_residual(density, lattice, atoms, result)         -> rho - sum_a rho0_a

The iteration runs in libbader_hip.so (xb_mbis_setup, xb_mbis_iterate, csrc/k_mbis.h) on the geometry of the context's Hirshfeld
setup.  The device evaluates no exp: it interpolates the one table exp_table() builds here with numpy, and all sums are 64-bit
integers, so every iterate is bit-defined (include/bader_hip.h; tests/test_mbis_cpu.py restates it in numpy).
The charges are the last iteration's own sums: no extra pass.

THE CUTOFF TRUNCATES EXPONENTIALS.  A shell of width sigma keeps the share 1 - e^-x (1 + x + x^2/2), x = r_cut / sigma, of its
population inside r_cut; MbisResult.tail reports what the fitted model loses, and mbis_charges warns above 1e-3."""
import math
import warnings

import numpy as np

from . import _lib, device
from .isa import _context, _rho_bound
from .utils import ensure_density

BOHR = 0.529177210903   # Angstrom
_PERIOD_ENDS = (2, 10, 18, 36, 54, 86, 118)
_PERIOD_POPULATIONS = (2.0, 8.0, 8.0, 18.0, 18.0, 32.0, 32.0)


class MbisResult:
    """charge, volume f64[n]; rest f64[2] (charge and volume of the voxels no atom reaches); populations, widths f64[n, M] (M the
    largest shell count; entries beyond an atom's own shells are 0 and 1); shells int[n]; iterations; converged; history
    f64[iterations, n] (every iteration's charges); tail f64[n] (the share of the model's population beyond r_cut); stats (the
    routes of the last call and 'eN', 'eS', 'eV', 'eR', 'cmax', 'pairs' of the setup); r_cut, rho_bound, knots_per_unit, x_max,
    voxel_volume as used"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def exp_table(knots_per_unit=256, x_max=48):
    """E[k] = exp(-k / J) for k = 0 .. KE - 1, KE = x_max * J, and E[KE] = 0.0 exactly -> f64[KE + 1] (192 KiB by default)"""
    J, KE = int(knots_per_unit), int(x_max) * int(knots_per_unit)
    E = np.zeros(KE + 1)
    E[:KE] = np.exp(-(np.arange(KE, dtype=np.float64) / np.float64(J)))
    return E


def default_initial(shells):
    """N_ai = 1 / m_a, sigma_ai = 0.2 A * 2^i -- a setting -> (N f64[n, M], sigma f64[n, M])"""
    sh = np.asarray(shells, dtype=np.int64).reshape(-1)
    M = int(sh.max())
    N, sg = np.zeros((sh.size, M)), np.ones((sh.size, M))
    for a, m in enumerate(sh):
        N[a, :m] = 1.0 / m
        sg[a, :m] = 0.2 * 2.0 ** np.arange(m)
    return N, sg


def initial_from_numbers(Z):
    """The paper's hydrogenic start for ALL-ELECTRON densities: one shell per period up to the atom's own, the populations
    2, 8, 8, 18, 18, 32, 32 rescaled to sum to Z, the exponents 1 / sigma running geometrically from 2 Z (innermost) to 2 (outermost)
    in bohr^-1 (a single shell: 2 Z), converted to Angstrom -> (shells int[n], N f64[n, M], sigma f64[n, M])"""
    Z = np.asarray(Z, dtype=np.int64).reshape(-1)
    if Z.size == 0 or (Z < 1).any() or (Z > _PERIOD_ENDS[-1]).any():
        raise ValueError('initial_from_numbers: atomic numbers in 1 .. 118 are wanted')
    sh = np.array([next(p + 1 for p, end in enumerate(_PERIOD_ENDS) if z <= end) for z in Z], np.int64)
    M = int(sh.max())
    N, sg = np.zeros((Z.size, M)), np.ones((Z.size, M))
    for a, (z, m) in enumerate(zip(Z, sh)):
        pop = np.array(_PERIOD_POPULATIONS[:m])
        N[a, :m] = pop * (float(z) / pop.sum())
        alpha = np.array([2.0 * z]) if m == 1 else 2.0 * z * (1.0 / z) ** (np.arange(m) / (m - 1.0))
        sg[a, :m] = BOHR / alpha
    return sh, N, sg


def tail(populations, widths, r_cut):
    """per atom the share of the model's population beyond the cutoff: sum_i N_ai e^-x (1 + x + x^2/2) / sum_i N_ai at
    x = r_cut / sigma_ai (the integral of a Slater shell from r_cut on); 0 for an atom without population"""
    N, sg = np.asarray(populations, dtype=np.float64), np.asarray(widths, dtype=np.float64)
    x = np.asarray(r_cut, dtype=np.float64).reshape(-1, 1) / sg
    lost = (N * np.exp(-x) * (1.0 + x + 0.5 * x * x)).sum(axis=1)
    total = N.sum(axis=1)
    return np.divide(lost, total, out=np.zeros_like(lost), where=total > 0)


def _results(info, voxel_volume, qsum, vsum, rest):
    """the last row of a call -> (charge, volume, rest): exact scalings of the integer sums"""
    vv = float(voxel_volume)
    charge = vv * np.ldexp(qsum.astype(np.float64), -info['eN'])
    volume = vv * np.ldexp(vsum.astype(np.float64), -info['eV'])
    return charge, volume, np.array([vv * math.ldexp(float(rest[0]), -info['eR']), vv * float(rest[1])])


def mbis_charges(density, lattice, atoms, voxel_volume, shells=1, r_cut=5.0, tol=1e-6, max_iter=500, check_every=8, initial=None,
                 knots_per_unit=256, x_max=48, direct=False, full_search=False, rho_bound=None):
    """MBIS charge and volume of every atom.

    density      host array, or a float32 / float64 device array
    lattice      the CELL's lattice, one row per axis
    atoms        [n, 3] Cartesian, already `atoms - voxel_offset`; taken as given, not wrapped
    shells       a number or one per atom, 1 .. 8: the Slater shells of an atom
    r_cut        a number or one per atom: where an atom's weight ends (the exponentials are truncated there: see `tail`)
                 A tile of 8^3 voxels that more than 256 atom images reach within r_cut runs over the whole image list instead
                 of its own (stats['full_tiles']): the same bits, far slower -- with a few hundred atoms in reach, lower r_cut
    tol          the caller's convergence threshold on max_a |charge_a(i) - charge_a(i - 1)| between consecutive iterations, in the
                 density's charge units -- a setting, not a measured number
    max_iter     the most iterations; check_every: how many run per library call (one host wait each)
    initial      None (default_initial) or (N, sigma), each f64[n, M]; initial_from_numbers(Z)[1:] for all-electron densities
    knots_per_unit, x_max   the table of exp(-x): J knots per unit of x = r / sigma up to x_max, beyond which a shell is zero
    direct, full_search   the second implementations of the shell pass and of the tile search: the same bits
    rho_bound    None (max |density|) or a larger bound, for a later pass on another density with the same weights

    -> MbisResult.  The iteration stops AT the first iteration whose change is below tol: when the library's last call ran on past
    it, the parameters from before that call are loaded again and exactly the iterations up to it are repeated (the parameters are
    the whole state, so these are the same bits)."""
    ctx = _context(density)
    at = np.ascontiguousarray(atoms, dtype=np.float64).reshape(-1, 3)
    n = at.shape[0]
    rc = np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (n,)).copy()
    sh = np.broadcast_to(np.asarray(shells, dtype=np.int32), (n,)).copy()
    every = max(1, min(int(check_every), _lib.XB_MBIS_ITERS_MAX))
    N0, s0 = default_initial(sh) if initial is None else initial
    ensure_density(ctx, density)
    bound = _rho_bound(ctx, density) if rho_bound is None else float(rho_bound)
    if not bound > 0:
        raise ValueError('mbis_charges: the density is zero everywhere (or not finite)')
    info = ctx.mbis_setup(lattice, at, rc, sh, exp_table(knots_per_unit, x_max), knots_per_unit, N0, s0, bound, voxel_volume)
    rows, last, converged, final, stats = [], None, False, None, {}
    while len(rows) < int(max_iter) and not converged:
        m = min(every, int(max_iter) - len(rows))
        before = ctx.mbis_params()[:2] if m > 1 else None
        q, v, r, stats = ctx.mbis_iterate(m, direct, full_search)
        for j in range(m):
            row = _results(info, voxel_volume, q[j], v[j], r[j])
            rows.append(row[0])
            final = row
            if last is not None and np.max(np.abs(row[0] - last)) < tol:
                converged = True
                if j + 1 < m:
                    ctx.mbis_load(*before)
                    ctx.mbis_iterate(j + 1, direct, full_search)
                break
            last = row[0]
    if final is None:
        raise ValueError('mbis_charges: max_iter below 1')
    N, sg, _ = ctx.mbis_params()
    lost = tail(N, sg, rc)
    if (lost > 1e-3).any():
        warnings.warn(f'mbis_charges: the cutoff truncates up to {lost.max():.2e} of an atom\'s model population (atom {int(lost.argmax())}, '
                      f'r_cut = {rc[int(lost.argmax())]:g}); a larger r_cut recovers it', RuntimeWarning, stacklevel=2)
    return MbisResult(charge=final[0], volume=final[1], rest=final[2], populations=N, widths=sg, shells=sh, iterations=len(rows),
                      converged=bool(converged), history=np.array(rows).reshape(len(rows), n), tail=lost, stats=dict(stats, **info),
                      r_cut=rc, rho_bound=bound, knots_per_unit=int(knots_per_unit), x_max=int(x_max), voxel_volume=float(voxel_volume))


def _field(density, lattice, atoms, result, mode, full_search):
    ctx = _context(density)
    ctx.mbis_setup(lattice, atoms, result.r_cut, result.shells, exp_table(result.knots_per_unit, result.x_max), result.knots_per_unit,
                   result.populations, result.widths, result.rho_bound, result.voxel_volume)
    if mode == _lib.XB_HIRSHFELD_DEFORMATION:
        ensure_density(ctx, density)
    return ctx.mbis_field(mode, full_search, on_device=device.is_device_array(density))


def mbis_promolecule(density, lattice, atoms, result, full_search=False):
    """sum_a rho0_a of the converged atoms of `result` (an MbisResult) on the grid of `density`, which gives the shape and the kind
    of the result only: a host array for a host density, a device.DeviceArray for a device one (xb_mbis_field)."""
    return _field(density, lattice, atoms, result, _lib.XB_HIRSHFELD_PROMOLECULE, full_search)


def mbis_residual(density, lattice, atoms, result, full_search=False):
    """rho - sum_a rho0_a: what the Slater atoms of `result` cannot hold (xb_mbis_field)."""
    return _field(density, lattice, atoms, result, _lib.XB_HIRSHFELD_DEFORMATION, full_search)

"""What comes after a stockholder charge: the dipole, the second moments and the radial moments <r^2>, <r^3>, <r^4> of every atom's
share w_a rho of the density, for the three stockholder partitions of this package -- Hirshfeld (pybader_amd.hirshfeld), ISA
(pybader_amd.isa) and MBIS (pybader_amd.mbis) -- no counterpart in the reference.  multipole.moment_sum gives these for a label map,
that is for hard partitions; a weight several atoms share at a voxel is no label map.

    hirshfeld_moments(density, lattice, atoms, species, proatoms, voxel_volume)   -> StockholderMoments
    isa_moments(density, lattice, atoms, result, voxel_volume)                    -> StockholderMoments   (result: an isa.IsaResult)
    mbis_moments(density, lattice, atoms, result)                                 -> StockholderMoments   (result: an mbis.MbisResult)

One pass over the (voxel, image) pairs in libbader_hip.so (xb_stockholder_moments, csrc/k_stockmom.h) that keeps twelve 64-bit
integer sums per atom, so every result is bit-defined (include/bader_hip.h; tests/test_stockmom_cpu.py restates
it in numpy).  Every image of an atom is its own copy of it: the displacement is the one to that image, not a minimum image.

UNITS AND SIGN are multipole's: the density counts electrons as positive, `dipole` and `quadrupole` are the electronic ones.
<r^3> / <r^3>_free is the Hirshfeld volume ratio that scales C6, polarisability and vdW radius in the Tkatchenko-Scheffler
correction: ProAtoms.radial_moment(3) gives the free atoms' <r^3> of the tables themselves."""
import numpy as np

from . import multipole
from .hirshfeld import _setup
from .isa import _context, _rho_bound
from .utils import ensure_density

ORDER = (0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 4)     # which exponent E_k scales column c


class StockholderMoments:
    """moments f64[n, 12]: columns 0 .. 9 as a row of multipole.moment_sum (m0; m1 x y z; m2 xx xy xz yy yz zz), column 10 the
    integral of w_a rho r^3, column 11 of w_a rho r^4, each times voxel_volume; bins i64[n, 12], the integer sums they are exact
    scalings of; info {'E': (E0 .. E4), 'cmax', 'pairs', 'beyond_bound'}; stats (the routes of the call)"""

    def __init__(self, bins, info, stats, voxel_volume, species=None):
        self.bins, self.info, self.stats, self.voxel_volume = bins, info, stats, float(voxel_volume)
        self.species = np.arange(bins.shape[0]) if species is None else np.asarray(species, dtype=np.int64).reshape(-1)
        self.moments = scale(bins, info['E'], voxel_volume)

    @property
    def charge(self):
        return self.moments[:, 0]

    @property
    def dipole(self):
        """the electronic dipole -m1 [n, 3] (multipole.dipole)"""
        return multipole.dipole(self.moments[:, :10])

    @property
    def second_moment(self):
        """the symmetric matrices m2 [n, 3, 3] (multipole.second_moment)"""
        return multipole.second_moment(self.moments[:, :10])

    @property
    def quadrupole(self):
        """the electronic traceless quadrupole [n, 3, 3] (multipole.quadrupole)"""
        return multipole.quadrupole(self.moments[:, :10])

    @property
    def r2(self):
        """the integral of w_a rho r^2: the trace of the second moments, (xx + yy) + zz"""
        return (self.moments[:, 4] + self.moments[:, 7]) + self.moments[:, 9]

    @property
    def r3(self):
        return self.moments[:, 10]

    @property
    def r4(self):
        return self.moments[:, 11]

    def volume_ratio(self, free_r3):
        """r3 / free_r3[species]: the Hirshfeld volume ratio per atom; `free_r3` per species, e.g. ProAtoms.radial_moment(3)
        (`species` is the Hirshfeld call's; on ISA and MBIS atoms it is 0 .. n - 1: one entry per atom)"""
        free = np.asarray(free_r3, dtype=np.float64).reshape(-1)
        if self.species.size and int(self.species.max()) >= free.shape[0]:
            raise ValueError(f'volume_ratio: {free.shape[0]} free-atom moments, species up to {int(self.species.max())}')
        return self.r3 / free[self.species]


def scale(bins, E, voxel_volume):
    """moments[a][c] = voxel_volume * ldexp((double)bins[a][c], -E_order(c)): exact scalings"""
    b = np.asarray(bins, dtype=np.int64).reshape(-1, 12)
    e = np.array([-int(E[k]) for k in ORDER], dtype=np.int64)
    return float(voxel_volume) * np.ldexp(b.astype(np.float64), e[None, :])


def _moments(ctx, density, voxel_volume, rho_bound, direct, full_search, who, species=None):
    ensure_density(ctx, density)
    bound = _rho_bound(ctx, density) if rho_bound is None else float(rho_bound)
    if not bound > 0:
        raise ValueError(f'{who}: the density is zero everywhere (or not finite)')
    bins, info, stats = ctx.stockholder_moments(bound, direct, full_search)
    return StockholderMoments(bins, info, stats, voxel_volume, species)


def hirshfeld_moments(density, lattice, atoms, species, proatoms, voxel_volume, rho_bound=None, direct=False, full_search=False):
    """The moments of the Hirshfeld atoms (arguments as hirshfeld.hirshfeld_charges; the setup is made again only when they changed).
    rho_bound: None (max |density|) or a larger bound; direct, full_search: the second implementations, the same bits."""
    ctx = _setup(density, lattice, atoms, species, proatoms)
    return _moments(ctx, density, voxel_volume, rho_bound, direct, full_search, 'hirshfeld_moments', species)


def isa_moments(density, lattice, atoms, result, voxel_volume, rho_bound=None, direct=False, full_search=False):
    """The moments of the converged ISA atoms of `result` (an isa.IsaResult): its setup is built again from the result's tables."""
    ctx = _context(density)
    ctx.isa_setup(lattice, atoms, result.r_cut, result.shells, result.rho_bound, result.tables)
    return _moments(ctx, density, voxel_volume, rho_bound, direct, full_search, 'isa_moments')


def mbis_moments(density, lattice, atoms, result, rho_bound=None, direct=False, full_search=False):
    """The moments of the converged MBIS atoms of `result` (an mbis.MbisResult): its setup is built again from the result's shells;
    the voxel volume is the result's."""
    from .mbis import exp_table
    ctx = _context(density)
    ctx.mbis_setup(lattice, atoms, result.r_cut, result.shells, exp_table(result.knots_per_unit, result.x_max), result.knots_per_unit,
                   result.populations, result.widths, result.rho_bound, result.voxel_volume)
    return _moments(ctx, density, result.voxel_volume, rho_bound, direct, full_search, 'mbis_moments')

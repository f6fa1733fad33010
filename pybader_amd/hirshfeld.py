"""Hirshfeld (stockholder) charges, the promolecular density and the deformation density -- no counterpart in the reference.
Every voxel's density is shared among the atoms in proportion to what each FREE atom would put there,
w_a(r) = rho0_a(|r - R_a|) / sum_b rho0_b(|r - R_b|): no surfaces, no maxima, no sensitivity to noise, which is why the charge
is printed beside the Bader one as a cross-check.  The promolecular density sum_b rho0_b it needs also gives the deformation
density rho - rho_pro, the field a QTAIM user plots next to the Laplacian.

    ProAtoms(tables, r_cut) / ProAtoms.from_radial / ProAtoms.from_density              the free atoms
    hirshfeld_charges(density, lattice, atoms, species, proatoms, voxel_volume)         -> (charge, volume, rest, stats)
    promolecule(density, lattice, atoms, species, proatoms)                             -> the field P
    deformation_density(density, lattice, atoms, species, proatoms)                     -> the field rho - P

The weights run in libbader_hip.so (xb_hirshfeld_setup, xb_hirshfeld_sum, xb_hirshfeld_field, csrc/k_hirshfeld.h); the definition
-- tables uniform in r^2, the canonical image list, the running sums -- is in include/bader_hip.h and DESIGN.md section 19, and
tests/test_hirshfeld_cpu.py restates it in numpy.  Every value at a voxel is bit-defined; the sums per atom are float atomics in
any order.  No free-atom data is shipped: the pro-atoms are the caller's."""
import numpy as np

from . import _lib, device
from .utils import ensure_density


class ProAtoms:
    """The free atoms: `tables` f64[S, K + 1], row s the density of species s at r^2 = k * r_cut[s]^2 / K, finite, >= 0, the last
    column exactly 0; `r_cut` f64[S] > 0.

    WHAT THE r^2 SPACING RESOLVES.  Knot k sits at r_k = r_cut sqrt(k / K): the knots are dense at the cutoff (spacing
    r_cut / (2 K) there) and coarse at the nucleus -- the first interval ends at r_cut / sqrt(K), 0.047 A for r_cut = 3 A and
    K = 4096, and a quarter of all knots lie beyond r_cut sqrt(3) / 2.  The interpolant is linear in r^2, so a profile that is
    smooth in r^2 (a Gaussian, a valence pseudo-density, which is flat at the nucleus) is resolved well everywhere.  An
    all-electron density has a cusp, rho ~ exp(-2 Z r): linear in r, not in r^2, and it falls by a large factor inside the first
    interval, which the table renders as one straight piece in r^2.  The spacing is fine for valence pseudo-densities and
    coarse for an all-electron cusp; the voxel grid does not resolve that cusp either."""

    def __init__(self, tables, r_cut):
        self.tables = np.ascontiguousarray(tables, dtype=np.float64)
        self.r_cut = np.ascontiguousarray(r_cut, dtype=np.float64).reshape(-1)
        if self.tables.ndim != 2 or self.tables.shape[1] < 2 or self.tables.shape[0] != self.r_cut.shape[0]:
            raise ValueError(f'ProAtoms: tables of shape {self.tables.shape} and {self.r_cut.shape[0]} cutoffs; [S, K + 1] with K >= 1 and [S] are wanted')

    @property
    def n_species(self):
        return self.tables.shape[0]

    @property
    def knots(self):
        return self.tables.shape[1] - 1

    @staticmethod
    def knot_radii(r_cut, knots):
        """the radii of the K + 1 knots of one species: sqrt(k * r_cut^2 / K)"""
        return np.sqrt(np.arange(knots + 1, dtype=np.float64) * (float(r_cut) * float(r_cut)) / np.float64(knots))

    @classmethod
    def from_radial(cls, profiles, r_cut, knots=4096):
        """Resample radial profiles onto the r^2-uniform knots: `profiles` a list of (r, rho_r) per species (r ascending),
        `r_cut` a number or one per species.  numpy.interp at the knots' radii (the first and last values of a profile hold outside
        its range), negative values clipped to 0, the last knot set to 0."""
        rc = np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (len(profiles),)).copy()
        tab = np.zeros((len(profiles), int(knots) + 1))
        for s, (r, rho_r) in enumerate(profiles):
            tab[s] = np.interp(cls.knot_radii(rc[s], int(knots)), np.asarray(r, dtype=np.float64), np.asarray(rho_r, dtype=np.float64))
        np.maximum(tab, 0.0, out=tab)
        tab[:, -1] = 0.0
        return cls(tab, rc)

    @classmethod
    def from_density(cls, density, lattice, centre, r_cut, knots=4096):
        """One species from a free atom computed in a box (how VASP users get pro-atoms): the spherical average of `density`
        (host array, the cell `lattice`, a row per axis) about the Cartesian point `centre`, over the nearest periodic image of
        every voxel.  The voxels are binned in r^2 around each knot (bin k: |r^2 / h2 - k| < 1/2); a bin without a voxel is filled by
        numpy.interp from its neighbours.  The box must hold the sphere of r_cut; the last knot is set to 0."""
        rho = np.asarray(density, dtype=np.float64)
        lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
        frac = np.stack(np.meshgrid(*(np.arange(n) / n for n in rho.shape), indexing='ij'), -1).reshape(-1, 3)
        d = frac - np.linalg.solve(lat.T, np.asarray(centre, dtype=np.float64))
        d -= np.rint(d)
        r2 = ((d @ lat) ** 2).sum(axis=1)
        h2 = float(r_cut) ** 2 / int(knots)
        k = np.rint(r2 / h2).astype(np.int64)
        inside = k <= knots
        total = np.bincount(k[inside], weights=rho.reshape(-1)[inside], minlength=knots + 1)
        count = np.bincount(k[inside], minlength=knots + 1)
        have = count > 0
        if not have.any():
            raise ValueError('ProAtoms.from_density: no voxel within r_cut of the centre')
        idx = np.arange(knots + 1)
        tab = np.interp(idx, idx[have], total[have] / count[have])
        np.maximum(tab, 0.0, out=tab)
        tab[-1] = 0.0
        return cls(tab[None, :], [float(r_cut)])

    def radial_moment(self, k):
        """4 pi * the integral of rho0 r^(k + 2) dr from 0 to r_cut, per species -> f64[S]; k = 0 is the population, k = 3 the free
        atom's <r^3> of the Hirshfeld volume ratio.  The closed form for the table's OWN interpolant, which is piecewise linear in
        x = r^2: with p = (k + 1) / 2 and r^(k + 2) dr = x^p dx / 2, segment j (x_j .. x_j+1, slope b_j = (f_j+1 - f_j) / h2) gives
          2 pi * [ f_j * A_j + b_j * (B_j - x_j * A_j) ],   A_j = (x_j+1^(p+1) - x_j^(p+1)) / (p + 1),  B_j = (x_j+1^(p+2) - x_j^(p+2)) / (p + 2)
        k > -3 (the integrand is integrable at the nucleus)."""
        p = (float(k) + 1.0) / 2.0
        if not p + 1.0 > 0.0:
            raise ValueError(f'ProAtoms.radial_moment: k = {k}; k > -3 is wanted')
        K = self.knots
        out = np.zeros(self.n_species)
        for s in range(self.n_species):
            h2 = self.r_cut[s] * self.r_cut[s] / np.float64(K)
            x = np.arange(K + 1, dtype=np.float64) * h2
            f = self.tables[s]
            A = np.diff(x ** (p + 1.0)) / (p + 1.0)
            B = np.diff(x ** (p + 2.0)) / (p + 2.0)
            b = np.diff(f) / h2
            out[s] = 2.0 * np.pi * float(np.sum(f[:-1] * A + b * (B - x[:-1] * A)))
        return out

    def joined(self, other):
        """the species of self followed by those of `other` (the same number of knots)"""
        return ProAtoms(np.concatenate([self.tables, other.tables]), np.concatenate([self.r_cut, other.r_cut]))


def _setup(density, lattice, atoms, species, proatoms):
    """the default context on the grid of `density` with the library's setup made from these arguments -- made again only when
    one of them changed (a sum on the spin density after the one on the charge reuses it)"""
    ctx = _lib.default_context()
    shape = tuple(int(s) for s in density.shape)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    lat = np.ascontiguousarray(lattice, dtype=np.float64).reshape(9)
    at = np.ascontiguousarray(atoms, dtype=np.float64).reshape(-1, 3)
    sp = np.ascontiguousarray(species, dtype=np.int32).reshape(-1)
    key = (shape, lat.tobytes(), at.tobytes(), sp.tobytes(), proatoms.tables.tobytes(), proatoms.r_cut.tobytes(), proatoms.tables.shape)
    if ctx.hirshfeld_key != key:
        ctx.hirshfeld_key = None
        ctx.hirshfeld_setup(lat, at, sp, proatoms.tables, proatoms.r_cut)
        ctx.hirshfeld_key = key
    return ctx


def hirshfeld_charges(density, lattice, atoms, species, proatoms, voxel_volume, full_search=False):
    """Hirshfeld charge and volume of every atom.

    density      host array, or a float32 / float64 device array
    lattice      the CELL's lattice, one row per axis
    atoms        [n, 3] Cartesian, already `atoms - voxel_offset`; taken as given, not wrapped
    species      int[n], the row of `proatoms` each atom takes
    proatoms     a ProAtoms
    full_search  every tile of voxels runs over the whole image list instead of its candidate list: the second implementation

    -> (charge f64[n], volume f64[n], rest f64[2], stats): rest = charge and volume of the voxels no pro-atom reaches (they belong
    to nobody; sum(charge) + rest[0] is the integral of the density), stats = {'candidate_tiles', 'full_tiles', 'max_candidates'}."""
    ctx = _setup(density, lattice, atoms, species, proatoms)
    ensure_density(ctx, density)
    return ctx.hirshfeld_sum(voxel_volume, full_search)


def promolecule(density, lattice, atoms, species, proatoms, full_search=False):
    """The promolecular density P = the sum of the free atoms on the grid of `density`, which gives the shape and the kind of the
    result only (it is neither read nor uploaded): a host array for a host density, a device.DeviceArray for a device one."""
    ctx = _setup(density, lattice, atoms, species, proatoms)
    return ctx.hirshfeld_field(_lib.XB_HIRSHFELD_PROMOLECULE, full_search, on_device=device.is_device_array(density))


def deformation_density(density, lattice, atoms, species, proatoms, full_search=False):
    """The deformation density rho - P of `density` (host array, or a float32 / float64 device array), float64: a host array for
    a host density, a device.DeviceArray for a device one."""
    ctx = _setup(density, lattice, atoms, species, proatoms)
    ensure_density(ctx, density)
    return ctx.hirshfeld_field(_lib.XB_HIRSHFELD_DEFORMATION, full_search, on_device=device.is_device_array(density))

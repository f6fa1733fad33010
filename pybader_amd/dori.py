"""DORI, the density overlap regions indicator of de Silva and Corminboeuf (J. Chem. Theory Comput. 10, 3745 (2014)) -- no
counterpart in the reference.  One field on [0, 1] that shows covalent bonds and non-covalent contacts alike:

    gamma = theta / (1 + theta),    theta = |grad k^2|^2 / (k^2)^3,    k = grad rho / rho

is close to 1 where the densities of two atoms (or molecules) overlap and close to 0 inside a single atom's exponential tail, and
the sign of lambda2, the middle eigenvalue of the Hessian, colours it as in pybader_amd.nci: sign(lambda2) rho strongly negative
in a covalent bond, near zero in a van der Waals contact, positive in a ring or a steric clash.  Multiwfn prints the same.  It
needs rho, its gradient and its Hessian only -- NCI cuts the covalent bonds out (rho < rho_cut), and ELF needs the kinetic-energy
density, which a CHGCAR or a cube of rho does not carry.

It runs in libbader_hip.so (xb_dori_field, xb_dori_sum, csrc/k_dori.h) on the 19-point stencil of pybader_amd.laplacian.  The
definition is in include/bader_hip.h and DESIGN.md section 26, and tests/test_dori_cpu.py restates it in numpy.  With
u = rho H g - |g|^2 g, N = 4 |u|^2 and D = (|g|^2)^3 the indicator is N / (N + D): rho^6 cancels, so gamma is a handful of
multiplications and additions and one division of the ten values of xb_stencil_points -- bit-defined, as dori_value() forms it.

    dori_fields(density, lattice, rho_min)                                           (gamma, x = sign(lambda2) rho)
    dori_regions(density, volumes, lattice, n, voxel_volume, d_cut, rho_min, rho_split)  a DoriRegions
    dori_isosurface(density, lattice, level, rho_min)                                the surface gamma = level, an isosurface.Mesh
    dori_domains(density, lattice, volumes, n, voxel_volume, level, rho_min, rho_split)  the region's connected pieces, a DoriDomains
    bond_dori(density, lattice, lin, rho_min)                                        gamma at listed voxels

Units: gamma is dimensionless.  rho_min and rho_split are in the density's units; the defaults are the usual ones in atomic
units (e / bohr^3).  For a density in e / Angstrom^3 multiply them by E_PER_A3."""
import numpy as np

from . import device
from .laplacian import _PAIRS, _resident
from .nci import CLASSES, E_PER_A3, descartes_sign, invariants  # noqa: F401 -- CLASSES and E_PER_A3 are re-exported
from .nci import RHO_SPLIT as _NCI_RHO_SPLIT
from .regions import Regions
from .utils import ensure_labels

D_CUT = 0.9                  # the region's bound on gamma
RHO_MIN = 1e-3               # the density up to which gamma is 0: the usual molecular envelope, e / bohr^3
RHO_SPLIT = _NCI_RHO_SPLIT   # |sign(lambda2) rho| up to which a voxel of the region counts as van der Waals, e / bohr^3


def _parts(values):
    """(rho, N, S, whether the Hessian is not zero) of the definition from f64[m, 10] rows of xb_stencil_points"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 10)
    c, (g0, g1, g2), (xx, xy, xz, yy, yz, zz) = v[:, 0], v[:, 1:4].T, v[:, 4:].T
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        gg = (g0 * g0 + g1 * g1) + g2 * g2
        h0 = (xx * g0 + xy * g1) + xz * g2
        h1 = (xy * g0 + yy * g1) + yz * g2
        h2 = (xz * g0 + yz * g1) + zz * g2
        u0, u1, u2 = c * h0 - gg * g0, c * h1 - gg * g1, c * h2 - gg * g2
        n = 4.0 * ((u0 * u0 + u1 * u1) + u2 * u2)
        s = n + (gg * gg) * gg
    return c, n, s, (v[:, 4:] != 0).any(axis=1)


def dori_value(values, rho_min=RHO_MIN):
    """gamma of voxels given by their ten values of laplacian / xb_stencil_points (`values` f64[m, 10]: rho, the gradient, the
    Hessian).  The same operations in the same order as the kernels: the same bits as the voxel's entry in dori_fields.
    -> f64[m]"""
    c, n, s, curved = _parts(values)
    ok = (s > 0) & np.isfinite(s)
    with np.errstate(divide='ignore', invalid='ignore', under='ignore'):
        ratio = n / np.where(ok, s, 1.0)
    gamma = np.where(ok, ratio, np.where((s == 0) & curved, 1.0, 0.0))
    return np.where(c > rho_min, gamma, 0.0)


def colour_value(values, rho_min=RHO_MIN):
    """x = sign(lambda2) rho of the same voxels where rho > rho_min, +0 elsewhere -> f64[m]"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 10)
    sigma = descartes_sign(*invariants(v[:, 4:].T))
    with np.errstate(invalid='ignore'):
        return np.where(v[:, 0] > rho_min, sigma.astype(np.float64) * v[:, 0], 0.0)


def point_classes(values, d_cut=D_CUT, rho_min=RHO_MIN, rho_split=RHO_SPLIT):
    """The region's class of the same voxels: -1 outside the region gamma >= d_cut, else 0 attractive, 1 van der Waals,
    2 repulsive: the same answer as the voxel's place in dori_regions.  -> int8[m]"""
    x = colour_value(values, rho_min)
    cls = np.where(x < -rho_split, 0, np.where(x > rho_split, 2, 1))
    return np.where(dori_value(values, rho_min) >= d_cut, cls, -1).astype(np.int8)


def _check_cut(who, d_cut):
    if not 0.0 < float(d_cut) <= 1.0:
        raise ValueError(f'{who}: the bound on gamma must lie in (0, 1]')


def dori_fields(density, lattice, rho_min=RHO_MIN, gather=False, colour=True):
    """(gamma, x): DORI and sign(lambda2) rho of `density` (host array, or a float32 / float64 device array of any strides) in
    the cell `lattice` (a row per axis) at every voxel, float64: host arrays for a host density, device.DeviceArrays for a device
    density.  Where rho is not above `rho_min`, gamma = 0 and x = 0.  Without `colour` x is None and is not computed.  `gather`
    takes the second implementation: the same bits.  Inside utils.resident() nothing is uploaded again."""
    ctx, _ = _resident(density)
    return ctx.dori_field(lattice, rho_min, gather, on_device=device.is_device_array(density), colour=colour)


class DoriRegions:
    """The DORI region (gamma >= d_cut) per label and class (CLASSES: attractive, van der Waals, repulsive):

    count     int64[n, 3]   voxels
    volume    f64[n, 3]     count * voxel_volume
    charge    f64[n, 3]     the integral of rho: the electrons in the overlap region
    charge2   f64[n, 3]     the integral of rho^2
    d_cut, rho_min, rho_split   the thresholds they were made with"""

    def __init__(self, count, charge, charge2, voxel_volume, d_cut, rho_min, rho_split):
        self.count, self.charge, self.charge2 = count, charge, charge2
        self.volume = count.astype(np.float64) * float(voxel_volume)
        self.d_cut, self.rho_min, self.rho_split = float(d_cut), float(rho_min), float(rho_split)


def dori_regions(density, volumes, lattice, n, voxel_volume, d_cut=D_CUT, rho_min=RHO_MIN, rho_split=RHO_SPLIT, gather=False):
    """The DORI region of `density` summed over the voxels of every label 0 .. n - 1 of `volumes` (host or device array; labels
    < 0 and >= n are skipped) and every class.  -> DoriRegions"""
    ctx, shape = _resident(density)
    if tuple(int(s) for s in volumes.shape) != shape:
        raise ValueError(f'dori_regions: the label map has shape {tuple(volumes.shape)}, the density {shape}')
    ensure_labels(ctx, volumes)
    if int(n) < 1:
        return DoriRegions(np.zeros((0, 3), np.int64), np.zeros((0, 3)), np.zeros((0, 3)), voxel_volume, d_cut, rho_min, rho_split)
    count, charge, charge2 = ctx.dori_sum(lattice, n, voxel_volume, d_cut, rho_min, rho_split, gather)
    return DoriRegions(count, charge, charge2, voxel_volume, d_cut, rho_min, rho_split)


def dori_isosurface(density, lattice, level=D_CUT, rho_min=RHO_MIN):
    """The surface gamma = `level` of `density` (host or device array), coloured by sign(lambda2) rho -- the picture of DORI.
    Inside, in the sense of isosurface.Mesh, is gamma >= level: the region of dori_regions and dori_domains.  The two fields are
    made and read on the device, whichever side `density` lives on.  -> isosurface.Mesh"""
    from .isosurface import Mesh
    _check_cut('dori_isosurface', level)
    ctx, shape = _resident(density)
    gamma, x = ctx.dori_field(lattice, rho_min, on_device=True)
    out = ctx.isosurface(lattice, level, gamma, x, 0)
    ctx.isosurface_release()
    return Mesh(shape, level, lattice, *out)


class DoriDomains(Regions):
    """The connected pieces of the DORI region (gamma >= level) under the adjacency of pybader_amd.regions, numbered 0 .. m - 1 in
    ascending seed -- one per bond or contact.  A regions.Regions (labels, seed, voxel, count, volume, top, charge, charge2,
    shares, atoms; top, charge and charge2 are taken of the density) and:

    value      f64[m]        gamma at `top`, the domain's densest voxel
    kind       int8[m]       the class of `top` (point_classes; CLASSES): what the domain is called
    level, rho_min, rho_split   the thresholds they were made with"""

    def __init__(self, regions, value, kind, level, rho_min, rho_split):
        self.__dict__.update(vars(regions))
        self.value, self.kind = value, kind
        self.level, self.rho_min, self.rho_split = float(level), float(rho_min), float(rho_split)


def dori_domains(density, lattice, volumes=None, n=0, voxel_volume=1.0, level=D_CUT, rho_min=RHO_MIN, rho_split=RHO_SPLIT):
    """The DORI region of `density` (host or device array) split into its connected domains, each with its voxels and the integral
    of the density over it; with a label map `volumes` and n >= 1 also which labels 0 .. n - 1 every domain lies between.  gamma is
    made on the device and handed to regions.connected_regions as it is: the pieces are those of the field, the sums and the
    surface.  The labels are a host array for a host density.  -> DoriDomains"""
    from .regions import connected_regions
    _check_cut('dori_domains', level)
    ctx, _ = _resident(density)
    gamma, _ = ctx.dori_field(lattice, rho_min, on_device=True, colour=False)
    r = connected_regions(gamma, level, density=density, voxel_volume=voxel_volume, volumes=volumes, n=n)
    if not device.is_device_array(density):
        r.labels = r.labels.to_host()
    if r.m:
        ten = ctx.stencil_points(lattice, r.top)
        value, kind = dori_value(ten, rho_min), point_classes(ten, level, rho_min, rho_split)
    else:
        value, kind = np.zeros(0), np.zeros(0, np.int8)
    return DoriDomains(r, value, kind, level, rho_min, rho_split)


def bond_dori(density, lattice, lin, rho_min=RHO_MIN):
    """dori_value() at the linear C-order voxel indices `lin` of `density`: the ten values come from the library's gather
    (laplacian.point_properties' call).  -> f64[m]"""
    ctx, _ = _resident(density)
    return dori_value(ctx.stencil_points(lattice, np.asarray(lin, dtype=np.int64).reshape(-1)), rho_min)


assert _PAIRS == ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # the Hessian's component order _parts() relies on

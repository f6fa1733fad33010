"""The NCI index of Johnson et al. (J. Am. Chem. Soc. 132, 6498 (2010)) -- no counterpart in the reference.  Where the
non-covalent interactions of a density are, and of which kind: the reduced density gradient

    s = |grad rho| / (2 (3 pi^2)^(1/3) rho^(4/3))

is small where the density is flat on its own scale -- at the nuclei's tails and between molecules --, and the sign of lambda2, the
middle eigenvalue of the Hessian, tells an attractive contact (hydrogen bond: lambda2 < 0) from a repulsive one (ring closure,
steric clash: lambda2 > 0); |sign(lambda2) rho| near zero is van der Waals.  NCIPLOT, Multiwfn and Critic2 print the same.

It runs in libbader_hip.so (xb_nci_field, xb_nci_sum, xb_nci_hist, csrc/k_nci.h) on the 19-point stencil of
pybader_amd.laplacian.  The definition is in include/bader_hip.h and DESIGN.md section 20, and tests/test_nci_cpu.py restates it
in numpy.  sign(lambda2) comes from Descartes' rule on the Hessian's invariants, not from an eigen-solve; "s < e" is decided by
multiplications and a comparison (thresholds()), so regions, classes and bins are bit-defined; only the field s itself passes
through sqrt and cbrt.

    nci_fields(density, lattice)                                                     (s, x = sign(lambda2) rho)
    nci_regions(density, volumes, lattice, n, voxel_volume, s_cut, rho_cut, rho_split)   an NciRegions
    nci_histogram(density, lattice, s_edges, x_edges)                                int64[n_s, n_x]
    nci_isosurface(density, lattice, s_cut, rho_cut)                                 the surface s = s_cut, an isosurface.Mesh
    nci_domains(density, lattice, volumes, n, voxel_volume, s_cut, rho_cut, rho_split)   the region's connected pieces, an NciDomains

Units: s is dimensionless when density and lattice share a length unit.  rho_cut and rho_split are in the density's units; the
defaults S_CUT, RHO_CUT, RHO_SPLIT are the usual ones in atomic units (e / bohr^3).  For a density in e / Angstrom^3 multiply
them by E_PER_A3."""
import numpy as np

from . import _lib, device
from .laplacian import _PAIRS, _resident
from .utils import ensure_labels

S_CUT = 0.5          # the region's bound on s
RHO_CUT = 0.05       # ... and on rho, e / bohr^3
RHO_SPLIT = 0.01     # |sign(lambda2) rho| up to which a voxel of the region counts as van der Waals, e / bohr^3
E_PER_A3 = 1.0 / 0.529177210903 ** 3    # 1 e / bohr^3 in e / Angstrom^3 (6.748334...): rho_cut_A = RHO_CUT * E_PER_A3
C = _lib.NCI_C       # 2 (3 pi^2)^(1/3), the double of the header's XB_NCI_C
CLASSES = ('attractive', 'van der Waals', 'repulsive')


def thresholds(edges):
    """T(e) of the definition for thresholds `edges` on s: a = C e, a2 = a a, T = (a2 a2) a2, each operation one IEEE float64
    operation.  "s < e" means (g2 g2) g2 < T(e) ((rho rho)^2)^2.  -> f64 of the shape of `edges`"""
    e = np.asarray(edges, dtype=np.float64)
    if not np.isfinite(e).all() or (e < 0).any():
        raise ValueError('thresholds: a threshold on s is finite and not negative')
    a = C * e
    a2 = a * a
    return (a2 * a2) * a2


def invariants(hessian6):
    """(I1, I2, I3) of the symmetric matrices `hessian6` ([6, ...]: xx xy xz yy yz zz), in the definition's order"""
    xx, xy, xz, yy, yz, zz = hessian6
    i1 = (xx + yy) + zz
    i2 = ((xx * yy - xy * xy) + (xx * zz - xz * xz)) + (yy * zz - yz * yz)
    i3 = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)
    return i1, i2, i3


def _sgn(a):
    a = np.asarray(a, dtype=np.float64)
    return (a > 0).astype(np.int64) - (a < 0).astype(np.int64)      # (a NaN counts as a zero)


def descartes_sign(i1, i2, i3):
    """sigma, the sign of the middle root of lambda^3 - I1 lambda^2 + I2 lambda - I3 (all roots real), by Descartes' rule:
    p sign changes in (1, -I1, I2, -I3) with zeros skipped, z trailing zeros, 3 - p - z negative roots.  -> int64"""
    s = [-_sgn(i1), _sgn(i2), -_sgn(i3)]
    p, last = np.zeros(s[0].shape, np.int64), np.ones(s[0].shape, np.int64)
    for t in s:
        p = p + ((t != 0) & (t != last))
        last = np.where(t != 0, t, last)
    z = np.where(s[2] != 0, 0, np.where(s[1] != 0, 1, np.where(s[0] != 0, 2, 3)))
    return np.where(p >= 2, 1, np.where(3 - p - z >= 2, -1, 0)).astype(np.int64)


def point_classes(values, s_cut=S_CUT, rho_cut=RHO_CUT, rho_split=RHO_SPLIT):
    """The region's class of voxels given by their ten values of laplacian / xb_stencil_points (`values` f64[m, 10]: rho, the
    gradient, the Hessian): -1 outside the region, else 0 attractive, 1 van der Waals, 2 repulsive.  The same operations in the
    same order as the kernels: the same answer as the voxel's place in nci_regions.  -> int8[m]"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 10)
    rho, (gx, gy, gz) = v[:, 0], v[:, 1:4].T
    g2 = (gx * gx + gy * gy) + gz * gz
    sigma = descartes_sign(*invariants(v[:, 4:].T))
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        r2 = rho * rho
        r4 = r2 * r2
        inside = (rho > 0) & ((g2 * g2) * g2 < thresholds(s_cut) * (r4 * r4)) & (rho < rho_cut)
    x = sigma.astype(np.float64) * rho
    cls = np.where(x < -rho_split, 0, np.where(x > rho_split, 2, 1))
    return np.where(inside, cls, -1).astype(np.int8)


def nci_fields(density, lattice, gather=False):
    """(s, x): the reduced density gradient and sign(lambda2) rho of `density` (host array, or a float32 / float64 device array
    of any strides) in the cell `lattice` (a row per axis) at every voxel, float64: host arrays for a host density,
    device.DeviceArrays for a device density.  Where rho <= 0, s = +inf and x = 0.  `gather` takes the second implementation:
    the same bits.  Inside utils.resident() nothing is uploaded again."""
    ctx, _ = _resident(density)
    return ctx.nci_field(lattice, gather, on_device=device.is_device_array(density))


class NciRegions:
    """The NCI region (rho > 0, s < s_cut, rho < rho_cut) per label and class (CLASSES: attractive, van der Waals, repulsive):

    count     int64[n, 3]   voxels
    volume    f64[n, 3]     count * voxel_volume
    charge    f64[n, 3]     the integral of rho
    charge2   f64[n, 3]     the integral of rho^2 (NCIPLOT's n = 2 integral)
    s_cut, rho_cut, rho_split   the thresholds they were made with"""

    def __init__(self, count, charge, charge2, voxel_volume, s_cut, rho_cut, rho_split):
        self.count, self.charge, self.charge2 = count, charge, charge2
        self.volume = count.astype(np.float64) * float(voxel_volume)
        self.s_cut, self.rho_cut, self.rho_split = float(s_cut), float(rho_cut), float(rho_split)


def nci_regions(density, volumes, lattice, n, voxel_volume, s_cut=S_CUT, rho_cut=RHO_CUT, rho_split=RHO_SPLIT, gather=False):
    """The NCI region of `density` summed over the voxels of every label 0 .. n - 1 of `volumes` (host or device array; labels
    < 0 and >= n are skipped) and every class.  -> NciRegions"""
    ctx, shape = _resident(density)
    if tuple(int(s) for s in volumes.shape) != shape:
        raise ValueError(f'nci_regions: the label map has shape {tuple(volumes.shape)}, the density {shape}')
    ensure_labels(ctx, volumes)
    if int(n) < 1:
        return NciRegions(np.zeros((0, 3), np.int64), np.zeros((0, 3)), np.zeros((0, 3)), voxel_volume, s_cut, rho_cut, rho_split)
    count, charge, charge2 = ctx.nci_sum(lattice, n, voxel_volume, s_cut, rho_cut, rho_split, gather)
    return NciRegions(count, charge, charge2, voxel_volume, s_cut, rho_cut, rho_split)


def nci_histogram(density, lattice, s_edges, x_edges, gather=False):
    """The voxels of `density` with rho > 0 counted over the bins of s (edges `s_edges`, n_s + 1 of them, not negative) and of
    sign(lambda2) rho (`x_edges`, n_x + 1), both finite and strictly increasing.  A voxel lies in the bin whose lower edge is
    <= its value and whose upper edge is above it, s decided through thresholds(); outside the edges it is not counted.
    -> int64[n_s, n_x], exact"""
    ctx, _ = _resident(density)
    return ctx.nci_hist(lattice, s_edges, x_edges, gather)


def nci_isosurface(density, lattice, s_cut=S_CUT, rho_cut=RHO_CUT, gather=False):
    """The surface s = `s_cut` of the reduced gradient of `density` (host or device array), coloured by sign(lambda2) rho -- the
    picture of the NCI index.  As NCIPLOT does, s is first raised to _lib.ISO_NCI_RAISED wherever rho >= `rho_cut` (and where it
    is not below that value: the +inf of a voxel without density), so only the low-density surfaces remain.  Inside, in the sense
    of isosurface.Mesh, is s >= s_cut: the normals point into the NCI region and `volume` is what lies outside it.  The two
    fields are made, masked and read on the device, whichever side `density` lives on.  -> isosurface.Mesh"""
    from .isosurface import Mesh
    if not 0.0 <= float(s_cut) < _lib.ISO_NCI_RAISED:
        raise ValueError(f'nci_isosurface: s_cut must lie in [0, {_lib.ISO_NCI_RAISED})')
    ctx, shape = _resident(density)
    s, x = ctx.nci_field(lattice, gather, on_device=True)
    ctx.isosurface_nci_mask(s, rho_cut)
    out = ctx.isosurface(lattice, s_cut, s, x, 0, gather)
    ctx.isosurface_release()
    return Mesh(shape, s_cut, lattice, *out)


class NciDomains:
    """The connected pieces of the NCI region (rho > 0, s < s_cut, rho < rho_cut) under the adjacency of pybader_amd.regions,
    numbered 0 .. m - 1 in ascending seed -- one per contact:

    shape, m
    labels     int32 of the grid's shape: the domain of every voxel, -1 outside the region (host array or device.DeviceArray,
               as the density)
    seed       int64[m]      the smallest linear C-order index of the domain;  voxel int64[m, 3]: the same as grid coordinates
    count      int64[m, 3]   voxels per class (CLASSES: attractive, van der Waals, repulsive)
    volume     f64[m, 3]     count * voxel_volume
    charge     f64[m, 3]     the integral of rho per class;  charge2 f64[m, 3]: of rho^2
    size       int64[m]      voxels in all;  total f64[m], total2 f64[m]: the integrals of rho and rho^2 over the whole domain
    top        int64[m]      the domain's greatest voxel of rho in the order of critical.critical_points
    kind       int8[m]       the class of `top` (point_classes): what the domain is called
    shares     (domain, label, count) triplets against `volumes`;  atoms int64[m, 2]: the two labels with the largest counts
    s_cut, rho_cut, rho_split   the thresholds they were made with"""

    def __init__(self, shape, labels, seed, size, top, total, total2, count, charge, charge2, kind, shares, voxel_volume, s_cut, rho_cut,
                 rho_split):
        from .regions import atoms_from_shares
        self.shape, self.m = tuple(int(s) for s in shape), int(seed.shape[0])
        self.labels, self.seed, self.size, self.top, self.total, self.total2 = labels, seed, size, top, total, total2
        self.count, self.charge, self.charge2, self.kind, self.shares = count, charge, charge2, kind, shares
        self.voxel = np.stack(np.unravel_index(seed, self.shape), axis=1).astype(np.int64).reshape(-1, 3)
        self.volume = count.astype(np.float64) * float(voxel_volume)
        self.atoms = atoms_from_shares(self.m, shares)
        self.s_cut, self.rho_cut, self.rho_split = float(s_cut), float(rho_cut), float(rho_split)

    def __len__(self):
        return self.m


def nci_domains(density, lattice, volumes=None, n=0, voxel_volume=1.0, s_cut=S_CUT, rho_cut=RHO_CUT, rho_split=RHO_SPLIT, gather=False,
                global_route=False, shares_list=False):
    """The NCI region of `density` (host or device array) split into its connected domains, each summed per class; with a label
    map `volumes` and n >= 1 also which labels 0 .. n - 1 every domain lies between.  `gather` reads the predicate's stencil from
    global memory, `global_route` runs every union in global memory, `shares_list` counts the shares from a sorted key list: second
    implementations, the same results.  -> NciDomains"""
    from .regions import _shares
    ctx, shape = _resident(density)
    m = ctx.regions_label(_lib.XB_DOMAINS_NCI, None, 0.0, lattice, s_cut, rho_cut, global_route=global_route, gather=gather)
    try:
        labels = ctx.regions_map(on_device=device.is_device_array(density))
        seed, size, top, total, total2, count, charge, charge2 = ctx.regions_sums(m, voxel_volume, rho_split)
        shares = _shares(ctx, shape, volumes, n, shares_list, 'nci_domains')
    finally:
        ctx.regions_release()      # (the map does not outlive the call, whichever way it ends)
    kind = point_classes(ctx.stencil_points(lattice, top), s_cut, rho_cut, rho_split) if m else np.zeros(0, np.int8)
    return NciDomains(shape, labels, seed, size, top, total, total2, count, charge, charge2, kind, shares, voxel_volume, s_cut, rho_cut,
                      rho_split)


def bond_classes(density, lattice, lin, s_cut=S_CUT, rho_cut=RHO_CUT, rho_split=RHO_SPLIT):
    """point_classes() at the linear C-order voxel indices `lin` of `density`: the ten values come from the library's gather
    (laplacian.point_properties' call).  -> int8[m]"""
    ctx, _ = _resident(density)
    return point_classes(ctx.stencil_points(lattice, np.asarray(lin, dtype=np.int64).reshape(-1)), s_cut, rho_cut, rho_split)


assert _PAIRS == ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # the Hessian's component order invariants() relies on

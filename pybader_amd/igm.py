"""IGM, the independent gradient model (Lefebvre et al., Phys. Chem. Chem. Phys. 19, 17928 (2017)) and its Hirshfeld-partitioned
form IGMH (Lu and Chen, J. Comput. Chem. 43, 539 (2022)) -- no counterpart in the reference.  NCI and DORI see one density and
cannot say WHOSE interaction a region is.  IGM compares the norm of the density gradient with the norm it would have if the
atomic gradients could not cancel:

    delta-g       = | sum_a |grad rho_a| |  -  | sum_a grad rho_a |          (component-wise magnitudes in the first sum)
    delta-g_inter = | sum_F |sum_{a in F} grad rho_a| |  -  | sum_a grad rho_a |

delta-g_inter lets only the cancellation BETWEEN user-named fragments count: it is non-zero only where the densities of two
fragments interpenetrate, and its isosurface coloured by sign(lambda2) rho is the picture people publish in place of the NCI one.
delta-g_intra = delta-g - delta-g_inter is the caller's subtraction.

The atomic densities are the table terms of a Hirshfeld setup (pybader_amd.hirshfeld.ProAtoms) or of converged ISA atoms
(pybader_amd.isa.IsaResult): functions of r^2, so their gradients need no square root.  mode 'pro' takes the free atoms' own
gradients (IGM on the promolecule), mode 'stockholder' the gradients of the stockholder shares w_a rho of the actual density
(IGMH).  The gradient of a table is that of its own interpolant, linear in r^2: piecewise constant in slope, as
ProAtoms.radial_moment takes the interpolant at its word.

AN ISA SETUP IS ACCEPTED AND GIVES ZERO FIELDS.  The library keeps ISA tables piecewise CONSTANT on their shells (the pairs are
(A[k], +0.0)), and `isa=` loads them exactly as isa_promolecule does.  Their own gradient is zero, so mode 'pro' gives exact zeros,
and mode 'stockholder' gives grad rho_a = w_a grad rho for every atom: all parallel, nothing cancels, and delta-g and
delta-g_inter vanish up to rounding.  The call is bit-defined and tested, but it is no picture of an interaction.  A user
without pro-atoms who wants one takes the converged shells as knots of an interpolant that is linear in r^2 instead:
ProAtoms(np.c_[result.tables, np.zeros(n)], result.r_cut) with species = arange(n).

It runs in libbader_hip.so (xb_igm_field, xb_igm_sum, csrc/k_igm.h); the definition is in include/bader_hip.h and DESIGN.md
section 27, and tests/test_igm_cpu.py restates it in numpy.  Every value at a voxel is bit-defined.

    igm_fields(density, lattice, atoms, fragments, species, proatoms | isa=...)      (dg, dg_inter, x = sign(lambda2) rho)
    igm_regions(density, volumes, lattice, atoms, fragments, n, voxel_volume, ...)   an IgmRegions
    igm_domains(density, lattice, atoms, fragments, volumes, n, voxel_volume, ...)   the region's connected pieces, an IgmDomains
    igm_isosurface(density, lattice, atoms, fragments, level, ...)                   the surface dg_inter = level, an isosurface.Mesh

Units: delta-g has the units of the density's gradient.  P_MIN, the floor on the promolecular density below which both fields are
0 (it keeps 1 / P finite: near the tables' cutoff P -> 0 while rho does not), is a CHOICE in the density's units, not a measured
number; so is DG_CUT."""
import math

import numpy as np

from . import _lib, device
from .nci import CLASSES, E_PER_A3  # noqa: F401 -- re-exported
from .nci import RHO_SPLIT as _NCI_RHO_SPLIT
from .regions import Regions
from .utils import ensure_density, ensure_labels

MODES = {'pro': _lib.XB_IGM_PRO, 'stockholder': _lib.XB_IGM_STOCKHOLDER}
P_MIN = 1e-6                 # the floor on the promolecular density: a choice, not a measurement
DG_CUT = 0.01                # the region's bound on delta-g_inter: a choice (the isovalue IGMPlot draws weak contacts at, a.u.)
RHO_SPLIT = _NCI_RHO_SPLIT   # |sign(lambda2) rho| up to which a voxel of the region counts as van der Waals, e / bohr^3


def check_fragments(fragments, n_atoms):
    """-> (int32[n], F): every entry in -1 .. F - 1 with F = max + 1 (at least 1) and F <= XB_IGM_FRAGMENTS_MAX"""
    fr = np.asarray(fragments)
    if fr.ndim != 1 or fr.shape[0] != int(n_atoms) or not np.issubdtype(fr.dtype, np.integer):
        raise ValueError(f'igm: fragments must be {int(n_atoms)} integers, one per atom (got {fr.dtype} of shape {fr.shape})')
    if fr.size and int(fr.min()) < -1:
        raise ValueError(f'igm: fragment {int(fr.min())}; -1 (in no fragment) is the least')
    F = max(int(fr.max()) + 1 if fr.size else 1, 1)
    if F > _lib.XB_IGM_FRAGMENTS_MAX:
        raise ValueError(f'igm: {F} fragments; at most {_lib.XB_IGM_FRAGMENTS_MAX} are supported')
    return np.ascontiguousarray(fr, dtype=np.int32), F


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f"igm: mode {mode!r}; 'pro' or 'stockholder' is wanted")
    return MODES[mode]


def _check_floor(p_min):
    if not (math.isfinite(float(p_min)) and float(p_min) >= 0.0):
        raise ValueError(f'igm: p_min = {p_min}; a finite number >= 0 is wanted')


def _check_cut(who, cut):
    if not (math.isfinite(float(cut)) and float(cut) > 0.0):
        raise ValueError(f'{who}: the bound on delta-g_inter must be finite and above 0')


def _setup(density, lattice, atoms, species, proatoms, isa):
    """the default context with the table setup of these arguments current and `density` resident"""
    if (isa is None) == (proatoms is None):
        raise ValueError('igm: give either species and proatoms (a hirshfeld.ProAtoms) or isa (an isa.IsaResult)')
    if isa is not None:
        from .isa import _context
        ctx = _context(density)
        ctx.isa_setup(lattice, atoms, isa.r_cut, isa.shells, isa.rho_bound, isa.tables)   # (as isa_promolecule loads them)
    else:
        from .hirshfeld import _setup as hirshfeld_setup
        if species is None:
            raise ValueError('igm: proatoms need species (int[n_atoms])')
        ctx = hirshfeld_setup(density, lattice, atoms, species, proatoms)
    ensure_density(ctx, density)
    return ctx


def _device_fields(density, lattice, atoms, fragments, species, proatoms, isa, mode, p_min, full_search, want_dg, colour):
    """-> (ctx, dg, dgi, x) left on the device (dg None unless wanted, x None without colour)"""
    at = np.ascontiguousarray(atoms, dtype=np.float64).reshape(-1, 3)
    fr, F = check_fragments(fragments, at.shape[0])
    code = _mode(mode)
    _check_floor(p_min)
    ctx = _setup(density, lattice, at, species, proatoms, isa)
    dg, dgi, _ = ctx.igm_field(lattice, fr, code, p_min, full_search, on_device=True, want=(want_dg, True), n_fragments=F)
    x = ctx.nci_field(lattice, on_device=True)[1] if colour else None
    return ctx, dg, dgi, x


def igm_fields(density, lattice, atoms, fragments, species=None, proatoms=None, isa=None, mode='stockholder', p_min=P_MIN,
               full_search=False, colour=True):
    """(dg, dg_inter, x): delta-g, delta-g_inter and sign(lambda2) rho of `density` (host array, or a float32 / float64 device
    array) at every voxel, float64: host arrays for a host density, device.DeviceArrays for a device one.

    lattice      the CELL's lattice, one row per axis
    atoms        [n, 3] Cartesian, already `atoms - voxel_offset`; taken as given, not wrapped
    fragments    int[n]: the fragment 0 .. F - 1 of every atom, F <= 4, or -1 for an atom that is in none (it still enters the
                 promolecular density P and its gradient)
    species, proatoms   the free atoms (hirshfeld.ProAtoms) and the row each atom takes; or
    isa          an isa.IsaResult: its converged tables are loaded as isa_promolecule loads them
    mode         'stockholder' (IGMH: the gradients of w_a rho) or 'pro' (the free atoms' own gradients)
    p_min        both fields are +0 where the promolecular density P is not above it.  The default 1e-6 is a choice, not a
                 measurement
    full_search  every tile runs over the whole image list: the second implementation, the same bits
    colour       without it x is None and is not computed (x is the second field of nci.nci_fields)"""
    at = np.ascontiguousarray(atoms, dtype=np.float64).reshape(-1, 3)
    fr, F = check_fragments(fragments, at.shape[0])
    code = _mode(mode)
    _check_floor(p_min)
    ctx = _setup(density, lattice, at, species, proatoms, isa)
    on_device = device.is_device_array(density)
    dg, dgi, _ = ctx.igm_field(lattice, fr, code, p_min, full_search, on_device=on_device, n_fragments=F)
    x = ctx.nci_field(lattice, on_device=on_device)[1] if colour else None
    return dg, dgi, x


class IgmRegions:
    """The region delta-g_inter >= cut per label and class (CLASSES: attractive, van der Waals, repulsive by sign(lambda2) rho):

    count     int64[n, 3]   voxels
    volume    f64[n, 3]     count * voxel_volume
    charge    f64[n, 3]     the integral of rho: the electrons in the region
    integral  f64[n, 3]     the integral of delta-g_inter: what IGMPlot and Multiwfn print as the strength of the contact
    cut, rho_split, mode, p_min   what they were made with"""

    def __init__(self, count, charge, integral, voxel_volume, cut, rho_split, mode, p_min):
        self.count, self.charge, self.integral = count, charge, integral
        self.volume = count.astype(np.float64) * float(voxel_volume)
        self.cut, self.rho_split, self.mode, self.p_min = float(cut), float(rho_split), mode, float(p_min)


def igm_regions(density, volumes, lattice, atoms, fragments, n, voxel_volume, cut=DG_CUT, rho_split=RHO_SPLIT, species=None,
                proatoms=None, isa=None, mode='stockholder', p_min=P_MIN, full_search=False):
    """The region delta-g_inter >= cut of `density` summed over the voxels of every label 0 .. n - 1 of `volumes` (host or device
    array; labels < 0 and >= n are skipped) and every class.  The region is decided on the stored field, so it is that of
    igm_fields, igm_domains and igm_isosurface.  -> IgmRegions"""
    _check_cut('igm_regions', cut)
    shape = tuple(int(s) for s in density.shape)
    if tuple(int(s) for s in volumes.shape) != shape:
        raise ValueError(f'igm_regions: the label map has shape {tuple(volumes.shape)}, the density {shape}')
    ctx, _, dgi, x = _device_fields(density, lattice, atoms, fragments, species, proatoms, isa, mode, p_min, full_search, False, True)
    if int(n) < 1:
        return IgmRegions(np.zeros((0, 3), np.int64), np.zeros((0, 3)), np.zeros((0, 3)), voxel_volume, cut, rho_split, mode, p_min)
    ensure_labels(ctx, volumes)
    count, charge, integral = ctx.igm_sum(dgi, x, n, voxel_volume, cut, rho_split)
    return IgmRegions(count, charge, integral, voxel_volume, cut, rho_split, mode, p_min)


def igm_isosurface(density, lattice, atoms, fragments, level=DG_CUT, species=None, proatoms=None, isa=None, mode='stockholder',
                   p_min=P_MIN, full_search=False):
    """The surface delta-g_inter = `level` of `density` (host or device array), coloured by sign(lambda2) rho -- the picture of
    IGM.  Inside, in the sense of isosurface.Mesh, is delta-g_inter >= level: the region of igm_regions and igm_domains.  The two
    fields are made and read on the device, whichever side `density` lives on.  -> isosurface.Mesh"""
    from .isosurface import Mesh
    _check_cut('igm_isosurface', level)
    ctx, _, dgi, x = _device_fields(density, lattice, atoms, fragments, species, proatoms, isa, mode, p_min, full_search, False, True)
    out = ctx.isosurface(lattice, level, dgi, x, 0)
    ctx.isosurface_release()
    return Mesh(tuple(int(s) for s in density.shape), level, lattice, *out)


class IgmDomains(Regions):
    """The connected pieces of the region delta-g_inter >= level under the adjacency of pybader_amd.regions, numbered 0 .. m - 1
    in ascending seed -- one per contact between fragments.  A regions.Regions (labels, seed, voxel, count, volume, top, charge,
    charge2, shares, atoms: the two labels of `volumes` the piece lies between; top, charge and charge2 are taken of the density)
    and:

    value      f64[m]        delta-g_inter at `top`, the domain's densest voxel
    integral   f64[m]        the integral of delta-g_inter over the domain
    kind       int8[m]       the class of `top` by sign(lambda2) rho against rho_split (CLASSES): what the domain is called
    level, rho_split, mode, p_min   what they were made with"""

    def __init__(self, regions, value, integral, kind, level, rho_split, mode, p_min):
        self.__dict__.update(vars(regions))
        self.value, self.integral, self.kind = value, integral, kind
        self.level, self.rho_split, self.mode, self.p_min = float(level), float(rho_split), mode, float(p_min)


def igm_domains(density, lattice, atoms, fragments, volumes=None, n=0, voxel_volume=1.0, level=DG_CUT, rho_split=RHO_SPLIT,
                species=None, proatoms=None, isa=None, mode='stockholder', p_min=P_MIN, full_search=False):
    """The region delta-g_inter >= level of `density` (host or device array) split into its connected domains, each with its
    voxels, the integrals of the density and of delta-g_inter over it; with a label map `volumes` and n >= 1 also which labels
    0 .. n - 1 every domain lies between.  delta-g_inter is made on the device and handed to regions.connected_regions as it is:
    the pieces are those of the field, the sums and the surface.  The integral per domain is xb_igm_sum with the domains' own map
    as the labels (it becomes the resident label map).  The labels are a host array for a host density.  -> IgmDomains"""
    from .regions import connected_regions
    _check_cut('igm_domains', level)
    ctx, _, dgi, x = _device_fields(density, lattice, atoms, fragments, species, proatoms, isa, mode, p_min, full_search, False, True)
    r = connected_regions(dgi, level, density=density, voxel_volume=voxel_volume, volumes=volumes, n=n)
    if r.m:
        ensure_labels(ctx, r.labels)
        _, _, per_class = ctx.igm_sum(dgi, x, r.m, voxel_volume, level, rho_split)
        integral = (per_class[:, 0] + per_class[:, 1]) + per_class[:, 2]
        value = dgi.to_host().reshape(-1)[r.top]
        xt = x.to_host().reshape(-1)[r.top]
        kind = np.where(xt < -float(rho_split), 0, np.where(xt > float(rho_split), 2, 1)).astype(np.int8)
    else:
        value, integral, kind = np.zeros(0), np.zeros(0), np.zeros(0, np.int8)
    if not device.is_device_array(density):
        r.labels = r.labels.to_host()
    return IgmDomains(r, value, integral, kind, level, rho_split, mode, p_min)

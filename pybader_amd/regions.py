"""Connected regions of a field on the periodic grid -- no counterpart in the reference.  How many pieces a level set has and what
each holds: the molecules inside the 0.001 envelope of a density, the pores of a framework (the pockets below a level), and --
through nci.nci_domains -- the single contacts of the NCI region, each with its size, its integral and the atoms it lies between.

Two voxels are neighbours along the 14 offsets of the Freudenthal triangulation of critical.py and isosurface.py, so the components
of {field >= level} are exactly the pieces the marching-tetrahedra surface encloses.  A component's seed is its smallest linear
C-order index and the components are numbered in ascending seed: every integer output is unique, whatever the schedule.  It runs
in libbader_hip.so (xb_regions_label / xb_regions_sums / xb_regions_shares, csrc/k_regions.h): a union-find per 8 x 8 x 32 tile in
LDS, a lock-free merge across the tiles' faces and the periodic wrap, a flatten; `global_route` takes the second implementation
(every union in global memory): the same map.  The definition is in include/bader_hip.h and DESIGN.md section 22, and
tests/test_regions_cpu.py restates it in numpy.

    connected_regions(field, level, below=False, density=None, voxel_volume=1.0, volumes=None, n=0)    a Regions"""
import numpy as np

from . import _lib, device
from .laplacian import _resident
from .utils import ensure_labels


def atoms_from_shares(m, shares):
    """int64[m, 2]: per component the two labels with the largest counts among the triplets `shares` (component, label, count),
    ties to the smaller label, -1 where a component touches fewer"""
    comp, lab, cnt = (np.asarray(a, dtype=np.int64).reshape(-1) for a in shares)
    out = np.full((int(m), 2), -1, np.int64)
    order = np.lexsort((lab, -cnt, comp))      # by component, then the largest count first, then the smaller label
    comp, lab = comp[order], lab[order]
    first = np.flatnonzero(np.r_[True, comp[1:] != comp[:-1]]) if comp.size else np.zeros(0, np.int64)
    out[comp[first], 0] = lab[first]
    second = first + 1
    second = second[(second < comp.size)]
    second = second[comp[second] == comp[second - 1]]
    out[comp[second], 1] = lab[second]
    return out


def _shares(ctx, shape, volumes, n, force_list, who):
    """the triplets of the last labelling against the label map `volumes`, or three empty arrays without one"""
    n = int(n)
    if volumes is None or n < 1:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    if tuple(int(s) for s in volumes.shape) != shape:
        raise ValueError(f'{who}: the label map has shape {tuple(volumes.shape)}, the field {shape}')
    ensure_labels(ctx, volumes)
    return ctx.regions_shares(n, force_list)


class Regions:
    """The connected components of a mask of the grid, numbered 0 .. m - 1 in ascending seed:

    shape, m
    labels     int32 of the grid's shape: the component of every voxel, -1 outside (a host array for a host field, a
               device.DeviceArray for a device field)
    seed       int64[m]      the smallest linear C-order index of the component
    voxel      int64[m, 3]   the same as grid coordinates
    count      int64[m]      voxels
    volume     f64[m]        count * voxel_volume
    top        int64[m]      the greatest voxel of the density in the component, in the order of critical.critical_points
    charge     f64[m]        the integral of the density over the component
    charge2    f64[m]        the integral of its square
    shares     (component int32[t], label int32[t], count int64[t]): the voxels per component and label of `volumes`, count > 0,
               ascending in (component, label); empty without a label map
    atoms      int64[m, 2]   the two labels with the largest counts, ties to the smaller label, -1 where there are fewer"""

    def __init__(self, shape, labels, seed, count, top, charge, charge2, shares, voxel_volume):
        self.shape, self.m = tuple(int(s) for s in shape), int(seed.shape[0])
        self.labels, self.seed, self.count, self.top, self.charge, self.charge2, self.shares = labels, seed, count, top, charge, charge2, shares
        self.voxel = np.stack(np.unravel_index(seed, self.shape), axis=1).astype(np.int64).reshape(-1, 3)
        self.volume = count.astype(np.float64) * float(voxel_volume)
        self.atoms = atoms_from_shares(self.m, shares)

    def __len__(self):
        return self.m


def connected_regions(field, level, below=False, density=None, voxel_volume=1.0, volumes=None, n=0, global_route=False,
                      shares_list=False):
    """The connected components of {field >= level}, or with `below` of {field < level}; a NaN is outside either.

    field         host array, or a float32 / float64 device array: it becomes the resident density, as in the other analyses --
                  unless `density` names the resident one (inside utils.resident() nothing is uploaded again); then `field` is
                  another field on the same grid: a float64 C-contiguous device array is read where it is, a host array goes
                  through a scratch upload
    density       what top, charge and charge2 are taken of; `field` itself by default
    volumes, n    with n >= 1: the label map (host or device) whose labels 0 .. n - 1 the shares are counted against
    global_route  the second implementation (every union in global memory): the same results
    shares_list   the shares by the route of the large case (a sorted key list instead of a dense table): the same triplets

    -> Regions"""
    ctx, shape = _resident(field if density is None else density)
    fdev = None
    if density is not None:
        if tuple(int(s) for s in field.shape) != shape:
            raise ValueError(f'connected_regions: the field has shape {tuple(field.shape)}, the density {shape}')
        if device.is_device_array(field):
            fdev = field
        else:
            fdev = ctx.device_copy(np.ascontiguousarray(field, dtype=np.float64))
    m = ctx.regions_label(_lib.XB_DOMAINS_BELOW if below else _lib.XB_DOMAINS_ABOVE, fdev, level, global_route=global_route)
    try:
        labels = ctx.regions_map(on_device=device.is_device_array(field))
        seed, count, top, s1, s2 = ctx.regions_sums(m, voxel_volume)
        shares = _shares(ctx, shape, volumes, n, shares_list, 'connected_regions')
    finally:
        ctx.regions_release()      # (the map does not outlive the call, whichever way it ends)
    return Regions(shape, labels, seed, count, top, s1, s2, shares, voxel_volume)

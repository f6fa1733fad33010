"""The weight method of grid-based Bader analysis (Yu & Trinkle, J. Chem. Phys. 134, 064111, 2011; `bader -b weight` in the
Henkelman group's code): charge and volume per maximum with the surface voxels split fractionally.  Neither pybader nor the
on-grid / near-grid path of this library has it; it sits next to utils.charge_sum and changes none of their results.

    voronoi_weights(voxel_lattice)   the 26 neighbour weights alpha_d = facet area / distance (host, float64)
    weight_sum(reference, density, lattice, volumes=None)   (maxima, charge, volume) on the GPU (csrc/k_weight.h)

The definition (flux, accumulation, neighbour order, vacuum) is in DESIGN.md and in include/bader_hip.h at xb_weight_sum."""
import itertools

import numpy as np

from . import _lib, device
from .utils import ensure_density, ensure_labels

AREA_TOL = 1e-10          # a facet below AREA_TOL * V_voxel^(2/3) is a line or a point: its weight is 0


def _clip(poly, normal, offset):
    """the part of the convex polygon `poly` (k x 3) with x . normal <= offset (Sutherland-Hodgman)"""
    if len(poly) == 0:
        return poly
    d = poly @ normal - offset
    out = []
    for k in range(len(poly)):
        a, b, da, db = poly[k], poly[(k + 1) % len(poly)], d[k], d[(k + 1) % len(poly)]
        if da <= 0:
            out.append(a)
        if (da < 0 < db) or (db < 0 < da):
            out.append(a + (b - a) * (da / (da - db)))
    return np.array(out).reshape(-1, 3)


def _area(poly):
    if len(poly) < 3:
        return 0.0
    s = np.zeros(3)
    for k in range(1, len(poly) - 1):
        s += np.cross(poly[k] - poly[0], poly[k + 1] - poly[0])
    return 0.5 * float(np.linalg.norm(s))


def _facet_area(r, others):
    """area of the facet the bisector plane of `r` contributes to the cell cut out by the bisector planes of `others`"""
    l2 = float(r @ r)
    n = r / np.sqrt(l2)
    u = np.cross(n, np.eye(3)[np.argmin(np.abs(n))])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    big = 4.0 * max(np.sqrt(float(o @ o)) for o in others)
    c = 0.5 * r
    poly = np.array([c + big * (su * u + sv * v) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    for o in others:
        poly = _clip(poly, o, 0.5 * float(o @ o))
        if len(poly) < 3:
            return 0.0
    return _area(poly)


def _pair_offsets():
    """one offset of each +-d pair of {-1, 0, 1}^3 \\ {0}: the 13 with d > -d, in ascending tuple order"""
    return [d for d in itertools.product(range(-1, 2), repeat=3) if d > tuple(-x for x in d)]


def voronoi_areas(voxel_lattice, who='voronoi_areas'):
    """area[i, j, k] = a_d for the 26 offsets d in {-1, 0, 1}^3 \\ {0}: the area of the facet the bisector plane of r_d = d . L
    contributes to the Voronoi (Wigner-Seitz) cell of the voxel lattice L (one row per axis).  Indexed like
    voronoi_weights; a facet below AREA_TOL * V_voxel^(2/3) is 0; a_d == a_{-d} exactly (computed once per pair).  Raises
    ValueError as voronoi_weights does (which divides these areas by |r_d|)."""
    L = np.asarray(voxel_lattice, dtype=np.float64).reshape(3, 3)
    vol = abs(float(np.linalg.det(L)))
    if not np.isfinite(vol) or vol == 0.0:
        raise ValueError(f'{who}: the voxel lattice is singular')
    tol = AREA_TOL * vol ** (2.0 / 3.0)
    offsets = [d for d in itertools.product(range(-2, 3), repeat=3) if d != (0, 0, 0)]
    vec = {d: np.array(d, dtype=np.float64) @ L for d in offsets}
    areas = np.zeros((3, 3, 3), dtype=np.float64)
    for d in offsets:
        if d < tuple(-x for x in d):          # one of each +-d pair
            continue
        r = vec[d]
        area = _facet_area(r, [vec[o] for o in offsets if o != d])
        if area < tol:
            continue
        if max(abs(x) for x in d) > 1:
            raise ValueError(f'{who}: the offset {d} contributes a facet to the Voronoi cell of the voxel lattice: '
                             'it is too skewed for the 26-neighbour stencil')
        areas[tuple(x % 3 for x in d)] = area
        areas[tuple(-x % 3 for x in d)] = area
    return areas


def voronoi_weights(voxel_lattice):
    """alpha[i, j, k] = a_d / |r_d| for the 26 offsets d in {-1, 0, 1}^3 \\ {0}: r_d = d . L, a_d the area of the facet the
    bisector plane of r_d contributes to the Voronoi (Wigner-Seitz) cell of the voxel lattice L (one row per axis).
    Indexed like distance_matrix: index 0 is step 0, 1 is step +1, 2 is step -1; the centre is 0.  A facet below
    1e-10 * V_voxel^(2/3) -- the edge and corner neighbours of an orthogonal cell touch it in a line or a point -- gets
    weight 0.  alpha_d == alpha_{-d} exactly (computed once per pair).

    The cell is cut out by the bisector planes of all offsets in {-2..2}^3; a facet from an offset outside {-1, 0, 1}^3
    raises ValueError: the voxel lattice is too skewed for a 26-neighbour stencil (reduce the cell first)."""
    L = np.asarray(voxel_lattice, dtype=np.float64).reshape(3, 3)
    areas = voronoi_areas(L, 'voronoi_weights')
    alpha = np.zeros((3, 3, 3), dtype=np.float64)
    for d in _pair_offsets():
        area = areas[tuple(x % 3 for x in d)]
        if area == 0.0:
            continue
        r = np.array(d, dtype=np.float64) @ L
        a = area / float(np.sqrt(r @ r))
        alpha[tuple(x % 3 for x in d)] = a
        alpha[tuple(-x % 3 for x in d)] = a
    return alpha


def _same_field(a, b):
    """is `a` the very array `b` (then the resident copy serves as the integrand)"""
    if a is b:
        return True
    if device.is_device_array(a) or device.is_device_array(b):
        return (device.is_device_array(a) and device.is_device_array(b)
                and device.describe(a).identity == device.describe(b).identity)
    return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
            and a.strides == b.strides and a.ctypes.data == b.ctypes.data)


def weight_sum(reference, density, lattice, volumes=None):
    """Weight-method charge and volume of every maximum of `reference`.

    reference   the partition field rho (host array, or a float32 / float64 device array)
    density     the field to integrate, of the same shape: `reference` itself, or another one (charge with a separate
                reference, spin); host or device array
    lattice     the CELL's lattice, one row per axis; the voxel lattice is row i divided by shape[i]
    volumes     None, or a label map whose -1 marks are vacuum: such a voxel is absent (no maximum, sends and receives
                nothing).  Its other labels are not read.

    -> (maxima int64[M, 3] voxel indices in C-order scan order, charge f64[M], volume f64[M]).  Bit-identical to a plain
    float64 loop over the voxels in ascending `reference` (tests/test_weight_cpu.py restates it)."""
    ctx = _lib.default_context()
    shape = tuple(int(n) for n in reference.shape)
    if tuple(int(n) for n in density.shape) != shape:
        raise ValueError(f'weight_sum: reference has shape {shape}, density {tuple(density.shape)}')
    lattice = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    voxel_lattice = lattice / np.array(shape, dtype=np.float64)[:, None]
    voxel_volume = np.abs(np.dot(lattice[0], np.cross(*lattice[1:]))) / np.prod(shape)
    alpha = voronoi_weights(voxel_lattice)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    same = _same_field(density, reference)
    ensure_density(ctx, reference)
    if volumes is not None:
        ensure_labels(ctx, volumes)
    # (without a map the resident labels, whatever they are, are neither read nor written)
    idx, charge, volume = ctx.weight_sum(alpha, voxel_volume, None if same else density, use_labels=volumes is not None)
    maxima = np.stack(np.unravel_index(idx, shape), axis=1).astype(np.int64) if idx.size else np.zeros((0, 3), np.int64)
    return maxima, charge, volume

"""The Laplacian and the Hessian of the density -- no counterpart in the reference.  Two questions of a QTAIM analysis rest on
them: what kind of bond a bond point marks (the sign of the Laplacian there tells a shared-shell from a closed-shell interaction,
the Hessian's eigenvalues give the ellipticity, and a shallow saddle of the tails has eigenvalues near zero), and how good the
integration is (L = the integral of the Laplacian over a basin vanishes over an exact zero-flux basin: the figure of merit AIM
codes print next to the charge).

One compact second-order stencil on 19 points serves all of it; it runs in libbader_hip.so (xb_laplacian_field,
xb_laplacian_sum, xb_stencil_points, csrc/k_stencil.h).  The definition is in include/bader_hip.h and DESIGN.md section 18, and
tests/test_laplacian_cpu.py restates it in numpy.  Every value at a voxel is bit-defined; the sums per basin are float atomics in
any order.

    laplacian(density, lattice)                                      the field
    basin_laplacian(density, volumes, lattice, n, voxel_volume)      (L, L_abs, volume) per label
    point_properties(density, lattice, voxels)                       a PointProperties"""
import numpy as np

from . import _lib, device
from .utils import ensure_density, ensure_labels

_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # the six Hessian components of a row of xb_stencil_points
_EDGES = ((0, 1), (0, 2), (1, 2))                               # the mixed terms of the stencil


def _resident(density):
    ctx = _lib.default_context()
    shape = tuple(int(s) for s in density.shape)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    return ctx, shape


def laplacian(density, lattice, gather=False):
    """The Laplacian of `density` (host array, or a float32 / float64 device array) in the cell `lattice` (a row per axis) at
    every voxel, float64: a host array for a host density, a device.DeviceArray for a device density.  `gather` takes the second
    implementation (one thread per voxel reading global memory instead of tiles in LDS): the same bits.  Inside
    utils.resident() nothing is uploaded again."""
    ctx, _ = _resident(density)
    return ctx.laplacian_field(lattice, gather, on_device=device.is_device_array(density))


def basin_laplacian(density, volumes, lattice, n, voxel_volume, gather=False):
    """The Laplacian of `density` summed over the voxels of every label 0 .. n - 1 of `volumes` (host or device array; labels
    < 0 and >= n are skipped), each sum multiplied once by `voxel_volume`.

    -> (L f64[n], L_abs f64[n], volume f64[n]): L is the integral of the Laplacian over the basin -- zero for an exact zero-flux
    basin --, L_abs the integral of its magnitude, the scale |L| is read against."""
    ctx, shape = _resident(density)
    if tuple(int(s) for s in volumes.shape) != shape:
        raise ValueError(f'basin_laplacian: the label map has shape {tuple(volumes.shape)}, the density {shape}')
    ensure_labels(ctx, volumes)
    if int(n) < 1:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    return ctx.laplacian_sum(lattice, n, voxel_volume, gather)


class PointProperties:
    """The density and its derivatives at listed voxels:

    shape          the grid
    lin            int64[m]       linear C-order index;  voxels int64[m, 3]
    rho            f64[m]
    gradient       f64[m, 3]      Cartesian, central differences
    hessian        f64[m, 3, 3]   Cartesian, symmetric
    laplacian      f64[m]         the bit-defined value of the field at the voxel (from the Laplacian's own coefficients, not the
                                  Hessian's trace, which differs from it in the last bits)
    eigenvalues    f64[m, 3]      of the Hessian, ascending (numpy.linalg.eigvalsh on the host)
    ellipticity    f64[m]         l1 / l2 - 1 where l1 <= l2 < 0 (the two curvatures across a bond path), NaN elsewhere
    signature      int64[m]       the sum of the eigenvalues' signs: -3 a maximum, -1 a bond point, +1 a ring point, +3 a cage point"""

    def __init__(self, shape, lin, values, lap):
        self.shape = tuple(int(s) for s in shape)
        self.lin = lin
        self.voxels = np.stack(np.unravel_index(lin, self.shape), axis=1).astype(np.int64).reshape(-1, 3)
        self.rho = np.ascontiguousarray(values[:, 0])
        self.gradient = np.ascontiguousarray(values[:, 1:4])
        self.hessian = np.empty((lin.shape[0], 3, 3), np.float64)
        for k, (i, j) in enumerate(_PAIRS):
            self.hessian[:, i, j] = values[:, 4 + k]
            self.hessian[:, j, i] = values[:, 4 + k]
        self.laplacian = lap
        self.eigenvalues = np.linalg.eigvalsh(self.hessian) if lin.shape[0] else np.zeros((0, 3))
        l1, l2 = self.eigenvalues[:, 0], self.eigenvalues[:, 1]
        self.ellipticity = np.full(lin.shape[0], np.nan)
        across = l2 < 0
        self.ellipticity[across] = l1[across] / l2[across] - 1.0
        self.signature = np.sign(self.eigenvalues).sum(axis=1).astype(np.int64)

    def __len__(self):
        return self.lin.shape[0]


def _neighbour_indices(vox, shape):
    """the linear indices of the 19 stencil points of each voxel, [19, m]: the voxel, (+i, -i) per axis, then per edge term ij
    (+i+j, +i-j, -i+j, -i-j); every coordinate wrapped"""
    n = np.array(shape, dtype=np.int64)
    steps = [(0, 0, 0)]
    for i in range(3):
        for s in (1, -1):
            d = [0, 0, 0]
            d[i] = s
            steps.append(tuple(d))
    for i, j in _EDGES:
        for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            d = [0, 0, 0]
            d[i], d[j] = si, sj
            steps.append(tuple(d))
    out = np.empty((len(steps), vox.shape[0]), np.int64)
    for k, d in enumerate(steps):
        p = (vox + np.array(d, dtype=np.int64)) % n
        out[k] = (p[:, 0] * n[1] + p[:, 1]) * n[2] + p[:, 2]
    return out


def _laplacian_at(rho19, w):
    """the Laplacian of the definition from the 19 densities of _neighbour_indices ([19, m]) and the six coefficients, every
    operation in the order the definition writes: the bits of the field"""
    c = rho19[0]
    d = [(rho19[1 + 2 * i] - c) + (rho19[2 + 2 * i] - c) for i in range(3)]
    for k in range(3):
        pp, pm, mp, mm = rho19[7 + 4 * k: 11 + 4 * k]
        d.append((pp - pm) - (mp - mm))
    lap = w[0] * d[0] + w[1] * d[1]
    for k in range(2, 6):
        lap = lap + w[k] * d[k]
    return lap


def point_properties(density, lattice, voxels):
    """rho, its gradient, its Hessian and what follows from them at `voxels` (int[m, 3], or linear C-order indices int[m]) of
    `density` (host array, or a float32 / float64 device array) in the cell `lattice`.  -> PointProperties.

    The library's call gives ten values per voxel; the Laplacian is formed here from the densities of the voxel's 19 stencil
    points (the same call on those voxels) with the coefficients of _lib.stencil_coeffs, operation by operation as the field
    kernel forms it."""
    ctx, shape = _resident(density)
    v = np.asarray(voxels, dtype=np.int64)
    if v.ndim == 2:
        if v.shape[1] != 3:
            raise ValueError(f'point_properties: voxels of shape {v.shape}; [m, 3] or [m] is wanted')
        if v.size and (v.min() < 0 or (v >= np.array(shape)).any()):
            raise ValueError('point_properties: a voxel lies outside the grid')
        lin = np.ravel_multi_index(v.T, shape).astype(np.int64) if v.size else np.zeros(0, np.int64)
    else:
        lin = np.ascontiguousarray(v.reshape(-1))
    values = ctx.stencil_points(lattice, lin)
    if lin.shape[0] == 0:
        return PointProperties(shape, lin, values, np.zeros(0))
    vox = np.stack(np.unravel_index(lin, shape), axis=1).astype(np.int64)
    idx = _neighbour_indices(vox, shape)
    rho19 = ctx.stencil_points(lattice, idx.reshape(-1))[:, 0].reshape(idx.shape)
    _, w, _ = _lib.stencil_coeffs(lattice, shape)
    return PointProperties(shape, lin, values, _laplacian_at(rho19, w))
